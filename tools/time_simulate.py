"""Rate of the read simulator (covest_simulate_reads_device, sim_reads.hip) against the torch generator of
bench.py's bench_kmer (copied below as it stands there) and against hipMemsetAsync on the same buffer, in one run:
10^8 and 10^9 bases of 100-bp reads from a 25 Mbp genome, 1 % substitutions.  HIP events on the stream, after a
spin-up; per case the median of N timed repetitions, the three routes taking turns.  Reported only: there is no bar.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/time_simulate.py [--reps 7] [--out profiles/simulate_rate.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from covest_amd import _capi, simulate as sim  # noqa: E402

GENOME_LEN, READ_LEN, ERROR_RATE, SEED = 25_000_000, 100, 0.01, 20240601


def torch_route(reads, genome, lut, ar, gen, n_reads, dev):
    """The generator of bench_kmer (bench.py), reads only: the genome is made before the clock starts on either route."""
    read_len, genome_len = READ_LEN, genome.numel()
    chunk = 2_000_000
    for a in range(0, n_reads, chunk):
        b = min(n_reads, a + chunk)
        starts = torch.randint(0, genome_len - read_len, (b - a,), device=dev, generator=gen)
        r = genome[starts[:, None] + ar[None, :]]
        err = torch.rand(r.shape, device=dev, generator=gen) < 0.01
        r = torch.where(err, lut[torch.randint(0, 4, r.shape, device=dev, generator=gen)], r)
        reads[a * read_len:b * read_len] = r.reshape(-1)


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "simulate_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_simulate.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.lib()
    runtimes = _capi.hip_runtimes_mapped()
    hip = ctypes.CDLL(runtimes[0])  # the runtime torch brought: already mapped
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    genome = torch.empty(GENOME_LEN, dtype=torch.uint8, device=dev)
    sim.random_genome_device(genome.data_ptr(), GENOME_LEN, SEED, stream=stream)
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    ar = torch.arange(READ_LEN, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)

    lines = ["# read simulator: GB/s of output (bases), median of %d; 100-bp reads, 25 Mbp genome, e = 0.01; %s"
             % (args.reps, torch.cuda.get_device_name(0)),
             "# %-12s %12s %12s %12s %16s %16s" % ("bases", "kernel GB/s", "memset GB/s", "torch GB/s", "kernel / memset",
                                                   "kernel / torch")]
    for n_bases in (10 ** 8, 10 ** 9):
        n_reads = n_bases // READ_LEN
        reads = torch.empty(n_bases, dtype=torch.uint8, device=dev)

        def kernel():
            sim.simulate_reads_device(genome.data_ptr(), GENOME_LEN, READ_LEN, n_reads, reads.data_ptr(),
                                      error_rate=ERROR_RATE, seed=SEED, stream=stream)

        def memset():
            if hip.hipMemsetAsync(reads.data_ptr(), 0x41, n_bases, stream) != 0:
                raise SystemExit("hipMemsetAsync failed")

        def torch_gen():
            torch_route(reads, genome, lut, ar, gen, n_reads, dev)

        routes = (("kernel", kernel), ("memset", memset), ("torch", torch_gen))
        for _, fn in routes:  # spin-up: code objects loaded, the allocator's blocks in place, clocks up
            for _ in range(3):
                fn()
        for _ in range(20):
            kernel()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                ms[name].append(timed_ms(fn))
        rate = {name: n_bases / (statistics.median(t) * 1e-3) / 1e9 for name, t in ms.items()}
        lines.append("  %-12d %12.1f %12.1f %12.1f %16.3f %16.1f" % (n_bases, rate["kernel"], rate["memset"], rate["torch"],
                                                                    rate["kernel"] / rate["memset"],
                                                                    rate["kernel"] / rate["torch"]))
        del reads
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
