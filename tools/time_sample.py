"""Rate of the read sampler (covest_sample_reads_device, sample_reads.hip) against a device-to-device hipMemcpyAsync
of bases_kept bytes (the floor: the gather reads and writes that much) and against the torch route (bases2d[mask], the
mask given), in one run: 100-bp reads, 10^8 and 10^9 input bases, factors 2 and 16.  HIP events on the stream after a
spin-up; per case the median of N timed repetitions (and, of the call's, the least and the most), the three routes
taking turns.  Reported only: there is no bar.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/time_sample.py [--reps 7] [--out profiles/sample_rate.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from covest_amd import _capi, sample  # noqa: E402

READ_LEN, SEED = 100, 20241018


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sample.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.lib()
    hip = ctypes.CDLL(_capi.hip_runtimes_mapped()[0])  # the runtime torch brought: already mapped
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    lines = ["# read sampler: GB/s of KEPT bytes, median of %d; 100-bp reads; %s" % (args.reps, torch.cuda.get_device_name(0)),
             "# %-12s %6s %12s %12s %12s %12s %14s %14s   %s" % ("input bases", "factor", "kept bytes", "call GB/s", "memcpy GB/s",
                                                                "torch GB/s", "call / memcpy", "call / torch",
                                                                "call ms: min median max")]
    for n_bases in (10 ** 8, 10 ** 9):
        n_reads = n_bases // READ_LEN
        reads = torch.randint(65, 85, (n_reads, READ_LEN), dtype=torch.uint8, device=dev)
        out = torch.empty(n_bases, dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        for factor in (2, 16):
            def call():
                sample.sample_reads_device(reads.data_ptr(), n_reads, out.data_ptr(), counts.data_ptr(), factor, seed=SEED,
                                           read_len=READ_LEN, stream=stream)

            call()
            n_kept, kept_bytes = counts.cpu().tolist()
            mask = torch.zeros(n_reads, dtype=torch.bool, device=dev)
            mask[torch.randperm(n_reads, device=dev)[:n_kept]] = True   # as many rows as the call keeps

            def memcpy():
                if hip.hipMemcpyAsync(out.data_ptr(), reads.data_ptr(), kept_bytes, 3, stream) != 0:
                    raise SystemExit("hipMemcpyAsync failed")

            def torch_route():
                return reads[mask]

            routes = (("call", call), ("memcpy", memcpy), ("torch", torch_route))
            for _, fn in routes:  # spin-up: code objects loaded, the allocators' blocks in place, clocks up
                for _ in range(3):
                    fn()
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in routes}
            for _ in range(args.reps):
                for name, fn in routes:
                    ms[name].append(timed_ms(fn))
            rate = {name: kept_bytes / (statistics.median(t) * 1e-3) / 1e9 for name, t in ms.items()}
            lines.append("  %-12d %6d %12d %12.1f %12.1f %12.1f %14.3f %14.1f   %.4f %.4f %.4f" % (
                n_bases, factor, kept_bytes, rate["call"], rate["memcpy"], rate["torch"], rate["call"] / rate["memcpy"],
                rate["call"] / rate["torch"], min(ms["call"]), statistics.median(ms["call"]), max(ms["call"])))
        del reads, out
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
