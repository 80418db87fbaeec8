"""Rate of the repeat-genome kernel (covest_repeat_genome_device, sim_repeats.hip) beside covest_random_genome_device
into the same buffer, in one run: 10^9 bases at divergence 0 and 0.05, units of 1000 and of 101 bases.  The random
genome is the yardstick -- the same Philox work a base at divergence 0.  HIP events on the stream, after a spin-up; per
case the median of N timed repetitions, the routes taking turns.  Reported only: there is no bar.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/time_repeat.py [--reps 7] [--out profiles/repeat_rate.txt]
"""
import argparse
import os
import statistics
import sys

import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from covest_amd import _capi, simulate as sim  # noqa: E402

N_BASES, SEED = 10 ** 9, 20240601
Q = (0.7, 0.5, 0.5)


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "repeat_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_repeat.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.lib()
    out = torch.empty(N_BASES, dtype=torch.uint8, device=dev)

    def random_genome():
        sim.random_genome_device(out.data_ptr(), N_BASES, SEED, stream=stream)

    lines = ["# repeat genome: GB/s of output (bases), median of %d; %d bases, (q1, q2, q) = (%g, %g, %g); %s"
             % ((args.reps, N_BASES) + Q + (torch.cuda.get_device_name(0),)),
             "# %-9s %-11s %14s %16s %10s" % ("unit_len", "divergence", "repeat GB/s", "random_genome GB/s", "ratio")]
    for unit_len in (1000, 101):
        n_units = -(-N_BASES // unit_len)
        plan, _ = sim.repeat_plan(n_units, *Q, seed=SEED)
        d_plan = torch.from_numpy(plan).to(dev)
        for divergence in (0.0, 0.05):
            def repeat():
                sim.repeat_genome_device(d_plan.data_ptr(), n_units, unit_len, N_BASES, out.data_ptr(),
                                         divergence=divergence, seed=SEED, stream=stream)

            routes = (("repeat", repeat), ("random", random_genome))
            for _, fn in routes:  # spin-up: code objects loaded, clocks up
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in routes}
            for _ in range(args.reps):
                for name, fn in routes:
                    ms[name].append(timed_ms(fn))
            rate = {name: N_BASES / (statistics.median(t) * 1e-3) / 1e9 for name, t in ms.items()}
            lines.append("  %-9d %-11g %14.1f %16.1f %10.3f" % (unit_len, divergence, rate["repeat"], rate["random"],
                                                              rate["repeat"] / rate["random"]))
        del d_plan
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
