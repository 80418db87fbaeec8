"""Latency of the truncated-Poisson entry points (covest_amd.poisson over tp_eval.hip): microseconds a call at 1, 256
and 10^6 pairs (value mode: the in-place route, its upper boundary, one copy either way), and for the recurrence
table over tp_table.json's distinct rates and keys (417 x 244: the table of tests/test_gpu_tp.py).  One process, one
device, after the spin-up the other timing tools use; per case the median and the fastest of N calls, every call
ending with its values on the host.  Reported only: there is no bar.

    python tools/time_tp.py [--calls 30] [--out profiles/tp_latency.txt]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from covest_amd import poisson  # noqa: E402
from time_hessian import spin_up, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tp_latency.txt"))
    args = ap.parse_args()
    rows = json.load(open(os.path.join(REPO, "tests", "golden", "tp_table.json")))["rows"]
    rates = np.array(sorted({r[0] for r in rows if r[0] > 0}))
    keys = np.array(sorted({r[1] for r in rows}), dtype=np.int64)
    rng = np.random.default_rng(1)
    l = rng.uniform(0.5, 400.0, 10 ** 6)
    j = rng.integers(1, 600, 10 ** 6)
    lines = ["# covest_truncated_poisson (value mode) and covest_truncated_poisson_table; microseconds a call, median "
             "(fastest) of %d" % args.calls,
             "# %-34s %14s %22s" % ("case", "values", "us a call")]
    cases = [("pairs, 1", 1, lambda: poisson.truncated_poisson_many(l[:1], j[:1])),
             ("pairs, 256 (in place)", 256, lambda: poisson.truncated_poisson_many(l[:256], j[:256])),
             ("pairs, 10^6", 10 ** 6, lambda: poisson.truncated_poisson_many(l, j)),
             ("table, %d rates x %d keys" % (len(rates), len(keys)), len(rates) * len(keys),
              lambda: poisson.truncated_poisson_table(rates, keys))]
    for name, n, fn in cases:
        spin_up(fn)
        t = timed(fn, args.calls)
        lines.append("  %-34s %14d %12.1f (%8.1f)" % (name, n, statistics.median(t), min(t)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
