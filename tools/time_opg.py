"""Latency of one value+gradient+score-outer-product call (covest_eval_points_opg, ll_deriv.hip's third mode) on one
point, beside covest_eval_points_grad on the same point measured in the same process: the new mode is order 1's walk
plus 3 or 15 products a key and as many reductions, so K-grad is the reference.  One process, one device, after the
spin-up bench.py uses; per case the median and the fastest of N calls, each call ending in a synchronise (both entry
points wait for their stream), every route in a run of calls of its own; the grad column is measured twice, before and
after the opg column, and the second run's median is printed beside the first's as the run-to-run spread.

    python tools/time_opg.py [--calls 30] [--out profiles/opg_latency.txt]
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from bench import load_hist  # noqa: E402
from covest_amd import BasicModel, RepeatsModel  # noqa: E402
from time_hessian import CASES, spin_up, timed  # noqa: E402  (6f's four rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "opg_latency.txt"))
    args = ap.parse_args()
    lines = ["# one point: covest_eval_points_opg against covest_eval_points_grad; microseconds a call, median (fastest) of %d,"
             % args.calls,
             "# each route in a run of its own; grad again: the same route measured a second time, after the opg column",
             "# %-8s %-16s %6s %5s %20s %20s %12s %10s" % ("model", "histogram", "keys", "T", "opg, 1 point", "grad, 1 point",
                                                          "grad again", "opg / grad")]
    for kind, hname, tail, point in CASES:
        cls = RepeatsModel if kind == "repeats" else BasicModel
        m = cls(21, 100, load_hist(hname), tail, max_error=8)
        one = np.array([point], dtype=np.float64)
        T = int(m.get_hist_threshold_values([point[2:5]])[0]) if kind == "repeats" else 2
        spin_up(lambda: m.loglikelihood_gradient_points(one))
        t_g = timed(lambda: m.loglikelihood_gradient_points(one), args.calls)
        spin_up(lambda: m.loglikelihood_score_outer_points(one))
        t_b = timed(lambda: m.loglikelihood_score_outer_points(one), args.calls)
        spin_up(lambda: m.loglikelihood_gradient_points(one))
        t_g2 = timed(lambda: m.loglikelihood_gradient_points(one), args.calls)
        mb, mg = statistics.median(t_b), statistics.median(t_g)
        lines.append("  %-8s %-16s %6d %5d %10.1f (%7.1f) %10.1f (%7.1f) %12.1f %9.2fx" % (
            kind, hname, m.bins_evaluated, T, mb, min(t_b), mg, min(t_g), statistics.median(t_g2), mb / mg))
        m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
