"""Latency of one value+gradient+Hessian call (covest_eval_points_hess, ll_deriv.hip) on one point, beside the route it
replaces measured in the same process: one covest_eval_points_grad call of the 2P points a central difference of the
analytic gradient needs.  One process, one device, after the spin-up bench.py uses; per case the median and the fastest
of N calls, each call ending in a synchronise (both entry points wait for their stream), every route in a run of calls
of its own.

    python tools/time_hessian.py [--calls 30] [--out profiles/hessian_latency.txt] [--only hess|grad]

--only: spin up and time ONE route only (nothing written unless --out is given): for a kernel trace of that route alone.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from bench import load_hist  # noqa: E402
from covest_amd import BasicModel, RepeatsModel  # noqa: E402

CASES = [("repeats", "sim_c10_e0.05", 0, [10.0, 0.05, 0.8, 0.5, 0.5]),
         ("repeats", "H10k_rep_trim", 11192, [23.7, 0.0195, 0.56, 0.5, 0.11]),
         ("repeats", "H10k_rep", 0, [25.0, 0.02, 0.6, 0.5, 0.1]),
         ("basic", "H10k_basic_trim", 163, [4000.0, 0.02])]


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def spin_up(fn):
    fn()
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    per_step = (time.perf_counter() - t0) / 5
    for _ in range(max(25, min(400, int(0.020 / max(per_step, 1e-6)) + 1))):
        fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--only", choices=("hess", "grad"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out if args.out or args.only else os.path.join(REPO, "profiles", "hessian_latency.txt")
    lines = ["# one Hessian: covest_eval_points_hess on 1 point against covest_eval_points_grad on the 2P points of a central",
             "# difference of the analytic gradient (step 1e-4 |theta|); microseconds a call, median (fastest) of %d, each route in a"
             % args.calls,
             "# run of its own",
             "# %-8s %-16s %6s %5s %22s %22s %8s" % ("model", "histogram", "keys", "T", "closed form, 1 point", "gradients, 2P points",
                                                     "grad / cf")]
    for kind, hname, tail, point in CASES:
        cls = RepeatsModel if kind == "repeats" else BasicModel
        m = cls(21, 100, load_hist(hname), tail, max_error=8)
        P = m.param_count
        one = np.array([point], dtype=np.float64)
        fd = np.repeat(one, 2 * P, axis=0)
        for d in range(P):
            fd[2 * d, d] += 1e-4 * abs(point[d])
            fd[2 * d + 1, d] -= 1e-4 * abs(point[d])
        T = int(m.get_hist_threshold_values([point[2:5]])[0]) if kind == "repeats" else 2
        t_cf = t_fd = [float("nan")]
        if args.only != "grad":
            spin_up(lambda: m.loglikelihood_hessian_points(one))
            t_cf = timed(lambda: m.loglikelihood_hessian_points(one), args.calls)
        if args.only != "hess":
            spin_up(lambda: m.loglikelihood_gradient_points(fd))
            t_fd = timed(lambda: m.loglikelihood_gradient_points(fd), args.calls)
        mc, mf = statistics.median(t_cf), statistics.median(t_fd)
        lines.append("  %-8s %-16s %6d %5d %12.1f (%7.1f) %12.1f (%7.1f) %7.2fx" % (
            kind, hname, m.bins_evaluated, T, mc, min(t_cf), mf, min(t_fd), mf / mc))
        m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
