"""Latency of one value+gradient call (covest_eval_points_grad, ll_deriv.hip) against the P + 1-point value call the
finite-difference route of CoverageEstimator makes (covest_eval_points, the route there was before), and a 20-start
multi-start (bench.py --workload f2's set-up) with gradient="fd" and gradient="analytic".  One process, one device,
after the spin-up bench.py uses; per case the median and the fastest of N calls, each call ending in a synchronise
(both entry points wait for their stream), every route in a run of calls of its own.

    python tools/time_gradient.py [--calls 30] [--out profiles/gradient_latency.txt]
"""
import argparse
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from bench import load_hist  # noqa: E402
from covest_amd import BasicModel, CoverageEstimator, RepeatsModel, initial_grid  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gradient_latency.txt"))
    args = ap.parse_args()
    lines = ["# one gradient: covest_eval_points_grad on 1 point against covest_eval_points on the P + 1 points of scipy's",
             "# 2-point scheme (step 1e-8); microseconds a call, median (fastest) of %d, each route in a run of its own" % args.calls,
             "# %-8s %-16s %6s %5s %22s %22s %8s" % ("model", "histogram", "keys", "T", "analytic, 1 point", "fd, P + 1 points", "fd / an")]
    for kind, hname, tail, point in CASES:
        cls = RepeatsModel if kind == "repeats" else BasicModel
        m = cls(21, 100, load_hist(hname), tail, max_error=8)
        P = m.param_count
        one = np.array([point], dtype=np.float64)
        fd = np.repeat(one, P + 1, axis=0)
        for d in range(P):
            fd[1 + d, d] += 1e-8
        T = int(m.get_hist_threshold_values([point[2:5]])[0]) if kind == "repeats" else 2
        spin_up(lambda: m.loglikelihood_points(fd))
        spin_up(lambda: m.loglikelihood_gradient_points(one))
        t_an = timed(lambda: m.loglikelihood_gradient_points(one), args.calls)
        t_fd = timed(lambda: m.loglikelihood_points(fd), args.calls)
        ma, mf = statistics.median(t_an), statistics.median(t_fd)
        lines.append("  %-8s %-16s %6d %5d %12.1f (%7.1f) %12.1f (%7.1f) %7.2fx" % (
            kind, hname, m.bins_evaluated, T, ma, min(t_an), mf, min(t_fd), mf / ma))
        m.close()
    # ---- the 20-start multi-start of bench.py --workload f2
    m = RepeatsModel(21, 100, load_hist("H10k_rep"), 0, max_error=8)
    lines.append("# 20-start multi-start (bench.py --workload f2: H10k_rep, initial_grid seed 20240521), starts one after the other")
    lines.append("# %-9s %9s %6s %7s %9s %22s  %s" % ("gradient", "seconds", "nit", "evals", "launches", "best -LL", "best x"))
    for mode in ("fd", "analytic"):
        est = CoverageEstimator(m, gradient=mode)
        random.seed(20240521)
        starts = initial_grid([25.0, 0.02, 0.6, 0.5, 0.1], count=20, bounds=est.bounds)
        est._optimize(starts[0])
        t0 = time.perf_counter()
        results = [est._optimize(s) for s in starts]
        wall = time.perf_counter() - t0
        best = min(results, key=lambda r: r.fun)
        nfev = sum(r.nfev for r in results)
        evals = nfev * (6 if mode == "fd" else 1)
        launches = nfev * (1 if mode == "fd" else 2)  # (K-grad: the segments' launch and the finishing one)
        lines.append("  %-9s %9.3f %6d %7d %9d %22.10f  %s" % (mode, wall, sum(r.nit for r in results), evals, launches, best.fun,
                                                            " ".join("%.10g" % v for v in best.x)))
    m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
