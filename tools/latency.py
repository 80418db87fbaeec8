"""Latency of one point-list call through the C ABI (what scipy's refinement waits for): covest_eval_points with 1, 6, 64,
300 and 5000 points, covest_eval_points_grad and covest_eval_points_hess with 1 and 300, wall time per call after a
warm-up call of the same shape.  The library is the one COVEST_AMD_LIB names (covest_amd/_capi.py), else the tree's.

    python tools/latency.py
    python tools/latency.py --ab NEW.so PARENT.so [--rounds 5] [--out profiles/points_latency_ab.txt]

--ab: the two libraries alternately, a fresh process each, `rounds` times each; per row both medians and spreads
(max - min over the rounds).  A row is marked when the new median exceeds the parent's by more than the parent's own
spread in this same run, and the exit status says whether any is.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MODELS = (("basic H10k_basic", "H10k_basic", (4000.0, 0.02)), ("repeats H10k_rep", "H10k_rep", (25.0, 0.02, 0.6, 0.5, 0.1)),
          ("repeats sim", "sim_c10_e0.05", (10.0, 0.05, 0.8, 0.5, 0.3)))
CALLS = [("value", n) for n in (1, 6, 64, 300, 5000)] + [("grad", 1), ("grad", 300), ("hess", 1), ("hess", 300)]


def measure():
    """One process: 'name | call | n | us per call' per row."""
    import numpy as np
    from bench import load_hist
    from covest_amd import BasicModel, RepeatsModel
    for name, hist, p in MODELS:
        m = (BasicModel if len(p) == 2 else RepeatsModel)(21, 100, load_hist(hist), 0, max_error=8)
        m.compute_loglikelihood(*p)
        for call, n in CALLS:
            fn = {"value": m.loglikelihood_points, "grad": m.loglikelihood_gradient_points, "hess": m.loglikelihood_hessian_points}[call]
            pts = np.tile(np.array(p), (n, 1)) * (1 + 1e-3 * np.arange(n) / max(1, n // 64))[:, None]
            fn(pts)
            reps = 200 if n <= 64 else 50 if n <= 300 else 10
            t0 = time.perf_counter()
            for _ in range(reps):
                fn(pts)
            dt = (time.perf_counter() - t0) / reps
            print("%s | %s | %d | %.1f" % (name, call, n, 1e6 * dt), flush=True)
        m.close()


def ab(new, parent, rounds, out):
    got = {"new": {}, "parent": {}}
    for r in range(rounds):
        for tag, lib in (("parent", parent), ("new", new)):
            env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:  # nothing more is started after a child that failed
                print("round %d: the %s library's run ended with status %d" % (r, tag, p.returncode))
                return 2
            for line in p.stdout.splitlines():
                name, call, n, us = [f.strip() for f in line.split("|")]
                got[tag].setdefault((name, call, int(n)), []).append(float(us))
            print("round %d %s done" % (r, tag), flush=True)
    lines = ["# us per call, median and spread (max - min) of %d fresh processes each, parent and new alternating (tools/latency.py --ab)" % rounds,
             "%-18s %-5s %5s %10s %8s %10s %8s  %s" % ("model", "call", "n", "parent", "spread", "new", "spread", "new - parent")]
    slower = 0
    for key in got["parent"]:
        a, b = got["parent"][key], got["new"][key]
        ma, mb, sa, sb = statistics.median(a), statistics.median(b), max(a) - min(a), max(b) - min(b)
        over = mb > ma + sa
        slower += over
        lines.append("%-18s %-5s %5d %10.1f %8.1f %10.1f %8.1f  %+8.1f%s" % (key[0], key[1], key[2], ma, sa, mb, sb, mb - ma,
                                                                             "  BEYOND the parent's spread" if over else ""))
    lines.append("rows whose new median exceeds the parent's by more than the parent's spread: %d" % slower)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 1 if slower else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", nargs=2, metavar=("NEW", "PARENT"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "points_latency_ab.txt"))
    args = ap.parse_args()
    if args.ab:
        return ab(args.ab[0], args.ab[1], args.rounds, args.out)
    measure()
    return 0


if __name__ == "__main__":
    sys.exit(main())
