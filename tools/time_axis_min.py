"""Per-axis minima of the C3 grid (bench.py's 262 144 points on H10k_rep): the device route, DenseGrid.axis_minima,
against the route there was before it -- loglikelihoods() (8 bytes a point copied back) and the numpy restatement of
the per-cell scan (tests/test_gpu_axis_min.py numpy_axis_minima).  Both in this one process on one device, after the
spin-up bench.py uses (a stretch of evaluations for the clocks to settle); per mask the median and the fastest of N
calls of each route, every route in a run of calls of its own.  A last column times the device route when each call
follows a host-route call (the two interleaved, as a caller that mixes them would see it), and a last
line an argmin() on the idle handle: the wait and the host read that every call has.

    python tools/time_axis_min.py [--calls 30] [--out profiles/axis_min_c3.txt]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

from bench import load_hist, workload  # noqa: E402
from covest_amd import DenseGrid, RepeatsModel  # noqa: E402
from test_gpu_axis_min import numpy_axis_minima  # noqa: E402

MASKS = [("c,e", (0, 1)), ("c", (0,)), ("q1,q2,q", (2, 3, 4))]


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "axis_min_c3.txt"))
    args = ap.parse_args()
    if args.calls < 20:
        raise SystemExit("--calls: at least 20")
    kind, hname, axes = workload("c3", 1)
    assert kind == "repeats"
    m = RepeatsModel(21, 100, load_hist(hname), 0, max_error=8)
    g = DenseGrid(m, axes)
    g.evaluate()
    g.argmin()
    t0 = time.perf_counter()
    for _ in range(5):
        g.evaluate()
    g.argmin()
    per_step = (time.perf_counter() - t0) / 5
    spinup = max(25, min(400, int(0.020 / max(per_step, 1e-6)) + 1))
    for _ in range(spinup):
        g.evaluate()
    g.argmin()
    lines = ["# per-axis minima of the C3 grid (%s, %d points, %.3f ms an evaluation); microseconds a call, median (fastest) of %d"
             % (hname, g.total, per_step * 1e3, args.calls),
             "# device route: DenseGrid.axis_minima(keep); host route: loglikelihoods() + numpy per-cell scan; each route timed",
             "# in a run of calls of its own.  Last column: the device route when every call follows a host-route call.",
             "# %-8s %7s %20s %20s %22s %8s %22s" % ("mask", "cells", "device route", "host route", "of it loglikelihoods()", "ratio",
                                                    "device after host")]
    for label, keep in MASKS:
        def host_route():
            return numpy_axis_minima(g.loglikelihoods(), g.shape, keep)

        for _ in range(3):  # both routes warm (code objects, scratch, page-locked block)
            dev, host = g.axis_minima(keep), host_route()
        assert np.array_equal(dev[0].view(np.int64), host[0].view(np.int64)) and np.array_equal(dev[1], host[1]), label
        t_dev = timed(lambda: g.axis_minima(keep), args.calls)
        t_copy = timed(g.loglikelihoods, args.calls)
        t_host = timed(host_route, args.calls)
        t_after = []
        for _ in range(args.calls):
            host_route()
            t_after += timed(lambda: g.axis_minima(keep), 1)
        md, mh, mc, ma = (statistics.median(t) for t in (t_dev, t_host, t_copy, t_after))
        lines.append("  %-8s %7d %10.1f (%7.1f) %10.1f (%7.1f) %12.1f (%7.1f) %7.1fx %12.1f (%7.1f)" % (
            label, dev[0].size, md, min(t_dev), mh, min(t_host), mc, min(t_copy), mh / md, ma, min(t_after)))
    g.evaluate()
    base = statistics.median(timed(g.argmin, args.calls))
    lines.append("# argmin() on the idle handle (a stream wait and a host read, no launch): %.1f us median" % base)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
