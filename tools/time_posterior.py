"""Time of one covest_posterior_classes call on one point, beside covest_probabilities on the same model and point (which
walks the same components once, with one exp each; the posterior walks them three times, twice with an exp): by HIP
events on the null stream either side of the call, median (fastest) of 7 behind a warm-up, each route in a run of its own.
An event pair brackets everything the call puts on the stream -- the uploads, the launches and the copies back.

    python tools/time_posterior.py [--out profiles/posterior_latency.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from bench import load_hist  # noqa: E402
from covest_amd import BasicModel, RepeatsModel, _capi  # noqa: E402

CASES = [("repeats", "H10k_rep_trim", 11192, [23.7, 0.0195, 0.56, 0.5, 0.11]),
         ("repeats", "sim_c10_e0.05", 0, [10.0, 0.05, 0.8, 0.5, 0.5]),
         ("basic", "H10k_basic_trim", 163, [4000.0, 0.02])]


class Events:
    def __init__(self):
        _capi.lib()
        self.hip = ctypes.CDLL(_capi.hip_runtimes_mapped()[0])  # the runtime the library is bound to
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for ev in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(ev)) == 0

    def ms(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        out = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(out), self.a, self.b) == 0
        return out.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posterior_latency.txt"))
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    lines = ["# one point: covest_posterior_classes (4 copy columns, every output) against covest_probabilities; microseconds a",
             "# call by HIP events, median (fastest) of %d behind 10 warm-up calls, each route in a run of its own" % args.calls,
             "# %-8s %-16s %6s %5s %22s %22s %8s" % ("model", "histogram", "keys", "T", "posterior classes", "probabilities", "ratio")]
    ev = None
    for kind, hname, tail, point in CASES:
        cls = RepeatsModel if kind == "repeats" else BasicModel
        m = cls(21, 100, load_hist(hname), tail, max_error=8)
        one = np.array([point], dtype=np.float64)
        T = int(m.get_hist_threshold_values([point[2:5]])[0]) if kind == "repeats" else 2
        times = []
        # (the C entry points themselves, into arrays made once: no Python work between the events but the call)
        L, K, dp = _capi.lib(), len(m.hist), ctypes.POINTER(ctypes.c_double)
        outs = [np.empty(n) for n in (K, K * 8, K * 4, K)]
        ptrs = [a.ctypes.data_as(dp) for a in outs]
        par = one.ctypes.data_as(dp)
        for fn in (lambda: L.covest_posterior_classes(m.handle, 1, par, 1, 4, *ptrs),
                   lambda: L.covest_probabilities(m.handle, par, 1, ptrs[0])):
            assert fn() == 0
            for _ in range(10):
                fn()
            ev = ev or Events()
            times.append([1e3 * ev.ms(fn) for _ in range(args.calls)])
        mp_, mq = statistics.median(times[0]), statistics.median(times[1])
        lines.append("  %-8s %-16s %6d %5d %12.1f (%7.1f) %12.1f (%7.1f) %7.2fx" % (
            kind, hname, len(m.hist), T, mp_, min(times[0]), mq, min(times[1]), mp_ / mq))
        m.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
