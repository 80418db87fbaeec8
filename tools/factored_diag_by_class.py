#!/usr/bin/env python3
"""K-factored's per-wave stamps (tools/factored_diag.py) by CLASS of (c, e) pair: DESIGN.md 6ah, step 0.
A workgroup is mapped back to its pair -- ce = ce_end - 1 - blockIdx.x, ie = ce mod n_e -- and the pairs are grouped
twice: by quartile of lambda0 = c (1 - e)^k over the grid's pairs, and by quarter of the e axis (what
tools/time_deals.py times).  Per group and wave: enter, walk, shared+first, contract, log, barrier, and the items the
wave skipped by the column limit.  On the diagnostic build, on the GPU box:
  COVEST_AMD_LIB=tools/bin/libcovest_amd_diag.so python tools/factored_diag_by_class.py [c3|c3t] [--items N] [--shares OUT.json]
--shares writes, per quarter of the e axis, the share of the walk's items each builder wave builds."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["COVEST_FACTORED_DIAG"] = "1"
from bench import load_hist, workload, workload_tail  # noqa: E402
from covest_amd import DenseGrid, RepeatsModel, _capi  # noqa: E402

K = 21
ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="c3", choices=["c3", "c3t"])
ap.add_argument("--items", type=int, default=None, help="items of the walk (c3: 31, c3t: 12)")
ap.add_argument("--shares", default=None)
args = ap.parse_args()
n_items = args.items or {"c3": 31, "c3t": 12}[args.workload]

kind, hname, axes = workload(args.workload, 1)
m = RepeatsModel(K, 100, load_hist(hname), float(workload_tail(args.workload)), max_error=8)
g = DenseGrid(m, axes)
g.evaluate(kernel="factored")
g.argmin()
L = _capi.lib()
n = L.covest_grid_diag(g._handle, None, 0)
buf = np.zeros(n, dtype=np.int64)
L.covest_grid_diag(g._handle, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n)
st = buf.reshape(-1, 8, 8)
n_c, n_e = len(axes[0]), len(axes[1])
if st.shape[0] != n_c * n_e:
    raise SystemExit("%d workgroups for %d pairs: more than one q-block a pair, no class to map" % (st.shape[0], n_c * n_e))
ce = n_c * n_e - 1 - np.arange(st.shape[0])  # (the whole grid: ce_begin 0)
ic, ie = ce // n_e, ce % n_e
lam = np.asarray(axes[0])[ic] * (1.0 - np.asarray(axes[1])[ie]) ** K
print("%s: %d workgroups, %d items; lambda0 %.2f .. %.2f" % (args.workload, st.shape[0], n_items, lam.min(), lam.max()))


def table(sel, title):
    s = st[sel].astype(np.float64)
    skipped = (st[sel][:, :, 5] >> 20).astype(np.float64)
    print("%s: %d pairs" % (title, int(sel.sum())))
    print("  wave    enter     walk  wait-1st  shared+1st  contract      log  barrier   bar %  skipped  built %")
    share = []
    for w in range(8):
        a, b, c, bar = (s[:, w, k].mean() for k in range(4))
        b0, ent, fst = s[:, w, 4].mean(), s[:, w, 6].mean(), s[:, w, 7].mean()
        tot = ent + a + fst + b0 + b + c + bar
        sk = skipped[:, w].mean()
        share.append(1.0 - sk / n_items)
        print("  %4d %8.0f %8.0f %9.0f %11.0f %9.0f %8.0f %8.0f %6.1f %8.2f %7.1f" % (
            w, ent, a, fst, b0, b, c, bar, 100.0 * bar / tot, sk, 100.0 * share[-1]))
    print("  all waves: barrier %.1f %% of the wave-cycles" % (100.0 * s[:, :, 3].sum() / (s[:, :, :5].sum() + s[:, :, 6:].sum())))
    return share


table(np.ones(len(lam), dtype=bool), "all pairs")
cuts = np.quantile(lam, [0.25, 0.5, 0.75])
quart = np.searchsorted(cuts, lam, side="right")
for q in range(4):
    sel = quart == q
    table(sel, "lambda0 quartile %d (%.2f .. %.2f)" % (q, lam[sel].min(), lam[sel].max()))
shares = {}
for q in range(4):
    lo, hi = q * n_e // 4, (q + 1) * n_e // 4
    sel = (ie >= lo) & (ie < hi)
    e_ax = np.asarray(axes[1])
    sh = table(sel, "e quarter %d (e %.4f .. %.4f, lambda0 %.2f .. %.2f)" % (q, e_ax[lo], e_ax[hi - 1], lam[sel].min(), lam[sel].max()))
    shares[str(q)] = sh[:5]
if args.shares:
    os.makedirs(os.path.dirname(os.path.abspath(args.shares)), exist_ok=True)
    with open(args.shares, "w") as f:
        json.dump({"workload": args.workload, "items": n_items, "shares": shares}, f)
