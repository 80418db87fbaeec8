#!/usr/bin/env python3
"""What a class's own unit deal is worth: K-factored's launch time on C3-shaped grids restricted
to one quarter of the e axis each -- 8 values of e x 128 values of c over C3's range, 1024 workgroups, four rounds of the
chip as C3 itself (tools/time_rounds.py) -- under the shipped deal and under per-wave builder charges made from that
quarter's own shares: base x the share of the walk's items the wave builds there (tools/factored_diag_by_class.py --shares).
On the TUNING library (tools/build_tune.sh), which alone reads the overrides:
  COVEST_AMD_LIB=tools/bin/lib_tune.so python tools/time_deals.py SHARES.json [--bases 27,30,33] [--repeats 3]
The prediction for per-class deals is the sum over the quarters of (time at the shipped deal - best time) / 4: a quarter
is a quarter of C3's pairs, and every grid here has C3's number of rounds."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import load_hist, workload, workload_tail  # noqa: E402
from covest_amd import DenseGrid, RepeatsModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shares")
ap.add_argument("--bases", default="27,30,33")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--search", action="store_true", help="beside the shares' profiles, a lattice of profiles (an upper bound)")
ap.add_argument("--whole", action="store_true", help="search on the workload's whole grid instead of the quarters")
ap.add_argument("--strong", action="store_true", help="... on the strong-scaling grid (128 x 128 pairs)")
ap.add_argument("--quarter", type=int, default=None, help="with --whole --profiles: one quarter of the e axis")
ap.add_argument("--away", action="store_true", help="... on a grid away from C3's ranges: c 5..15, e 0.08..0.15")
ap.add_argument("--profiles", default=None, help="with --whole / --strong: 'p0,p1,..;p0,p1,..' shares in per cent, no search")
ap.add_argument("--out", default=None, help="directory for the search's timings")
ap.add_argument("--floor", default="0,0.5", help="a wave's share is not taken below this (one sweep per value)")
args = ap.parse_args()
with open(args.shares) as f:
    rec = json.load(f)
wl = rec["workload"]
kind, hname, axes = workload(wl, 1)
m = RepeatsModel(21, 100, load_hist(hname), float(workload_tail(wl)), max_error=8)
n_e = len(axes[1])


def time_grid(ax, env, warm=20, timed=40):
    """mean ms of a K-factored launch with the planner's overrides `env` (read when the plan is built)"""
    for k in ("COVEST_FACTORED_BUILD_COST", "COVEST_FACTORED_BUILD_COST_WAVES", "COVEST_FACTORED_BUILD_SHARE_WAVES"):
        os.environ.pop(k, None)
    os.environ.update(env)
    g = DenseGrid(m, ax)
    for _ in range(warm):
        g.evaluate()
    g.argmin()
    g.profile(True)
    for _ in range(timed):
        g.evaluate()
    g.argmin()
    ms, n = g.kernel_ms()
    g.close()
    return ms / n


SHARES = (100, 90, 75, 60, 50, 40, 30)


def search(label, ax, bases):
    """--search: an upper bound -- every non-increasing profile of shares (per cent of the base charge, wave 0 at 100)
    on a coarse lattice, at every base charge (None: the planner's own), one short timing each; all of them go to
    --out as JSON, the best six are timed again at full length.  Many profiles make the same deal: the times come in groups."""
    import itertools
    seen = []
    for base in bases:
        for rest in itertools.combinations_with_replacement(SHARES, 4):
            env = {"COVEST_FACTORED_BUILD_SHARE_WAVES": ",".join(str(x) for x in (100,) + rest)}
            if base is not None:
                env["COVEST_FACTORED_BUILD_COST"] = str(base)
            seen.append((time_grid(ax, env, 8, 16), "%s:%s" % (base, env["COVEST_FACTORED_BUILD_SHARE_WAVES"]), env))
    seen.sort(key=lambda r: r[0])
    print("%s: %d profiles, short timings %.4f .. %.4f ms; the best ten: %s" % (
        label, len(seen), seen[0][0], seen[-1][0], "  ".join("%s %.4f" % (w, t) for t, w, _ in seen[:10])))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "deals_search_%s.json" % label), "w") as f:
            json.dump({w: t for t, w, _ in seen}, f)
    return [("share %s" % w, env) for _, w, env in seen[:6]]


def report(label, configs, ax):
    configs = list({name: (name, env) for name, env in configs}.values())  # (two floors may round to one profile)
    times = {name: [] for name, _ in configs}
    for _ in range(args.repeats):  # (alternating: every configuration once a repeat)
        for name, env in configs:
            times[name].append(time_grid(ax, env))
    print(label)
    best = None
    for name, _ in configs:
        t = np.array(times[name])
        print("  %-34s mean %.4f ms  (%s)" % (name, t.mean(), " ".join("%.4f" % x for x in t)))
        if name != "shipped" and (best is None or t.mean() < best[1]):
            best = (name, t.mean())
    shipped = float(np.mean(times["shipped"]))
    print("  best: %s, %.4f ms; shipped %.4f ms (spread %.4f): gain %.1f us" % (
        best[0], best[1], shipped, float(np.ptp(times["shipped"])), 1e3 * (shipped - best[1])))
    return shipped, min(shipped, best[1])


if args.whole or args.strong or args.away:  # the workload's own grid: what ONE profile for every pair is worth
    if args.strong:
        axes = workload("c3", 1, "strong")[2]
    if args.away:  # C3's q axes at low c and high e: lambda0 = c (1 - e)^k below C3's range
        axes = [np.linspace(5.0, 15.0, 32), np.linspace(0.08, 0.15, 32)] + list(axes[2:])
    label = "%s, the %s grid" % (wl, "strong" if args.strong else "away (c 5..15, e 0.08..0.15)" if args.away else "whole")
    if args.profiles:  # given profiles of shares instead of the search
        found = [("share %s" % p, {"COVEST_FACTORED_BUILD_SHARE_WAVES": p}) for p in args.profiles.split(";")]
        if args.quarter is not None:  # ... on one quarter of the e axis, 128 values of c
            lo, hi = args.quarter * n_e // 4, (args.quarter + 1) * n_e // 4
            axes = [np.linspace(axes[0][0], axes[0][-1], 128), np.asarray(axes[1])[lo:hi]] + list(axes[2:])
            label = "%s, e quarter %d" % (wl, args.quarter)
    else:
        found = search(wl, axes, [None] if wl != "c3" else [int(b) for b in args.bases.split(",")])
    report(label, [("shipped", {})] + found, axes)
    sys.exit(0)

total_shipped, total_best = 0.0, 0.0
for q in range(4):
    lo, hi = q * n_e // 4, (q + 1) * n_e // 4
    ax = [np.linspace(axes[0][0], axes[0][-1], 128), np.asarray(axes[1])[lo:hi]] + list(axes[2:])
    share = rec["shares"][str(q)]
    configs = [("shipped", {})]
    for base in (int(b) for b in args.bases.split(",")):
        configs.append(("one charge %d" % base, {"COVEST_FACTORED_BUILD_COST": str(base)}))
        for fl in (float(x) for x in args.floor.split(",")):
            waves = ",".join(str(int(round(base * max(fl, s)))) for s in share)
            configs.append(("per wave %s" % waves, {"COVEST_FACTORED_BUILD_COST_WAVES": waves}))
    if args.search:
        configs += search("%s_q%d" % (wl, q), ax, [int(b) for b in args.bases.split(",")])
    shipped, best_t = report("e quarter %d (e %.4f .. %.4f), shares %s" % (q, ax[1][0], ax[1][-1], " ".join("%.2f" % s for s in share)),
                             configs, ax)
    total_shipped += shipped
    total_best += best_t
print("prediction for C3 (a quarter of its pairs each): %.4f -> %.4f ms, %.1f us a launch" % (
    total_shipped / 4, total_best / 4, 1e3 * (total_shipped - total_best) / 4))
