#!/usr/bin/env python3
"""Golden vectors for the per-axis minima of a dense grid (covest_grid_axis_min), made by running the REFERENCE:
covest.models.{Basic,Repeats}Model.compute_loglikelihood at every point of a small grid over
tests/golden/sim_c10_e0.05.hist, and per cell of the kept axes the selection loop of covest/grid.py:65-70
(started from +inf: strict <, first index wins) over the reference's own values.

Build container only (/root/reference).  Writes DATA ONLY: tests/golden/axis_min.json.

Per mask the fixture also records each cell's runner-up (the smallest value of the cell at another index) and how many
cells are NEAR TIES -- runner-up within 2e-9 relative of the winner, where an implementation that agrees with the
reference to 1e-9 may pick either.  Such cells must stay at most 1 % of a mask's cells: asserted here of the
reference's numbers and again by the test from the fixture.  If the assertion fails, change the axes, not the cap.
(With q1 = 1.0 on the axis q2 and q do not enter the value and a fifth of the cells are exact ties: the q1 axis stops
at 0.95.)

With a tail the reference's own term tail * log(1 - sp_j) (covest/models.py:103-104) can hang on the last bits of
sp_j = fsum(p_j).  For the cases with a tail the fixture records the sp_j the REFERENCE saw at every point and how
many points fall into the graded / flip classes of tests/parity_helpers.py _tail_slack -- a property of the
reference's numbers alone, the budget the test holds its use of that slack to.

Usage:  python tests/golden/make_golden_axis_min.py     (COVEST_GOLDEN_PROCS worker processes, default 8)
"""
import itertools
import json
import math
import multiprocessing
import os
import platform
import subprocess
import sys
import time

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("COVEST_REFERENCE", "/root/reference")
REF_BUILD = os.path.join(REPO, "oracle", "_ref")

subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle"), "ref"], stdout=subprocess.DEVNULL)
os.environ.setdefault("MPLBACKEND", "Agg")
import scipy  # noqa: E402
import scipy.misc  # noqa: E402
import scipy.special  # noqa: E402
if not hasattr(scipy.misc, "comb"):
    scipy.misc.comb = scipy.special.comb
sys.path.insert(0, REF_BUILD)
sys.path.insert(0, REFERENCE)
import covest.constants  # noqa: E402
covest.constants.VERBOSE = False
from covest.models import BasicModel, RepeatsModel  # noqa: E402

HIST, K, R, MAX_ERROR = "sim_c10_e0.05", 21, 100, 8
AXES = [np.linspace(8.0, 12.0, 9), np.linspace(0.02, 0.08, 7), np.linspace(0.4, 0.95, 4), np.array([0.2, 0.6, 0.9]),
        np.linspace(0.05, 0.9, 4)]
MASKS = {"c,e": (0, 1), "c": (0,), "e": (1,), "q1,q2,q": (2, 3, 4)}
NEAR_TIE, NEAR_TIE_CAP = 2e-9, 0.01


def load(name):
    hist = {}
    with open(os.path.join(HERE, name + ".hist")) as f:
        for line in f:
            if line.strip() and line[0] != "#":
                a, b = line.split()[:2]
                hist[int(a)] = int(b)
    return hist


_model = None


def _start(kind, tail):
    global _model
    cls = RepeatsModel if kind == "repeats" else BasicModel
    _model = cls(K, R, load(HIST), tail, max_error=MAX_ERROR)


def _ll(point):
    return float(_model.compute_loglikelihood(*point))


def _sp(point):
    return math.fsum(_model.compute_probabilities(*_model.fit_to_bounds(point)).values())


def reference_scan(negll, flat_indices):
    """covest/grid.py:65-70 with maximize=False from +inf over the points of one cell, in flat-index order; and the
    runner-up: the smallest value at another index (first occurrence)."""
    min_val, min_arg = math.inf, -1
    for i in flat_indices:
        val = negll[i]
        if val < min_val:
            min_val, min_arg = val, i
    second_val, second_arg = math.inf, -1
    for i in flat_indices:
        if i != min_arg and negll[i] < second_val:
            second_val, second_arg = negll[i], i
    return min_val, min_arg, second_val, second_arg


def per_mask(negll, shape, keep):
    cells = {}
    for flat, coord in enumerate(itertools.product(*[range(n) for n in shape])):
        cells.setdefault(tuple(coord[d] for d in keep), []).append(flat)
    rows = [reference_scan(negll, cells[c]) for c in sorted(cells)]  # row-major in the kept axes' order
    near = sum(1 for v, a, v2, a2 in rows if a2 >= 0 and abs(v2 - v) <= NEAR_TIE * abs(v))
    assert near <= NEAR_TIE_CAP * len(rows), "near ties in %d of %d cells: change the axes, not the cap" % (near, len(rows))
    gaps = [abs(v2 - v) / abs(v) for v, a, v2, a2 in rows if a2 >= 0]
    return {"keep": list(keep), "negll": [r[0] for r in rows], "index": [r[1] for r in rows],
            "runner_up_negll": [r[2] if r[3] >= 0 else None for r in rows], "runner_up_index": [r[3] for r in rows],
            "near_ties": near, "cells": len(rows), "smallest_relative_gap": min(gaps) if gaps else None}


def case(kind, tail, procs):
    axes = AXES if kind == "repeats" else AXES[:2]
    shape = [len(a) for a in axes]
    points = [tuple(float(v) for v in p) for p in itertools.product(*axes)]
    t0 = time.time()
    with multiprocessing.Pool(procs, initializer=_start, initargs=(kind, tail)) as pool:
        ll = pool.map(_ll, points, chunksize=8)
        sp = pool.map(_sp, points, chunksize=8) if tail else None
    assert all(math.isfinite(v) for v in ll), "a non-finite value on the grid: change the axes"
    negll = [-v for v in ll]
    masks = {name: per_mask(negll, shape, keep) for name, keep in MASKS.items() if max(keep) < len(axes)}
    print("%s tail %s: %d points in %.0f s; near ties %s" % (kind, tail, len(points), time.time() - t0,
                                                              {n: m["near_ties"] for n, m in masks.items()}), flush=True)
    out = {"model": kind, "tail": tail, "shape": shape, "ll": ll, "masks": masks}
    if tail:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        from parity_helpers import _tail_slack
        classes = [_tail_slack(tail, v, s, len(load(HIST)))[1] for v, s in zip(ll, sp)]
        out["sp"] = sp
        out["tail_slack"] = {"graded": classes.count("graded"), "flip": classes.count("flip"), "points": len(points)}
        print("%s tail %s: tail-term classes %s" % (kind, tail, out["tail_slack"]), flush=True)
    return out


def main():
    procs = int(os.environ.get("COVEST_GOLDEN_PROCS", "8"))
    out = {"_made_by": "tests/golden/make_golden_axis_min.py",
           "what": "reference LL at every point of a dense grid over %s.hist and, per mask of kept axes, per cell the "
                   "selection loop of covest/grid.py:65-70 over those values (negll, flat index), the runner-up and the "
                   "count of near ties (runner-up within %g relative)" % (HIST, NEAR_TIE),
           "hist": HIST, "k": K, "r": R, "max_error": MAX_ERROR, "axes": [[float(v) for v in a] for a in AXES],
           "near_tie": NEAR_TIE, "near_tie_cap": NEAR_TIE_CAP, "cases": {},
           "env": {"python": platform.python_version(), "scipy": scipy.__version__, "numpy": np.__version__,
                   "machine": platform.machine(), "reference": "mhozza/covest v0.5.6"}}
    for kind in ("repeats", "basic"):
        for tail in (0, 1000):
            out["cases"]["%s_tail%d" % (kind, tail)] = case(kind, tail, procs)
    path = os.path.join(HERE, "axis_min.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
