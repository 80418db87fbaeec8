#!/usr/bin/env python3
"""Golden vectors for the gradient of a histogram batch (covest_batch_eval_cross_grad / _pairs_grad, DESIGN.md section
6u): log-likelihood and analytic gradient of every histogram of a batch at every point, at 50 digits.

No formula is written here.  The restatement is make_golden_gradient.py's, imported (grad_partial, finish, consts_of), and
the batch identity is restated by how it is called: per shape and point the per-key rows [p, d_k p ...] are computed ONCE,
over every key of the model, and finish(rows, counts_b, tail_b, P) is called for each of the shape's B histograms.  The
shapes -- the model's histogram, the batch's rows, the points -- are tests/batch_grad_shapes.py's (see there for the
edges, and for why the coverage is set from the rate and not drawn from 5 .. 15).  Nothing of the reference is run or
read.

Before anything is written the generator asserts
  1. every point's threshold_o is the one the lot shape names, and the dead key's p_j is below 1e-400 at the dead point;
  2. selection, make_golden_gradient.py's rule 3 per (b, i): a finite LL, no counted p_j below 1e-300, with a tail
     |1 - sp| >= 1e-6 and the tail term in neither the graded nor the flip class of tests/parity_helpers.py _tail_slack,
     and 1e-9 Cg_k >= |tail| D_k delta / (1 - sp)^2 (delta = 8 eps n_keys) for every component not moved by the clamp;
     and, make_golden_deriv_shapes.py's clause for rates beyond 200, no component x = o lambda_s just above a multiple
     of 200 (residual below 1e-5 x: the reference's chunked normaliser hangs on the rounding of x there);
     an entry that fails is DROPPED and counted -- with ONE exception, the dead-key shapes' row that counts the dead key
     at the dead point, kept for its specials (LL = -inf there) --, and at most 5 % of the (b, i) entries of any shape,
     and of the whole, may be dropped (the cap tests/golden/make_golden_deriv_shapes.py states is 10 %; this one is the
     issue's).  If the cap is exceeded the points move, not the rule.

Writes DATA ONLY: tests/golden/batch_grad.json -- per shape the points, per point sp, T (repeats), D_k = |sum_j d_k p_j|
and which parameters the clamp moved (none of these depends on the histogram), per (b, i) ll, grad and the condition sums
Cg (9 digits: they enter a bound only), and the dropped (b, i) with the reason.  The rows themselves are not stored: they
are tests/batch_grad_shapes.py's, checked here by their sums.  Needs the built library for the model's host code (no
GPU).
Usage:  python tests/golden/make_golden_batch_grad.py     (COVEST_GOLDEN_PROCS worker processes, default 8, at most 16)
"""
import json
import multiprocessing
import os
import sys
import time

import mpmath
from mpmath import mp, mpf

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gradient as G  # noqa: E402  (the restatement; puts the repository and tests/ on the path)
import make_golden_deriv_shapes as DS  # noqa: E402  (near_chunk: its rule 2's last clause)
import batch_grad_shapes as S  # noqa: E402
from parity_helpers import _tail_slack  # noqa: E402

mp.dps = 50
K_TAIL, EPS = G.K_TAIL, G.EPS
MAX_PROCS = 16
MAX_DROPPED_SHARE = 0.05


def select(ll, sp, rows, counts, tail, n_keys, P, moved, Cg, D):
    """Rule 2: None to keep the entry, else why it is dropped."""
    p_min = min([row[0] for row, h in zip(rows, counts) if h != 0] or [mpf(1)])
    if not mp.isfinite(ll) or p_min < mpf(10) ** -300:
        return "a counted p_j beyond a double"
    if tail == 0:
        return None
    if abs(1 - sp) < 1e-6 or _tail_slack(tail, float(ll), float(sp), n_keys)[1] is not None:
        return "tail term graded or flip, 1 - sp = %s" % mp.nstr(1 - sp, 3)
    if not sp < 1:
        return None
    delta = K_TAIL * EPS * n_keys
    for k in range(P):
        if not moved[k] and not mpf(10) ** -9 * Cg[k] >= abs(tail) * D[k] * delta / (1 - sp) ** 2:
            return "gradient component %d's tail slack" % k
    return None


def _task(args):
    """One (shape, point): the rows once, then every histogram of the shape."""
    name, i = args
    mp.dps = 50
    case = S.shape(name)
    spec = case["spec"]
    m, consts, own, n_keys = G.consts_of(spec)
    assert consts[4] == spec["hist"]["keys"] and n_keys == case["n_keys"], "every key of the model"
    P = m.param_count
    point = [float(v) for v in case["points"][i]]
    clamped = m.fit_to_bounds(point)
    moved = [float(a) != float(b) for a, b in zip(point, clamped)]
    T = int(m.get_hist_threshold_values([clamped[2:5]])[0]) if P == 5 else 2
    theta = [mpf(float(v)) for v in clamped]
    rows = G.grad_partial(consts, theta, 1, T)
    near = DS.near_chunk(consts, theta, T)
    out = {"T": T, "moved": moved, "entries": []}
    dead_p = None
    if case["dead"]:
        dead_p = rows[consts[4].index(S.ISOLATED)][0]
    for b in range(len(case["counts"])):
        counts = [int(v) for v in case["counts"][b]]
        tail = int(case["tails"][b])
        ll, sp, grad, Cg, D = G.finish(rows, counts, tail, P)
        grad = [mpf(0) if mv else g for g, mv in zip(grad, moved)]
        why = select(ll, sp, rows, counts, tail, n_keys, P, moved, Cg, D)
        if why is None and near is not None:
            why = "copy number %d, class %d: x / xr = %s above a multiple of 200" % (near[0], near[1], mp.nstr(near[2], 3))
        special = case["dead"] and i == 0 and b == case["rows"]["dead"]
        if special:
            assert 0 < dead_p < mpf(10) ** -400 and counts[consts[4].index(S.ISOLATED)] != 0  # (0 in a double: LL = -inf)
            others = min(row[0] for row, h, j in zip(rows, counts, consts[4]) if h != 0 and j != S.ISOLATED)
            assert others >= mpf(10) ** -300
            why = None
        # (the special entry's LL is -inf in a double and its gradient NaN: nothing of the 50-digit value is compared)
        out["entries"].append({"ll": None if special else float(ll), "grad": None if special else [float(g) for g in grad], "Cg": [float("%.9g" % float(v)) for v in Cg],
                               "why": why, "special": bool(special)})
        out["sp"], out["D"] = float(sp), [float(v) for v in D]
    if dead_p is not None:
        out["log10_dead_p"] = float(mp.log10(dead_p))
    return out


def main():
    procs = min(MAX_PROCS, int(os.environ.get("COVEST_GOLDEN_PROCS", "8")))
    t0 = time.time()
    tasks = [(name, i) for name in S.SHAPES for i in range(len(S.shape(name)["points"]))]
    cost = lambda t: -S.shape(t[0])["n_keys"] * (50 if S.shape(t[0])["kind"] == "repeats" else 1) * (12 if S.shape(t[0])["dead"] else 1)  # noqa: E731
    order = sorted(range(len(tasks)), key=lambda at: cost(tasks[at]))  # the long ones first
    print("%d shapes, %d points, %d processes" % (len(S.SHAPES), len(tasks), procs), flush=True)
    with multiprocessing.Pool(procs) as pool:
        parts = pool.map(_task, [tasks[at] for at in order], chunksize=1)
    result = dict(zip([tasks[at] for at in order], parts))
    print("evaluated, %.0f s" % (time.time() - t0), flush=True)
    shapes, total, total_dropped = {}, 0, 0
    for name in S.SHAPES:
        case = S.shape(name)
        B, n = case["counts"].shape[0], len(case["points"])
        per_point = [result[(name, i)] for i in range(n)]
        if case["lot_tm1"]:  # assertion 1
            got = [r["T"] - 1 for r in per_point[:len(case["lot_tm1"])]]
            assert got == case["lot_tm1"], "threshold_o - 1 is %r, not %r" % (got, case["lot_tm1"])
            assert min(got) < S.LOT and S.LOT in got and max(got) > 2 * S.LOT
        dropped = [[b, i, per_point[i]["entries"][b]["why"]] for i in range(n) for b in range(B) if per_point[i]["entries"][b]["why"]]
        special = [[b, i] for i in range(n) for b in range(B) if per_point[i]["entries"][b]["special"]]
        assert len(special) == (1 if case["dead"] else 0)
        total += B * n
        total_dropped += len(dropped)
        print("%-24s %4d entries, %d dropped%s" % (name, B * n, len(dropped), "".join("\n    (%d, %d): %s" % tuple(d) for d in dropped)), flush=True)
        assert len(dropped) <= MAX_DROPPED_SHARE * B * n, "%s: %d of %d entries dropped" % (name, len(dropped), B * n)
        rec = {"model": case["kind"], "n_keys": case["n_keys"], "B": B, "n": n,
               "points": [[float(v) for v in p] for p in case["points"]],
               "row_sums": [float(v) for v in case["counts"].sum(axis=1)], "tails": [float(v) for v in case["tails"]],
               "T": [r["T"] for r in per_point], "sp": [r["sp"] for r in per_point], "D": [r["D"] for r in per_point],
               "moved": [r["moved"] for r in per_point],
               "ll": [[per_point[i]["entries"][b]["ll"] for i in range(n)] for b in range(B)],
               "grad": [[per_point[i]["entries"][b]["grad"] for i in range(n)] for b in range(B)],
               "Cg": [[per_point[i]["entries"][b]["Cg"] for i in range(n)] for b in range(B)],
               "dropped": dropped, "special": special}
        if case["dead"]:
            rec["log10_dead_p"] = per_point[0]["log10_dead_p"]
        shapes[name] = rec
    assert total_dropped <= MAX_DROPPED_SHARE * total, "%d of %d entries dropped" % (total_dropped, total)
    print("%d entries, %d dropped (%.2f %%), %.0f s" % (total, total_dropped, 100.0 * total_dropped / total, time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_batch_grad.py",
           "what": "per shape of tests/batch_grad_shapes.py: ll[b][i], grad[b][i][k] and the condition sums Cg[b][i][k] of histogram b "
                   "at point i, restated in mpmath at 50 digits from ONE set of per-key rows a point; per point sp = sum p_j over "
                   "every key, threshold_o T, D_k = |sum d_k p_j| and which parameters the clamp moved (their components are 0); "
                   "`dropped`: the (b, i) left out and why; `special`: the (b, i) whose LL is -inf in a double (the dead key)",
           "k_tail": K_TAIL, "entries": total, "dropped": total_dropped, "shapes": shapes,
           "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    path = os.path.join(HERE, "batch_grad.json")
    with open(path, "w") as f:
        f.write(json.dumps(out, separators=(",", ":")).replace('},"', '},\n"'))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
