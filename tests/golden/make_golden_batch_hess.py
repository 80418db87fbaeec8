#!/usr/bin/env python3
"""Golden vectors for the Hessian of a histogram batch (covest_batch_eval_cross_hess / _pairs_hess):
the closed-form Hessian of every stored histogram of a batch at every point, at 50 digits.

No formula is written here.  The restatement is make_golden_hessian.py's, imported (hess_partial, finish_hess), and the batch
identity is restated by how it is called: per shape and point the per-key rows [p, d_k p ..., d_k d_l p ...] are computed
ONCE, over every key of the model, and finish_hess(rows, counts_b, tail_b, P) is called per histogram.  The shapes are
tests/batch_hess_shapes.py's: tests/batch_grad_shapes.py's unchanged and two repeats shapes with n = 3 and 4 (21 n table
rows either side of a wave's 64).  Nothing of the reference is run or read.

Selection is make_golden_deriv_shapes.py's `select`, imported, for the Hessian entries -- a finite LL, no counted p_j below
1e-300, with a tail |1 - sp| >= 1e-6 and the tail term in neither the graded nor the flip class, the gradient's and every
Hessian entry's tail slack (delta = 8 eps n_keys; C, D2) within 1e-9 of its condition sum (its outer-product clause is
handed a slack of 0: there is no outer product here) -- plus its near_chunk.  An entry that fails is DROPPED and counted
with its reason -- the dead-key shapes' special entry (LL = -inf in a double) excepted, as in batch_grad.json -- and at
most 5 % of the stored entries of any shape, and of the whole, may be dropped: asserted before anything is written.  If
the cap is exceeded the points move in tests/batch_hess_shapes.py, not the rule and not tests/batch_grad_shapes.py.

Rows stored: batch_hess_shapes.stored_rows -- every row below B = 15; from there the model's-own-counts row, the two
all-zero rows, the first and the last seeded row (the file stays below tests/golden/kmer_hist.json's size, the largest
fixture committed; asserted).

Writes DATA ONLY: tests/golden/batch_hess.json -- per shape the stored rows, per point sp, D_k = |sum d_k p|,
D2_kl = |sum d_k d_l p| and which parameters the clamp moved, per stored (b, i) the packed Hessian (k <= l, row by row; a
row and column of a moved parameter 0) and its condition sums C_kl (9 digits: they enter a bound only).  ll and grad are
pinned by tests/golden/batch_grad.json and not stored again.  Needs the built library for the model's host code (no GPU).
Usage:  python tests/golden/make_golden_batch_hess.py     (COVEST_GOLDEN_PROCS worker processes, default 8, at most 16)
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
import make_golden_gradient as G  # noqa: E402  (consts_of; puts the repository and tests/ on the path)
import make_golden_hessian as H2  # noqa: E402  (the restatement: hess_partial, finish_hess)
import make_golden_deriv_shapes as DS  # noqa: E402  (select, near_chunk, tri)
import batch_hess_shapes as S  # noqa: E402

mp.dps = 50
K_TAIL = G.K_TAIL
MAX_PROCS = 16
MAX_DROPPED_SHARE = 0.05
LARGEST_FIXTURE = "kmer_hist.json"


def _nine(v):
    return float("%.9g" % float(v))


def _task(args):
    """One (shape, point): the rows once, then every stored histogram of the shape."""
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
    rows = H2.hess_partial(consts, theta, 1, T)
    near = DS.near_chunk(consts, theta, T)
    ones = [[mpf(1)] * P for _ in range(P)]
    none = [[mpf(0)] * P for _ in range(P)]
    out = {"moved": moved, "entries": {}}
    for b in S.stored_rows(name):
        counts = [int(v) for v in case["counts"][b]]
        tail = int(case["tails"][b])
        ll, sp, grad, Cg, D, Hm, C, D2 = H2.finish_hess(rows, counts, tail, P)
        Hm = [[mpf(0) if moved[k] or moved[l] else Hm[k][l] for l in range(P)] for k in range(P)]
        why = DS.select(ll, sp, rows, counts, tail, n_keys, P, moved, Cg, D, C, D2, ones, none)
        if why is None and near is not None:
            why = "copy number %d, class %d: x / xr = %s above a multiple of 200" % (near[0], near[1], mp.nstr(near[2], 3))
        special = bool(case["dead"] and i == 0 and b == case["rows"]["dead"])
        if special:  # (make_golden_batch_grad.py asserts what makes it one)
            assert rows[consts[4].index(S.ISOLATED)][0] < mpf(10) ** -400 and counts[consts[4].index(S.ISOLATED)] != 0
            why = None
        out["entries"][b] = {"hess": None if special else DS.tri(Hm, P), "C": [_nine(v) for v in DS.tri(C, P)], "why": why,
                             "special": special}
        out["sp"], out["D"], out["D2"] = float(sp), [float(v) for v in D], [_nine(v) for v in DS.tri(D2, P)]
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
        stored = S.stored_rows(name)
        per_point = [result[(name, i)] for i in range(n)]
        dropped = [[b, i, per_point[i]["entries"][b]["why"]] for i in range(n) for b in stored if per_point[i]["entries"][b]["why"]]
        special = [[b, i] for i in range(n) for b in stored if per_point[i]["entries"][b]["special"]]
        assert len(special) == (1 if case["dead"] else 0)
        total += len(stored) * n
        total_dropped += len(dropped)
        print("%-24s %4d entries, %d dropped%s" % (name, len(stored) * n, len(dropped),
                                                    "".join("\n    (%d, %d): %s" % tuple(d) for d in dropped)), flush=True)
        assert len(dropped) <= MAX_DROPPED_SHARE * len(stored) * n, "%s: %d of %d entries dropped" % (name, len(dropped), len(stored) * n)
        shapes[name] = {"model": case["kind"], "n_keys": case["n_keys"], "B": B, "n": n, "base": case["base"], "rows": stored,
                        "points": [[float(v) for v in p] for p in case["points"]],
                        "row_sums": [float(v) for v in case["counts"].sum(axis=1)], "tails": [float(v) for v in case["tails"]],
                        "sp": [r["sp"] for r in per_point], "D": [r["D"] for r in per_point], "D2": [r["D2"] for r in per_point],
                        "moved": [r["moved"] for r in per_point],
                        "hess": [[per_point[i]["entries"][b]["hess"] for i in range(n)] for b in stored],
                        "C": [[per_point[i]["entries"][b]["C"] for i in range(n)] for b in stored],
                        "dropped": dropped, "special": special}
    assert total_dropped <= MAX_DROPPED_SHARE * total, "%d of %d entries dropped" % (total_dropped, total)
    print("%d entries, %d dropped (%.2f %%), %.0f s" % (total, total_dropped, 100.0 * total_dropped / total, time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_batch_hess.py",
           "what": "per shape of tests/batch_hess_shapes.py and stored row `rows`[at]: hess[at][i], the closed-form Hessian of "
                   "histogram rows[at] at point i as an upper triangle (k <= l, row by row), and its condition sums C[at][i], "
                   "restated in mpmath at 50 digits from ONE set of per-key rows a point; per point sp = sum p_j over every "
                   "key, D_k = |sum d_k p_j|, D2_kl = |sum d_k d_l p_j| and which parameters the clamp moved (their rows and "
                   "columns are 0); `dropped`: the (b, i) left out and why; `special`: the (b, i) whose LL is -inf in a double; "
                   "`base`: the shape of tests/golden/batch_grad.json that pins ll and grad of the same (b, i)",
           "k_tail": K_TAIL, "entries": total, "dropped": total_dropped, "shapes": shapes,
           "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    text = json.dumps(out, separators=(",", ":")).replace('},"', '},\n"') + "\n"
    assert len(text) <= os.path.getsize(os.path.join(HERE, LARGEST_FIXTURE)), "%d bytes: store fewer rows" % len(text)
    path = os.path.join(HERE, "batch_hess.json")
    with open(path, "w") as f:
        f.write(text)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
