#!/usr/bin/env python3
"""Golden vectors for the outer product of the scores (covest_eval_points_opg): the meat B of the
sandwich covariance A^-1 B A^-1, restated in mpmath at 50 digits on the per-key rows [p, dp (5)] of
tests/golden/make_golden_gradient.py's grad_partial (imported, not changed).  Nothing of the reference is run or read.

The function differentiated is the gradient's: what the kernels evaluate, piece by piece, at the point after
fit_to_bounds, threshold_o = T held fixed, the two reference roundings kept in the weights and given no derivative.
With r_k(j) = d_k p_j / p_j, sp = sum_j p_j, S_k = sum_j d_k p_j over the evaluated keys, on = [tail != 0 and sp < 1]:
    B_kl = sum_{h_j != 0} h_j r_k(j) r_l(j)  +  on tail S_k S_l / (1 - sp)^2
the uncentred sum over k-mers of the outer product of their scores, the tail as one more class.  A row and column whose
parameter the clamp moved are 0.

Candidates: every point tests/golden/gradient.json keeps.  Before anything is written the generator asserts
  (a) its LL and gradient equal gradient.json's as doubles;
  (b) on the points tests/golden/hessian.json also keeps, the identity with the Hessian  B_kl = D_kl - H_kl,
      D_kl = sum h dd'p / p - on tail sum dd'p / (1 - sp),  with H and D recomputed from make_golden_hessian.py's rows
      (imported, not changed; that H rounds to hessian.json's doubles), to 1e-20 of the entry's condition sum C_kl: the
      new yardstick is tied to the one already checked against mpmath.diff;
  (c) selection: per entry the condition sum  C_kl = sum_j |h r_k r_l| + |on tail S_k S_l / (1 - sp)^2|  and the tail slack
      s_kl = |tail| 2 |S_k| |S_l| delta / (1 - sp)^3,  delta = 8 eps n_keys (tests/parity_helpers.py K_TAIL: the
      first-order propagation of the slack the parity suite grants sp); a candidate with an entry s_kl > 1e-9 C_kl is
      DROPPED and counted;
and the conditions on the fixture: at most 10 of the 70 candidates dropped, and at least one kept in each of basic /
repeats x tail 0 / tail != 0, the full H10k_rep, e = 0, a clamped parameter, each recorded optimum.

Writes DATA ONLY: tests/golden/opg.json.  Needs the built library for the model's host code (no GPU).
Usage:  python tests/golden/make_golden_opg.py     (COVEST_GOLDEN_PROCS worker processes, default 8)
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
import make_golden_gradient as G  # noqa: E402  (the restatement: grad_partial, finish, consts_of, ...)
import make_golden_hessian as H2  # noqa: E402  (hess_partial, finish_hess, PAIR_AT: assertion (b))

mp.dps = 50
K_TAIL = G.K_TAIL
EPS = G.EPS
MAX_DROPPED = 10


def finish_opg(rows, counts, tail, P):
    """(ll, sp, grad[P], Cg[P], D[P], S[P], B[P][P], C[P][P], s_over_delta[P][P]) from the per-key rows [p, dp ...]; the
    last is s_kl / delta = |tail| 2 |S_k| |S_l| / (1 - sp)^3 (0 without a live tail)."""
    ll, sp, grad, Cg, D = G.finish(rows, counts, tail, P)
    on = tail != 0 and sp < 1
    S = [mp.fsum(row[1 + d] for row in rows) for d in range(P)]
    counted = [(row, h) for row, h in zip(rows, counts) if h != 0 and row[0] > 0]
    B = [[mpf(0)] * P for _ in range(P)]
    C = [[mpf(0)] * P for _ in range(P)]
    sl = [[mpf(0)] * P for _ in range(P)]
    for k in range(P):
        for l in range(k, P):
            terms = [h * (row[1 + k] / row[0]) * (row[1 + l] / row[0]) for row, h in counted]
            t = tail * S[k] * S[l] / (1 - sp) ** 2 if on else mpf(0)
            B[k][l] = B[l][k] = mp.fsum(terms) + t
            C[k][l] = C[l][k] = mp.fsum(abs(v) for v in terms) + abs(t)
            sl[k][l] = sl[l][k] = abs(tail) * 2 * abs(S[k]) * abs(S[l]) / (1 - sp) ** 3 if on else mpf(0)
    return ll, sp, grad, Cg, D, S, B, C, sl


def identity_with_hessian(hrows, counts, tail, P, B, C):
    """Assertion (b) for one point: the worst |B_kl - (D_kl - H_kl)| / C_kl over its entries, and the Hessian (not zeroed
    for the clamp) the rows give."""
    out = H2.finish_hess(hrows, counts, tail, P)
    sp, Hm = out[1], out[5]
    on = tail != 0 and sp < 1
    worst = mpf(0)
    for k in range(P):
        for l in range(k, P):
            at = 6 + H2.PAIR_AT[(k, l)]
            Dkl = mp.fsum(h * row[at] / row[0] for row, h in zip(hrows, counts) if h != 0 and row[0] > 0)
            if on:
                Dkl -= tail * mp.fsum(row[at] for row in hrows) / (1 - sp)
            err = abs(B[k][l] - (Dkl - Hm[k][l]))
            worst = max(worst, err / C[k][l] if C[k][l] != 0 else err)
    return worst, Hm


def cut(n_keys_eval, T, per_task):
    work = n_keys_eval * max(T - 1, 1)
    n_cut = max(1, min(T - 1, int(work // per_task)))
    edges = [1 + (T - 1) * i // n_cut for i in range(n_cut + 1)]
    return list(zip(edges[:-1], edges[1:]))


def gather(pool, task, tasks, where, width):
    rows_of = {}
    for key, part in zip(where, pool.map(task, tasks, chunksize=1)):
        if key not in rows_of:
            rows_of[key] = part
        else:
            for acc, row in zip(rows_of[key], part):
                for d in range(width):
                    acc[d] += row[d]
    return rows_of


def main():
    procs = int(os.environ.get("COVEST_GOLDEN_PROCS", "8"))
    t0 = time.time()
    gradient = G.load_json("gradient.json")
    hessian = G.load_json("hessian.json")
    hess_of = {(c["source"], tuple(p)): (c["hess"][i], c["moved"][i]) for c in hessian["cases"] for i, p in enumerate(c["points"])}
    own = G.load_json("own_optimum.json")["models"]
    optimum = {"basic": [own["basic"]["coverage"], own["basic"]["error_rate"]],
               "repeats": [own["repeats"][n] for n in ("coverage", "error_rate", "q1", "q2", "q")]}
    cases = gradient["cases"]
    g_tasks, g_where, h_tasks, h_where = [], [], [], []
    n_cand = 0
    for ci, case in enumerate(cases):
        spec = H2.spec_of(case)
        m, consts, counts, n_keys = G.consts_of(spec)
        assert n_keys == case["n_keys"]
        for pi, point in enumerate(case["points"]):
            n_cand += 1
            T = case["T"][pi]
            for lo, hi in cut(len(consts[4]), T, 40000):
                g_tasks.append((spec, point, T, lo, hi))
                g_where.append((ci, pi))
            if (case["source"], tuple(point)) in hess_of:
                for lo, hi in cut(len(consts[4]), T, 20000):
                    h_tasks.append((spec, point, T, lo, hi))
                    h_where.append((ci, pi))
    print("%d candidates in %d tasks, %d more for the identity with the Hessian" % (n_cand, len(g_tasks), len(h_tasks)), flush=True)
    with multiprocessing.Pool(procs) as pool:
        rows_of = gather(pool, G._task, g_tasks, g_where, 6)
        hrows_of = gather(pool, H2._task, h_tasks, h_where, H2.N_ROW)
    print("partial sums done, %.0f s" % (time.time() - t0), flush=True)
    out_cases, kept, dropped = [], 0, 0
    worst_same, worst_ratio, worst_identity, n_identity = 0.0, 0.0, mpf(0), 0
    seen = set()
    for ci, case in enumerate(cases):
        spec = H2.spec_of(case)
        m, consts, counts, n_keys = G.consts_of(spec)
        P, tail = m.param_count, spec["tail"]
        delta = K_TAIL * EPS * n_keys
        rec = dict(spec, source=case["source"], n_keys=n_keys, points=[], T=[], ll=[], sp=[], grad=[], Cg=[], D=[], moved=[],
                   opg=[], C=[], s=[])
        for pi, point in enumerate(case["points"]):
            ll, sp, grad, Cg, D, S, B, C, sl = finish_opg(rows_of[(ci, pi)], counts, tail, P)
            clamped = m.fit_to_bounds(point)
            moved = [float(a) != float(b) for a, b in zip(point, clamped)]
            # (a) the same doubles as gradient.json's
            grad = [mpf(0) if mv else g for g, mv in zip(grad, moved)]
            same = 0.0 if float(ll) == case["ll"][pi] else abs(float(ll) - case["ll"][pi]) / abs(case["ll"][pi])
            for d in range(P):
                want = case["grad"][pi][d]
                if float(grad[d]) != want:
                    same = max(same, abs(float(grad[d]) - want) / abs(want) if want != 0 else abs(float(grad[d])))
            worst_same = max(worst_same, same)
            assert same == 0.0, "value or gradient off gradient.json's: %s %r: %.3g" % (case["source"], point, same)
            # (b) B = D - H on hessian.json's points
            if (ci, pi) in hrows_of:
                err, Hm = identity_with_hessian(hrows_of[(ci, pi)], counts, tail, P, B, C)
                stored, stored_moved = hess_of[(case["source"], tuple(point))]
                assert stored_moved == [bool(v) for v in moved]
                for k in range(P):
                    for l in range(P):
                        assert (0.0 if moved[k] or moved[l] else float(Hm[k][l])) == stored[k][l], (
                            "the recomputed Hessian is not hessian.json's", case["source"], point, k, l)
                worst_identity = max(worst_identity, err)
                n_identity += 1
                assert err <= mpf(10) ** -20, "B is not D - H: %s %r: %s of C_kl" % (case["source"], point, mp.nstr(err, 5))
            B = [[mpf(0) if moved[k] or moved[l] else B[k][l] for l in range(P)] for k in range(P)]
            # (c) the selection rule
            ok = True
            for k in range(P):
                for l in range(k, P):
                    if moved[k] or moved[l]:
                        continue
                    s_kl = sl[k][l] * delta
                    if s_kl == 0:
                        continue
                    ratio = float(s_kl / (mpf(10) ** -9 * C[k][l])) if C[k][l] != 0 else float("inf")
                    if not ratio <= 1.0:
                        ok = False
                        print("  drop %s %r: entry (%d, %d) s_kl / (1e-9 C_kl) = %.3g, 1 - sp = %.3g" % (
                            case["source"], point, k, l, ratio, float(1 - sp)), flush=True)
                    else:
                        worst_ratio = max(worst_ratio, ratio)
            if not ok:
                dropped += 1
                continue
            kept += 1
            kind = spec["model"]
            seen.add("%s/tail %s" % (kind, "0" if tail == 0 else "!= 0"))
            if spec["hist"] == "H10k_rep":
                seen.add("full H10k_rep")
            if float(clamped[1]) == 0.0:
                seen.add("e = 0")
            if any(moved):
                seen.add("clamped")
            if spec["hist"] == "sim_c10_e0.05" and [float(v) for v in point] == [float(v) for v in optimum[kind]]:
                seen.add("optimum " + kind)
            rec["points"].append([float(v) for v in point])
            rec["T"].append(case["T"][pi])
            rec["ll"].append(float(ll))
            rec["sp"].append(float(sp))
            rec["grad"].append([float(g) for g in grad])
            rec["Cg"].append([float(v) for v in Cg])
            rec["D"].append([float(v) for v in D])
            rec["moved"].append([bool(v) for v in moved])
            rec["opg"].append([[float(v) for v in row] for row in B])
            rec["C"].append([[float(v) for v in row] for row in C])
            rec["s"].append([[float(v * delta) for v in row] for row in sl])
        if rec["points"]:
            out_cases.append(rec)
    need = {"basic/tail 0", "basic/tail != 0", "repeats/tail 0", "repeats/tail != 0", "full H10k_rep", "e = 0", "clamped",
            "optimum basic", "optimum repeats"}
    assert dropped <= MAX_DROPPED, "%d of %d candidates dropped, at most %d may be" % (dropped, n_cand, MAX_DROPPED)
    assert need <= seen, "no kept point in: %s" % sorted(need - seen)
    print("kept %d points, dropped %d of %d candidates (worst kept s_kl / (1e-9 C_kl) %.3g); value and gradient equal "
          "gradient.json's to %.3g; B = D - H on %d points of hessian.json (worst %s relative to C_kl); %.0f s" % (
              kept, dropped, n_cand, worst_ratio, worst_same, n_identity, mp.nstr(worst_identity, 3), time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_opg.py",
           "what": "log-likelihood, sp = sum p_j, the analytic gradient and the outer product of the scores "
                   "B_kl = sum h (d_k p / p)(d_l p / p) + on tail S_k S_l / (1 - sp)^2 (of what the kernels evaluate, after "
                   "fit_to_bounds, threshold_o = T fixed) restated in mpmath at 50 digits, with the condition sums Cg_k, "
                   "D_k = |S_k| = |sum d_k p| of the gradient (as tests/golden/gradient.json's C, D) and per entry "
                   "C_kl = sum |h r_k r_l| + |on tail S_k S_l / (1 - sp)^2| and the tail slack "
                   "s_kl = |tail| 2 |S_k| |S_l| delta / (1 - sp)^3, delta = k_tail eps n_keys",
           "k_tail": K_TAIL, "kept": kept, "dropped": dropped, "candidates": n_cand,
           "worst_identity_check": float(worst_identity), "points_identity_checked": n_identity, "cases": out_cases,
           "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    path = os.path.join(HERE, "opg.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
