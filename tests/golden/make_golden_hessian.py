#!/usr/bin/env python3
"""Golden vectors for the closed-form Hessian of the log-likelihood (covest_eval_points_hess):
the formulas restated in mpmath at 50 digits, on top of the restatement of tests/golden/make_golden_gradient.py (imported,
not changed).  Nothing of the reference is run or read here.

The function differentiated is the gradient's: what the kernels evaluate, piece by piece, at the point after
fit_to_bounds, threshold_o = T held fixed, the two reference roundings kept in the weights and given no derivative.
Second derivatives term by term (hess_partial below): with x = o lambda_s, dx = o dlambda,
    d d'n  = comb_s e^-x (d d'x - dx d'x)
    d d'a  = (d d'n - da d'tot - d'a dtot - a d d'tot) / tot                       (0 where tot was replaced)
    d d'[a TP(x, j)] = TP(x, j) (alpha2 + j beta2 + j^2 gamma2),   L = log of the normaliser,
        gamma2 = a dx d'x / x^2
        beta2  = (da d'x + d'a dx) / x + a d d'x / x - 2 a L' dx d'x / x - a dx d'x / x^2
        alpha2 = d d'a - L' (da d'x + d'a dx) - a L' d d'x + a dx d'x (L'^2 - L'')
    (theta, q_k): the class's inner sum of d theta weighted by db_o / dq_k;  (q_k, q_l): the plain inner sum weighted by
    d2 b_o / dq_k dq_l
    d d'LL = sum_{h_j != 0} h_j [d d'p_j / p_j - dp_j d'p_j / p_j^2]
             - [tail != 0, sp < 1] tail [sum_j d d'p_j / (1 - sp) + (sum_j dp_j)(sum_j d'p_j) / (1 - sp)^2]
A row and column whose parameter the clamp moved are 0.

Candidates: every point tests/golden/gradient.json keeps.  Before anything is written the generator asserts
  1. its LL and gradient equal gradient.json's to 1e-15 relative (the same restatement);
  2. on the small cases (at most 32 keys, or H256) every entry of the SMOOTH function's Hessian (quantize=False) agrees
     with mpmath.diff of its own value -- (2,) on the diagonal, (1, 1) off it -- to 1e-20 of the entry's condition sum
     C_kl, the e entries AT e = 0 excepted as in the gradient's generator;
  3. selection: with delta = 8 eps n_keys (tests/parity_helpers.py K_TAIL), an entry's tail slack
     s_kl = |tail| (D_kl delta / (1 - sp)^2 + 2 D_k D_l delta / (1 - sp)^3) must not exceed 1e-9 C_kl; a candidate with a
     failing entry is DROPPED and counted;
and the conditions on the fixture: at least 50 points kept, and at least one kept in each of basic / repeats x tail 0 /
tail != 0, the full H10k_rep, e = 0, a clamped parameter, each recorded optimum.

Writes DATA ONLY: tests/golden/hessian.json.  Needs the built library for the model's host code (no GPU).
Usage:  python tests/golden/make_golden_hessian.py     (COVEST_GOLDEN_PROCS worker processes, default 8)
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
import make_golden_gradient as G  # noqa: E402  (the restatement: log_norm, dlog_norm, weights, consts_of, ll_only, ...)

mp.dps = 50
K_TAIL = G.K_TAIL
EPS = G.EPS
SPEC_KEYS = ("model", "hist", "k", "r", "tail", "max_error", "max_cov", "threshold", "min_single_copy_ratio")
PAIRS = [(k, l) for k in range(5) for l in range(k, 5)]  # row by row, k <= l
PAIR_AT = {kl: i for i, kl in enumerate(PAIRS)}
N_ROW = 1 + 5 + len(PAIRS)  # p, dp[5], d2p[15]


def d2log_norm(x):
    if x <= G.SMALL:
        return -1 / x ** 2
    n, xr = G.residual(x)
    if xr <= G.SMALL:
        return -1 / x ** 2
    t = mp.exp(-xr)
    return -t / (1 - t) ** 2


def weights2(q1, q2, q, o):
    """d2 b_o: (q1q2, q1q, q2q, qq); q1q1 = q2q2 = 0."""
    if o == 1:
        return mpf(0), mpf(0), mpf(0), mpf(0)
    if o == 2:
        return mpf(-1), mpf(0), mpf(0), mpf(0)
    n = o - 3
    g = q * (1 - q) ** n
    g1 = mpf(1) if n == 0 else (1 - q) ** n - n * q * (1 - q) ** (n - 1)
    g2 = mpf(0)
    if n > 0:
        g2 -= 2 * n * (1 - q) ** (n - 1)
    if n > 1:
        g2 += n * (n - 1) * q * (1 - q) ** (n - 2)
    return g, -(1 - q2) * g1, -(1 - q1) * g1, (1 - q1) * (1 - q2) * g2


def coef2(a, da, dap, d2a, dx, dxp, d2x, x, l1, l2):
    xx = dx * dxp
    cross = da * dxp + dap * dx
    ga = a * xx / x ** 2
    be = (cross + a * d2x - 2 * a * l1 * xx) / x - ga
    al = d2a - l1 * cross - a * l1 * d2x + a * xx * (l1 ** 2 - l2)
    return al, be, ga


def hess_partial(consts, theta, o_lo, o_hi, quantize=True):
    """The copy numbers o_lo <= o < o_hi's share of p_j, its five first and fifteen second derivatives, for every evaluated
    key: a list of [p, dp (5), d2p (15, PAIRS order)] per key.  quantize as in make_golden_gradient.grad_partial."""
    k, r, comb, repeats, keys = consts
    c, e = theta[0], theta[1]
    q1, q2, q = (theta[2], theta[3], theta[4]) if repeats else (mpf(1), mpf(0), mpf(0))
    S = len(comb)
    ck1 = mpf(r - k + 1) / r
    ck = c * (r - k + 1) / r
    lam, dlc, dle, dlce, dlee = [], [], [], [], []
    for s in range(S):
        ks = k - s
        lam.append(ck * mpf(3) ** -s * (1 - e) ** ks * e ** s)
        dlc.append(ck1 * mpf(3) ** -s * (1 - e) ** ks * e ** s)
        d, d2 = mpf(0), mpf(0)
        if s > 0:
            d += s * e ** (s - 1) * (1 - e) ** ks
        if ks > 0:
            d -= ks * e ** s * (1 - e) ** (ks - 1)
        if s > 1:
            d2 += s * (s - 1) * e ** (s - 2) * (1 - e) ** ks
        if s > 0 and ks > 0:
            d2 -= 2 * s * ks * e ** (s - 1) * (1 - e) ** (ks - 1)
        if ks > 1:
            d2 += ks * (ks - 1) * e ** s * (1 - e) ** (ks - 2)
        dle.append(ck * mpf(3) ** -s * d)
        dlce.append(ck1 * mpf(3) ** -s * d)
        dlee.append(ck * mpf(3) ** -s * d2)
    j_of = {}
    for at, j in enumerate(keys):
        j_of.setdefault(max(j, 0), []).append(at)
    j_max = max(j_of) if j_of else 0
    out = [[mpf(0)] * N_ROW for _ in keys]
    for o in range(o_lo, o_hi):
        x = [o * l for l in lam]
        ex = [mp.exp(-v) for v in x]
        n = [comb[s] * (1 - (mpf(float(ex[s])) if quantize else ex[s])) for s in range(S)]
        tot = mp.fsum(n)
        replaced = tot == 0
        if replaced:
            tot = mpf(1)
        a = [v / tot for v in n]
        dxc = [o * v for v in dlc]
        dxe = [o * v for v in dle]
        d2xce = [o * v for v in dlce]
        d2xee = [o * v for v in dlee]
        cex = [comb[s] * ex[s] for s in range(S)]
        dnc = [cex[s] * dxc[s] for s in range(S)]
        dne = [cex[s] * dxe[s] for s in range(S)]
        d2ncc = [-cex[s] * dxc[s] ** 2 for s in range(S)]
        d2nce = [cex[s] * (d2xce[s] - dxc[s] * dxe[s]) for s in range(S)]
        d2nee = [cex[s] * (d2xee[s] - dxe[s] ** 2) for s in range(S)]
        sc, se, scc, sce, see = mp.fsum(dnc), mp.fsum(dne), mp.fsum(d2ncc), mp.fsum(d2nce), mp.fsum(d2nee)
        zero = mpf(0)
        dac = [zero if replaced else (dnc[s] - a[s] * sc) / tot for s in range(S)]
        dae = [zero if replaced else (dne[s] - a[s] * se) / tot for s in range(S)]
        d2acc = [zero if replaced else (d2ncc[s] - 2 * dac[s] * sc - a[s] * scc) / tot for s in range(S)]
        d2ace = [zero if replaced else (d2nce[s] - dac[s] * se - dae[s] * sc - a[s] * sce) / tot for s in range(S)]
        d2aee = [zero if replaced else (d2nee[s] - 2 * dae[s] * se - a[s] * see) / tot for s in range(S)]
        inner = [[mpf(0)] * 6 for _ in keys]  # plain, c, e, cc, ce, ee
        for s in range(S):
            if not x[s] > 0:
                continue  # TP(0, j) = 0 as the kernels have it
            z = mp.exp(-G.log_norm(x[s], quantize))
            l1, l2 = G.dlog_norm(x[s]), d2log_norm(x[s])
            A = a[s] * z
            alc = (dac[s] - a[s] * l1 * dxc[s]) * z
            bec = a[s] * dxc[s] / x[s] * z
            ale = (dae[s] - a[s] * l1 * dxe[s]) * z
            bee = a[s] * dxe[s] / x[s] * z
            cc = [v * z for v in coef2(a[s], dac[s], dac[s], d2acc[s], dxc[s], dxc[s], zero, x[s], l1, l2)]
            ce = [v * z for v in coef2(a[s], dac[s], dae[s], d2ace[s], dxc[s], dxe[s], d2xce[s], x[s], l1, l2)]
            ee = [v * z for v in coef2(a[s], dae[s], dae[s], d2aee[s], dxe[s], dxe[s], d2xee[s], x[s], l1, l2)]
            if A == 0 and alc == 0 and ale == 0 and not any(cc) and not any(ce) and not any(ee):
                continue
            u = mpf(1)
            for j in range(0, j_max + 1):
                if j > 0:
                    u = u * x[s] / j
                if j in j_of:
                    v0 = A * u
                    v1 = u * (alc + j * bec)
                    v2 = u * (ale + j * bee)
                    v3 = u * (cc[0] + j * (cc[1] + j * cc[2]))
                    v4 = u * (ce[0] + j * (ce[1] + j * ce[2]))
                    v5 = u * (ee[0] + j * (ee[1] + j * ee[2]))
                    for at in j_of[j]:
                        row = inner[at]
                        row[0] += v0
                        row[1] += v1
                        row[2] += v2
                        row[3] += v3
                        row[4] += v4
                        row[5] += v5
        if repeats:
            b, db1, db2, db3 = G.weights(q1, q2, q, o)
            d12, d1q, d2q, dqq = weights2(q1, q2, q, o)
        else:
            b, db1, db2, db3, d12, d1q, d2q, dqq = (mpf(1),) + (mpf(0),) * 7
        db = (db1, db2, db3)
        for at in range(len(keys)):
            row, acc = inner[at], out[at]
            acc[0] += b * row[0]
            acc[1] += b * row[1]
            acc[2] += b * row[2]
            acc[6 + PAIR_AT[(0, 0)]] += b * row[3]
            acc[6 + PAIR_AT[(0, 1)]] += b * row[4]
            acc[6 + PAIR_AT[(1, 1)]] += b * row[5]
            if repeats:
                for t in range(3):
                    acc[3 + t] += db[t] * row[0]
                    acc[6 + PAIR_AT[(0, 2 + t)]] += db[t] * row[1]
                    acc[6 + PAIR_AT[(1, 2 + t)]] += db[t] * row[2]
                acc[6 + PAIR_AT[(2, 3)]] += d12 * row[0]
                acc[6 + PAIR_AT[(2, 4)]] += d1q * row[0]
                acc[6 + PAIR_AT[(3, 4)]] += d2q * row[0]
                acc[6 + PAIR_AT[(4, 4)]] += dqq * row[0]
    return out


def finish_hess(rows, counts, tail, P):
    """(ll, sp, grad[P], Cg[P], D[P], hess[P][P], C[P][P], D2[P][P]) from the per-key rows."""
    ll, sp, grad, Cg, D = G.finish([row[:6] for row in rows], counts, tail, P)
    tail_on = tail != 0 and sp < 1
    dsp = [mp.fsum(row[1 + d] for row in rows) for d in range(P)]
    H = [[mpf(0)] * P for _ in range(P)]
    C = [[mpf(0)] * P for _ in range(P)]
    D2 = [[mpf(0)] * P for _ in range(P)]
    for k in range(P):
        for l in range(k, P):
            at = 6 + PAIR_AT[(k, l)]
            t1 = [h * row[at] / row[0] for row, h in zip(rows, counts) if h != 0 and row[0] > 0]
            t2 = [h * row[1 + k] * row[1 + l] / row[0] ** 2 for row, h in zip(rows, counts) if h != 0 and row[0] > 0]
            d2sp = mp.fsum(row[at] for row in rows)
            ta = tail * d2sp / (1 - sp) if tail_on else mpf(0)
            tb = tail * dsp[k] * dsp[l] / (1 - sp) ** 2 if tail_on else mpf(0)
            H[k][l] = H[l][k] = mp.fsum(t1) - mp.fsum(t2) - ta - tb
            C[k][l] = C[l][k] = mp.fsum(abs(v) for v in t1) + mp.fsum(abs(v) for v in t2) + abs(ta) + abs(tb)
            D2[k][l] = D2[l][k] = abs(d2sp)
    return ll, sp, grad, Cg, D, H, C, D2


def spec_of(case):
    return {key: case[key] for key in SPEC_KEYS if key in case}


def _task(args):
    spec, point, T, o_lo, o_hi = args
    mp.dps = 50
    m, consts, counts, n_keys = G.consts_of(spec)
    theta = [mpf(float(v)) for v in m.fit_to_bounds(point)]
    return hess_partial(consts, theta, o_lo, o_hi)


def _check_task(args):
    """Assertion 2 for one point: [(k, l, |closed form - mpmath.diff| / C_kl)] of the smooth function."""
    spec, point, T = args
    mp.dps = 50
    m, consts, counts, n_keys = G.consts_of(spec)
    P = m.param_count
    clamped = m.fit_to_bounds(point)
    moved = [float(a) != float(b) for a, b in zip(point, clamped)]
    theta = [mpf(float(v)) for v in clamped]
    smooth = finish_hess(hess_partial(consts, theta, 1, T, quantize=False), counts, spec["tail"], P)
    H, C = smooth[5], smooth[6]
    out = []
    for k in range(P):
        for l in range(k, P):
            if moved[k] or moved[l] or (theta[1] == 0 and 1 in (k, l)):
                continue
            if k == l:
                def f(v, k=k):
                    th = list(theta)
                    th[k] = v
                    return G.ll_only(spec, th, T)
                num = mp.diff(f, theta[k], 2)
            else:
                def f(v, w, k=k, l=l):
                    th = list(theta)
                    th[k], th[l] = v, w
                    return G.ll_only(spec, th, T)
                num = mp.diff(f, (theta[k], theta[l]), (1, 1))
            err = abs(num - H[k][l]) / C[k][l] if C[k][l] != 0 else abs(num - H[k][l])
            out.append((k, l, float(err), mp.nstr(H[k][l], 30), mp.nstr(num, 30)))
    return out


def main():
    procs = int(os.environ.get("COVEST_GOLDEN_PROCS", "8"))
    t0 = time.time()
    gradient = G.load_json("gradient.json")
    own = G.load_json("own_optimum.json")["models"]
    optimum = {"basic": [own["basic"]["coverage"], own["basic"]["error_rate"]],
               "repeats": [own["repeats"][n] for n in ("coverage", "error_rate", "q1", "q2", "q")]}
    cases = gradient["cases"]
    tasks, where = [], []
    n_cand = 0
    for ci, case in enumerate(cases):
        spec = spec_of(case)
        m, consts, counts, n_keys = G.consts_of(spec)
        assert n_keys == case["n_keys"]
        for pi, point in enumerate(case["points"]):
            n_cand += 1
            T = case["T"][pi]
            work = len(consts[4]) * max(T - 1, 1)
            n_cut = max(1, min(T - 1, int(work // 20000)))
            edges = [1 + (T - 1) * i // n_cut for i in range(n_cut + 1)]
            for lo, hi in zip(edges[:-1], edges[1:]):
                tasks.append((spec, point, T, lo, hi))
                where.append((ci, pi))
    print("%d candidates in %d tasks" % (n_cand, len(tasks)), flush=True)
    with multiprocessing.Pool(procs) as pool:
        parts = pool.map(_task, tasks, chunksize=1)
        rows_of = {}
        for key, part in zip(where, parts):
            if key not in rows_of:
                rows_of[key] = part
            else:
                for acc, row in zip(rows_of[key], part):
                    for d in range(N_ROW):
                        acc[d] += row[d]
        print("partial sums done, %.0f s" % (time.time() - t0), flush=True)
        # ---- finish, assertion 1, selection
        out_cases, kept, dropped, worst_same, worst_ratio = [], 0, 0, 0.0, 0.0
        seen = set()
        check_tasks = []
        for ci, case in enumerate(cases):
            spec = spec_of(case)
            m, consts, counts, n_keys = G.consts_of(spec)
            P, tail = m.param_count, spec["tail"]
            rec = dict(spec, source=case["source"], n_keys=n_keys, points=[], T=[], ll=[], sp=[], grad=[], Cg=[], D=[],
                       moved=[], hess=[], C=[], D2=[])
            for pi, point in enumerate(case["points"]):
                T = case["T"][pi]
                ll, sp, grad, Cg, D, H, C, D2 = finish_hess(rows_of[(ci, pi)], counts, tail, P)
                clamped = m.fit_to_bounds(point)
                moved = [float(a) != float(b) for a, b in zip(point, clamped)]
                grad = [mpf(0) if mv else g for g, mv in zip(grad, moved)]
                H = [[mpf(0) if moved[k] or moved[l] else H[k][l] for l in range(P)] for k in range(P)]
                # assertion 1: the same restatement as gradient.json's
                same = abs(float(ll) - case["ll"][pi]) / abs(case["ll"][pi])
                for d in range(P):
                    want = case["grad"][pi][d]
                    same = max(same, abs(float(grad[d]) - want) / abs(want) if want != 0 else abs(float(grad[d])))
                worst_same = max(worst_same, same)
                assert same <= 1e-15, "value or gradient off gradient.json's: %s %r: %.3g" % (case["source"], point, same)
                # rule 3
                ok = True
                if tail != 0 and sp < 1:
                    delta = K_TAIL * EPS * n_keys
                    for k in range(P):
                        for l in range(k, P):
                            if moved[k] or moved[l]:
                                continue
                            s_kl = abs(tail) * (D2[k][l] * delta / (1 - sp) ** 2 + 2 * D[k] * D[l] * delta / (1 - sp) ** 3)
                            ratio = float(s_kl / (mpf(10) ** -9 * C[k][l])) if C[k][l] != 0 else (0.0 if s_kl == 0 else float("inf"))
                            if not ratio <= 1.0:
                                ok = False
                                print("  drop %s %r: entry (%d, %d) s_kl / (1e-9 C_kl) = %.3g, 1 - sp = %.3g" % (
                                    case["source"], point, k, l, ratio, float(1 - sp)), flush=True)
                            else:
                                worst_ratio = max(worst_ratio, ratio)
                if not ok:
                    dropped += 1
                    continue
                if len(consts[4]) <= 32 or spec["hist"] == "H256":
                    check_tasks.append((spec, point, T))
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
                rec["T"].append(T)
                rec["ll"].append(float(ll))
                rec["sp"].append(float(sp))
                rec["grad"].append([float(g) for g in grad])
                rec["Cg"].append([float(v) for v in Cg])
                rec["D"].append([float(v) for v in D])
                rec["moved"].append([bool(v) for v in moved])
                rec["hess"].append([[float(v) for v in row] for row in H])
                rec["C"].append([[float(v) for v in row] for row in C])
                rec["D2"].append([[float(v) for v in row] for row in D2])
            if rec["points"]:
                out_cases.append(rec)
        # ---- assertion 2
        print("%d kept, %d dropped; checking %d small points against mpmath.diff" % (kept, dropped, len(check_tasks)), flush=True)
        worst_diff, checked_diff = 0.0, 0
        for (spec, point, T), res in zip(check_tasks, pool.map(_check_task, check_tasks, chunksize=1)):
            for k, l, err, closed, num in res:
                worst_diff = max(worst_diff, err)
                checked_diff += 1
                assert err <= 1e-20, "Hessian off mpmath.diff: %r %r entry (%d, %d): %s vs %s (%.3g)" % (
                    spec, point, k, l, closed, num, err)
    need = {"basic/tail 0", "basic/tail != 0", "repeats/tail 0", "repeats/tail != 0", "full H10k_rep", "e = 0", "clamped",
            "optimum basic", "optimum repeats"}
    assert kept >= 50, "only %d of %d candidates kept" % (kept, n_cand)
    assert need <= seen, "no kept point in: %s" % sorted(need - seen)
    print("kept %d points, dropped %d of %d candidates (worst kept s_kl / (1e-9 C_kl) %.3g); value and gradient equal "
          "gradient.json's to %.3g; %d entries checked against mpmath.diff (worst %.3g relative to C_kl); %.0f s" % (
              kept, dropped, n_cand, worst_ratio, worst_same, checked_diff, worst_diff, time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_hessian.py",
           "what": "log-likelihood, sp = sum p_j, the analytic gradient and the closed-form Hessian (of what the kernels "
                   "evaluate, after fit_to_bounds, threshold_o = T fixed) restated in mpmath at 50 digits, with the condition "
                   "sums Cg_k, D_k = |sum dp| of the gradient (as tests/golden/gradient.json's C, D) and per entry "
                   "C_kl = sum (|h dd'p/p| + |h dp d'p/p^2|) + |tail sum dd'p / (1 - sp)| + |tail sum dp sum d'p / (1 - sp)^2|, "
                   "D2_kl = |sum dd'p|",
           "k_tail": K_TAIL, "kept": kept, "dropped": dropped, "candidates": n_cand,
           "worst_diff_check": worst_diff, "entries_diff_checked": checked_diff, "cases": out_cases,
           "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    path = os.path.join(HERE, "hessian.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
