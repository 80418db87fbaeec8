#!/usr/bin/env python3
"""Golden vectors for the derivative kernel (ll_deriv.hip) at the shapes its LAYOUT can break: value, gradient, Hessian and
outer product of the scores at 50 digits, on synthetic histograms chosen for the kernel's cuts, not for their parameters.

The kernel cuts a wave into OT = 64 / S copy-number tiles of S = n_err error classes (lane % S, lane / S), walks
threshold_o - 1 copy numbers OT at a time, gives a workgroup a segment of 256 keys and a wave 64 of them.  The candidates:
  keys    n_keys in {1, 64, 65, 255, 256, 257, 513}, basic and repeats, tail 0 and > 0, two points each; the repeat model's
          two points at threshold_o - 1 = 3 (below OT) and 3 OT + 1 (several tiles and one), S = 9 (an idle lane) without
          a tail and S = 8 with one;
  tile    a 65-key histogram, S in {1, 2, 6, 9, 22, 32, 64} (k = 31 for 32, k = 63 for 64 = min(k + 1, 64), the largest a
          model may have), threshold_o - 1 in {1, 2, 3, 4, OT - 1, OT, OT + 1, 2 OT + 1} reached through `threshold`
          and q; and 300 copy numbers at S = 22 on a 70-key histogram;
  feature a zero-count key in the middle and as the last key of the last segment, keys descending, shuffled, with gaps and
          starting above 1, an isolated key 3000 with count 2 in a segment of its own -- with a normal p_j, and with
          p_j = 0 (LL = -inf: kept by its own rule, section "neg_inf");
  param   e in {0, 1e-9, 0.5}, c on its lower bound and large enough that o lambda_s > 200, q in {0, 1}, q1 = 1,
          q2 in {0, 1}, a parameter outside its bound -- each on a histogram of more than one segment;
  subnormal  a counted key whose p_j is a subnormal double while LL is finite (section "subnormal": with p_j and, per
          component, the bound h |d_k p / p| 2^-52 / (p / 2^-1074) on that key's share of the gradient).  The coverages were
          found by bisection on c of this restatement's p_j (--search prints them).

No formula is written here: the restatements are make_golden_gradient.py's, make_golden_hessian.py's and
make_golden_opg.py's, imported (hess_partial's rows hold grad_partial's; finish_hess, finish_opg, K_TAIL, the mpmath.diff
check).  Nothing of the reference is run or read.

Before anything is written the generator asserts -- properties of the reference numbers alone --
  1. every point's threshold_o is the one its class names;
  2. selection, make_golden_hessian.py's rule with the gradient's and the outer product's beside it: a finite LL, no counted
     p_j below 1e-300, with a tail |1 - sp| >= 1e-6, the tail term in neither the graded nor the flip class, and every
     component's and entry's tail slack (delta = 8 eps n_keys) within 1e-9 of its condition sum; a candidate that fails is
     DROPPED and counted, at most 10 % may be; and no component x = o lambda_s > 200 may sit just above a multiple of 200,
     its residual xr = x - 200 n below 1e-5 x: the reference's chunked normaliser has L' = 1 / (1 - e^-xr) ~ 1 / xr and
     L'' ~ -1 / xr^2 there, which move by x / xr times the rounding of x, and a double's x = o lambda_s carries a few
     2^-52 -- beyond x / xr = 1e5 no double evaluation holds 1e-9 of the condition sums (the first draw had 25 x 16.000003
     = 400.00008 at 256 keys: the Hessian's c-c entry 9e-9 off, the rounding of xr alone 3e-9);
  3. coverage: every (model, key count), every (S, threshold_o - 1) pair, every feature and parameter edge, each model
     with tail 0 and with a tail keep a point; the -inf and the subnormal cases are kept by their own rules;
  4. on the cases of at most 65 keys every Hessian entry of the smooth function agrees with mpmath.diff of its own value to
     1e-20 of the entry's condition sum (make_golden_hessian._check_task).

Writes DATA ONLY: tests/golden/deriv_shapes.json; matrices as upper triangles (k <= l, row by row), histograms inline as
key and count arrays in dictionary order.  Needs the built library for the model's host code (no GPU).
Usage:  python tests/golden/make_golden_deriv_shapes.py     (COVEST_GOLDEN_PROCS worker processes, default 8, at most 16)
"""
import json
import os
import sys
import time

import multiprocessing

import mpmath
from mpmath import mp, mpf

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gradient as G  # noqa: E402  (the restatement; puts tests/ on the path)
import make_golden_hessian as H2  # noqa: E402
import make_golden_opg as O  # noqa: E402
from parity_helpers import _tail_slack  # noqa: E402

mp.dps = 50
K_TAIL = G.K_TAIL
EPS = G.EPS
MAX_PROCS = 16
MAX_DROPPED_SHARE = 0.10
KEY_COUNTS = (1, 64, 65, 255, 256, 257, 513)
TILE_S = ((1, 21), (2, 21), (6, 21), (9, 21), (22, 21), (32, 31), (64, 63))  # (S = max_error, k)
ISOLATED = 3000


# ---------------------------------------------------------------------------------------------- histograms (integers only)
def _counts(keys, mode, width, top):
    return [1 + top * width * width // (width * width + (j - mode) ** 2) for j in keys]


def _hist(keys, mode, width, top=4000):
    return {"keys": list(keys), "counts": _counts(keys, mode, width, top)}


def _with(hist, **counts_at):
    out = {"keys": list(hist["keys"]), "counts": list(hist["counts"])}
    for at, v in counts_at.items():
        out["counts"][int(at[1:])] = v
    return out


def histograms():
    H = {}
    for n in KEY_COUNTS:
        H["keys%d" % n] = _hist([30] if n == 1 else range(1, n + 1), 30 if n == 1 else 7 * n // 10, max(4, n // 6))
    H["tile65"] = _hist(list(range(1, 63)) + [70, 90, 131], 25, 15)
    H["tile70"] = _hist(list(range(1, 67)) + [80, 120, 200, 330], 25, 15)
    asc = _hist(range(1, 301), 200, 50)
    H["asc300"] = asc
    H["zero_mid300"] = _with(asc, i149=0)
    H["zero_last512"] = _with(_hist(range(1, 513), 350, 80), i511=0)
    H["desc300"] = {"keys": asc["keys"][::-1], "counts": asc["counts"][::-1]}
    order = sorted(range(300), key=lambda i: (i * 2654435761) % 4294967296)
    H["shuffled300"] = {"keys": [asc["keys"][i] for i in order], "counts": [asc["counts"][i] for i in order]}
    gaps, j = [], 5
    for i in range(130):
        gaps.append(j)
        j += 2 if i % 2 == 0 else 3
    H["gaps130"] = _hist(gaps, 200, 50)
    iso = _hist(list(range(1, 257)) + [ISOLATED], 60, 40)
    iso["counts"][-1] = 2
    H["isolated257"] = iso  # 256 keys fill the first segment: the isolated key has the second to itself
    low = _hist(range(2, 302), 4, 6)
    low["counts"] = [h if j <= 30 else 0 for j, h in zip(low["keys"], low["counts"])]
    H["low300"] = low  # c on its lower bound: only the keys to 30 are counted, the rest weigh in sp alone
    return H


HISTS = histograms()


# ---------------------------------------------------------------------------------------------- candidates
def _round(v):
    return float("%.6g" % v)


def c_of(lam0, e, k=21, r=100):
    """The coverage at which the error-free rate lambda_0 = c (r - k + 1) / r (1 - e)^k is lam0."""
    return _round(lam0 / ((r - k + 1) / r * (1 - e) ** k))


def rep_q(Tm1, q, q1=0.6, q2=0.5):
    """(q1, q2, q) and the model's `threshold` at which threshold_o - 1 = Tm1."""
    T = Tm1 + 1
    head = (1 - q1) * (1 - q2) * q
    if T == 2:
        thr = ((1 - q1) * q2 + q1) / 2
    elif T == 3:
        thr = (1 - q1) * q2 * q ** 0.5
    else:
        thr = head * (1 - q) ** (T - 3.5)
    return [q1, q2, q], _round(thr)


def spec_of(model, hist, tail, S=8, k=21, threshold=None):
    s = {"model": model, "hist": hist, "k": k, "r": 100, "tail": tail, "max_error": S}
    if threshold is not None:
        s["threshold"] = threshold
    return s


def tile_edges(S):
    OT = 64 // S
    return sorted({v for v in (1, 2, 3, 4, OT - 1, OT, OT + 1, 2 * OT + 1) if v >= 1})


def candidates():
    """[{"spec", "point", "cls": [class names], "Tm1": threshold_o - 1 expected (repeats), "kind"}]"""
    out = []

    def add(spec, point, cls, Tm1=None, kind="regular"):
        out.append({"spec": spec, "point": [float(v) for v in point], "cls": cls, "Tm1": Tm1, "kind": kind})

    def rep(hist, tail, S, k, lam0, e, Tm1, q, cls, **kw):
        qs, thr = rep_q(Tm1, q, **kw)
        add(spec_of("repeats", hist, tail, S, k, thr), [c_of(lam0, e, k), e] + qs, cls, Tm1)

    # ---- key-count edges
    for n in KEY_COUNTS:
        top = 30 if n == 1 else n
        for tail in (0, 37):
            tag = "tail0" if tail == 0 else "tail+"
            for lam0, e in ((0.9 * top, 0.02), (1.05 * top, 0.05)):
                add(spec_of("basic", "keys%d" % n, tail), [c_of(lam0, e), e], ["keys/basic/%d" % n, "keys/basic/%d/%s" % (n, tag)])
            S = 9 if tail == 0 else 8
            OT = 64 // S
            rep("keys%d" % n, tail, S, 21, 0.45 * top, 0.03, 3, 0.3,
                ["keys/repeats/%d" % n, "keys/repeats/%d/%s" % (n, tag), "keys/repeats/below OT"])
            rep("keys%d" % n, tail, S, 21, max(1.03 * top / 16.0, 1.2), 0.03, 3 * OT + 1, 0.08,
                ["keys/repeats/%d" % n, "keys/repeats/%d/%s" % (n, tag), "keys/repeats/tiles and one"])
    # ---- tile edges
    for S, k in TILE_S:
        for Tm1 in tile_edges(S):
            rep("tile65", 0, S, k, max(0.4, min(12.0, 45.0 / Tm1)), 0.03, Tm1, min(0.3, 2.0 / Tm1), ["tile/S%d/%d" % (S, Tm1)])
    rep("tile70", 0, 22, 21, 0.3, 0.03, 300, 0.01, ["tile/S22/hundreds"])
    # ---- histogram features
    for name, hist, tail, top in (("zero count in the middle", "zero_mid300", 29, 300), ("zero count last of the last segment", "zero_last512", 29, 512),
                                  ("descending", "desc300", 0, 300), ("shuffled", "shuffled300", 29, 300),
                                  ("gaps, above 1", "gaps130", 29, 330)):
        add(spec_of("basic", hist, tail), [c_of(1.0 * top, 0.03), 0.03], ["feature/%s/basic" % name])
        rep(hist, tail, 8, 21, 0.45 * top, 0.03, 3, 0.3, ["feature/%s/repeats" % name])
    add(spec_of("basic", "isolated257", 0), [c_of(2090.0, 0.1), 0.1], ["feature/isolated key/basic"])
    rep("isolated257", 0, 8, 21, 1530.0, 0.1, 2, 0.3, ["feature/isolated key/repeats"])
    add(spec_of("basic", "isolated257", 0), [c_of(60.0, 0.03), 0.03], ["feature/isolated key, p = 0/basic"], kind="neg_inf")
    # ---- parameter edges, more than one segment
    for e in (0.0, 1e-9, 0.5):
        add(spec_of("basic", "asc300", 0), [c_of(150.0, e), e], ["param/e = %g/basic" % e])
        rep("asc300", 0, 8, 21, 130.0, e, 3, 0.3, ["param/e = %g/repeats" % e])
    add(spec_of("basic", "low300", 25), [0.01, 0.03], ["param/c on its bound/basic"])
    rep("low300", 25, 8, 21, 1.0, 0.03, 3, 0.3, ["param/c on its bound/repeats"])
    out[-1]["point"][0] = 0.01
    add(spec_of("basic", "asc300", 0), [c_of(208.0, 0.02), 0.02], ["param/o lambda > 200/basic"])
    rep("asc300", 0, 8, 21, 60.0, 0.02, 4, 0.3, ["param/o lambda > 200/repeats"])
    add(spec_of("basic", "asc300", 0), [c_of(150.0, 0.0), -0.1], ["param/outside its bound/basic"])
    rep("asc300", 0, 8, 21, 103.0, 0.03, 3, 0.3, ["param/outside its bound/repeats"], q1=0.3)
    out[-1]["point"][2] = 0.1  # q1 below min_single_copy_ratio: clamped to 0.3
    cq = c_of(130.0, 0.03)
    rp = spec_of("repeats", "asc300", 0)  # the default threshold 1e-8: these q decide threshold_o by being 0
    add(rp, [cq, 0.03, 0.6, 0.5, 0.0], ["param/q = 0/repeats"], 2)
    add(rp, [cq, 0.03, 0.6, 0.5, 1.0], ["param/q = 1/repeats"], 3)
    add(rp, [c_of(200.0, 0.03), 0.03, 1.0, 0.5, 0.3], ["param/q1 = 1/repeats"], 1)
    add(rp, [c_of(200.0, 0.03), 0.03, 0.6, 0.0, 0.3], ["param/q2 = 0/repeats"], 1)
    add(rp, [cq, 0.03, 0.6, 1.0, 0.3], ["param/q2 = 1/repeats"], 2)
    # ---- a counted key with a subnormal p_j (the coverages: --search)
    add(spec_of("basic", "isolated257", 0), [SUBNORMAL_C["basic"], 0.1], ["subnormal/basic"], kind="subnormal")
    qs, thr = rep_q(3, 0.3)
    add(spec_of("repeats", "isolated257", 0, threshold=thr), [SUBNORMAL_C["repeats"], 0.1] + qs, ["subnormal/repeats"], 3, kind="subnormal")
    return out


SUBNORMAL_C = {"basic": 15744.6, "repeats": 5257.33}  # (--search's output)
SUBNORMAL_TARGET = -315  # log10 of the isolated key's p_j


def inline(spec):
    return dict(spec, hist=HISTS[spec["hist"]])


def search():
    """Bisection on c of the restated p_j of the isolated key, to SUBNORMAL_TARGET."""
    for model in ("basic", "repeats"):
        qs, thr = rep_q(3, 0.3)
        spec = inline(spec_of(model, "isolated257", 0, threshold=thr if model == "repeats" else None))
        m, consts, counts, n_keys = G.consts_of(spec)
        consts = consts[:4] + ([ISOLATED],)
        T = 4 if model == "repeats" else 2
        lo, hi = 10.0, 40000.0

        def log10_p(c):
            theta = [mpf(float(v)) for v in ([c, 0.1] + (qs if model == "repeats" else []))]
            return mp.log10(G.grad_partial(consts, theta, 1, T, with_grad=False)[0][0])

        for _ in range(40):
            mid = (lo + hi) / 2
            if log10_p(mid) < SUBNORMAL_TARGET:
                lo = mid
            else:
                hi = mid
        c = _round(hi)
        print("%s: c = %r, log10 p_j = %s" % (model, c, mp.nstr(log10_p(c), 8)), flush=True)


# ---------------------------------------------------------------------------------------------- the run
def tri(M, P):
    return [float(M[k][l]) for k in range(P) for l in range(k, P)]


def near_chunk(consts, theta, T):
    """Rule 2's last clause: the (o, s, x / xr) of a component just above a multiple of 200, or None."""
    k, r, comb = consts[:3]
    for s, lam in enumerate(G.class_rates(k, r, theta[0], theta[1], len(comb))):
        for o in range(1, T):
            x = o * lam
            if x > 200:
                xr = G.residual(x)[1]
                if xr < mpf(10) ** -5 * x:
                    return o, s, x / xr
    return None


def select(ll, sp, rows, counts, tail, n_keys, P, moved, Cg, D, C, D2, CB, sl):
    """Rule 2: None to keep the point, else why it is dropped."""
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
    bound = mpf(10) ** -9
    for k in range(P):
        if not moved[k] and not bound * Cg[k] >= abs(tail) * D[k] * delta / (1 - sp) ** 2:
            return "gradient component %d's tail slack" % k
        for l in range(k, P):
            if moved[k] or moved[l]:
                continue
            s_h = abs(tail) * (D2[k][l] * delta / (1 - sp) ** 2 + 2 * D[k] * D[l] * delta / (1 - sp) ** 3)
            if not s_h <= bound * C[k][l]:
                return "Hessian entry (%d, %d)'s tail slack" % (k, l)
            if not sl[k][l] * delta <= bound * CB[k][l]:
                return "outer-product entry (%d, %d)'s tail slack" % (k, l)
    return None


def main():
    procs = min(MAX_PROCS, int(os.environ.get("COVEST_GOLDEN_PROCS", "8")))
    t0 = time.time()
    cands = candidates()
    tasks, where = [], []
    for ci, cand in enumerate(cands):
        spec = inline(cand["spec"])
        m, consts, counts, n_keys = G.consts_of(spec)
        clamped = m.fit_to_bounds(cand["point"])
        T = int(m.get_hist_threshold_values([clamped[2:5]])[0]) if spec["model"] == "repeats" else 2
        if cand["Tm1"] is not None:  # assertion 1
            assert T - 1 == cand["Tm1"], "threshold_o - 1 is %d, not %d: %r %r" % (T - 1, cand["Tm1"], cand["spec"], cand["point"])
        cand["T"] = T
        work = len(consts[2]) * (T - 1) * (max(consts[4]) + 1)
        n_cut = max(1, min(T - 1, int(work // 60000)))
        edges = [1 + (T - 1) * i // n_cut for i in range(n_cut + 1)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            tasks.append((work // n_cut, (spec, cand["point"], T, lo, hi)))
            where.append(ci)
    order = sorted(range(len(tasks)), key=lambda i: -tasks[i][0])  # the long ones first
    print("%d candidates in %d tasks, %d processes" % (len(cands), len(tasks), procs), flush=True)
    with multiprocessing.Pool(procs) as pool:
        parts = pool.map(H2._task, [tasks[i][1] for i in order], chunksize=1)
        rows_of = {}
        for i, part in zip(order, parts):
            ci = where[i]
            if ci not in rows_of:
                rows_of[ci] = part
            else:
                for acc, row in zip(rows_of[ci], part):
                    for d in range(H2.N_ROW):
                        acc[d] += row[d]
        print("partial sums done, %.0f s" % (time.time() - t0), flush=True)
        cases, case_at = [], {}
        neg_inf, subnormal, check_tasks = [], [], []
        kept, dropped, seen = 0, 0, {}
        for ci, cand in enumerate(cands):
            spec = inline(cand["spec"])
            m, consts, counts, n_keys = G.consts_of(spec)
            P, tail, rows, point, T = m.param_count, spec["tail"], rows_of[ci], cand["point"], cand["T"]
            ll, sp, grad, Cg, D, Hm, C, D2 = H2.finish_hess(rows, counts, tail, P)
            B, CB, sl = O.finish_opg([row[:6] for row in rows], counts, tail, P)[6:]
            moved = [float(a) != float(b) for a, b in zip(point, m.fit_to_bounds(point))]
            grad = [mpf(0) if mv else g for g, mv in zip(grad, moved)]
            zero = lambda M: [[mpf(0) if moved[k] or moved[l] else M[k][l] for l in range(P)] for k in range(P)]  # noqa: E731
            Hm, B = zero(Hm), zero(B)
            if cand["kind"] != "regular":
                at = consts[4].index(ISOLATED)
                p, h = rows[at][0], counts[at]
                others = min(row[0] for i, (row, hh) in enumerate(zip(rows, counts)) if hh != 0 and i != at)
                assert h != 0 and others >= mpf(10) ** -300 and tail == 0
                rec = dict(cand["spec"], cls=cand["cls"], point=point, T=T, key=ISOLATED, h=h)
                if cand["kind"] == "neg_inf":  # its own rule: p_j far below the smallest subnormal double
                    assert 0 < p < mpf(10) ** -400  # (0 in a double: LL = -inf there)
                    rec["log10_p"] = float(mp.log10(p))
                    neg_inf.append(rec)
                else:  # its own rule: p_j a subnormal double of at least a thousand units, LL finite
                    assert mpf(2) ** -1064 < p < mpf(2) ** -1022 and mp.isfinite(ll), mp.nstr(p, 5)
                    rec.update(p=float(p), ll=float(ll), grad=[float(g) for g in grad], Cg=[float(v) for v in Cg],
                               bound=[float(h * abs(rows[at][1 + d] / p) * mpf(2) ** -52 / (p / mpf(2) ** -1074)) for d in range(P)])
                    subnormal.append(rec)
                for c in cand["cls"]:
                    seen[c] = seen.get(c, 0) + 1
                continue
            why = select(ll, sp, rows, counts, tail, n_keys, P, moved, Cg, D, C, D2, CB, sl)
            near = near_chunk(consts, [mpf(float(v)) for v in m.fit_to_bounds(point)], T)
            if why is None and near is not None:
                why = "copy number %d, class %d: x / xr = %s above a multiple of 200" % (near[0], near[1], mp.nstr(near[2], 3))
            if why is not None:
                dropped += 1
                print("  drop %r %r: %s" % (cand["cls"], point, why), flush=True)
                continue
            kept += 1
            for c in cand["cls"] + ["%s/%s" % (spec["model"], "tail0" if tail == 0 else "tail+")]:
                seen[c] = seen.get(c, 0) + 1
            if len(consts[4]) <= 65:
                check_tasks.append((spec, point, T))
            key = json.dumps(cand["spec"], sort_keys=True)
            if key not in case_at:
                case_at[key] = len(cases)
                cases.append(dict(cand["spec"], n_keys=n_keys, points=[], cls=[], T=[], ll=[], sp=[], grad=[], Cg=[], D=[], moved=[],
                                  hess=[], C=[], D2=[], opg=[], Cb=[]))
            rec = cases[case_at[key]]
            rec["points"].append(point)
            rec["cls"].append(cand["cls"])
            rec["T"].append(T)
            rec["ll"].append(float(ll))
            rec["sp"].append(float(sp))
            rec["grad"].append([float(g) for g in grad])
            rec["Cg"].append([float(v) for v in Cg])
            rec["D"].append([float(v) for v in D])
            rec["moved"].append([bool(v) for v in moved])
            for name, M in (("hess", Hm), ("C", C), ("D2", D2), ("opg", B), ("Cb", CB)):
                rec[name].append(tri(M, P))
        # ---- rules 2 and 3
        n_cand = len(cands)
        assert dropped <= MAX_DROPPED_SHARE * n_cand, "%d of %d candidates dropped" % (dropped, n_cand)
        need = ["keys/%s/%d" % (model, n) for model in ("basic", "repeats") for n in KEY_COUNTS]
        need += ["keys/repeats/below OT", "keys/repeats/tiles and one", "tile/S22/hundreds"]
        need += ["tile/S%d/%d" % (S, v) for S, k in TILE_S for v in tile_edges(S)]
        need += ["%s/%s" % (model, t) for model in ("basic", "repeats") for t in ("tail0", "tail+")]
        need += sorted({c for cand in cands for c in cand["cls"] if c.startswith(("feature/", "param/", "subnormal/"))})
        missing = [c for c in need if not seen.get(c)]
        assert not missing, "no kept point in: %s" % missing
        assert len(neg_inf) == 1 and len(subnormal) == 2
        # ---- assertion 4
        print("%d kept, %d dropped; checking %d points of at most 65 keys against mpmath.diff, %.0f s" % (
            kept, dropped, len(check_tasks), time.time() - t0), flush=True)
        worst_diff, checked_diff = 0.0, 0
        for (spec, point, T), res in zip(check_tasks, pool.map(H2._check_task, check_tasks, chunksize=1)):
            for k, l, err, closed, num in res:
                worst_diff = max(worst_diff, err)
                checked_diff += 1
                assert err <= 1e-20, "Hessian off mpmath.diff: %r entry (%d, %d): %s vs %s (%.3g)" % (point, k, l, closed, num, err)
    print("kept %d points (and the -inf case and %d subnormal ones), dropped %d of %d candidates; %d classes; %d entries checked "
          "against mpmath.diff (worst %.3g relative to C_kl); %.0f s" % (kept, len(subnormal), dropped, n_cand, len(seen), checked_diff,
                                                                        worst_diff, time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_deriv_shapes.py",
           "what": "per point of a case: log-likelihood, sp = sum p_j, threshold_o T, the analytic gradient with its condition "
                   "sums Cg_k and D_k = |sum d_k p|, the closed-form Hessian `hess` with C_kl and D2_kl = |sum d_k d_l p| "
                   "(tests/golden/hessian.json's), the outer product of the scores `opg` with its condition sum Cb_kl "
                   "(tests/golden/opg.json's C), restated in mpmath at 50 digits; matrices as upper triangles, k <= l row by "
                   "row; `cls` the shape classes a point stands for; `hists` the histograms, keys and counts in dictionary order",
           "k_tail": K_TAIL, "kept": kept, "dropped": dropped, "candidates": n_cand, "classes": dict(sorted(seen.items())),
           "worst_diff_check": worst_diff, "entries_diff_checked": checked_diff, "hists": HISTS, "cases": cases,
           "neg_inf": neg_inf, "subnormal": subnormal, "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    path = os.path.join(HERE, "deriv_shapes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        main()
