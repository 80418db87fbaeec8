#!/usr/bin/env python3
"""Golden vectors for the analytic gradient of the log-likelihood (covest_eval_points_grad):
the formulas restated in mpmath at 50 digits.  Nothing of the reference is run or read here; its recorded VALUES
(tests/golden/basic_ll.json, repeats_ll.json, c3_trim.json, c2_trim.json) are what the restatement's own value is
checked against.

The function differentiated is what the kernels evaluate, piece by piece, at the point after fit_to_bounds, with
threshold_o = T held fixed:
    ck = c (r - k + 1) / r,  lambda_s = ck 3^-s (1 - e)^(k - s) e^s
    per copy number o < T and class s:  x = o lambda_s,  n_os = comb_s (1 - exp(-x)),  a_os = n_os / tot_o  (tot_o = 1 if 0)
    TP(x, j) = x^j / j! / exp(L(x)),  L the log of the normaliser the reference divides by (200-chunk pieces); TP(0, j) = 0
    p_j = sum_o b_o sum_s a_os TP(o lambda_s, j),  LL = sum_j h_j log p_j + tail log(1 - sp),  sp = sum_j p_j  (sp < 1)
and its gradient term by term (d lambda_s, d n_os, d a_os, L'(x), d b_o: see grad_partial below).  A component whose
parameter the clamp moved is 0.

Before anything is written the generator asserts
  1. its LL agrees with the reference's recorded value to 1e-9 relative wherever the point comes from a fixture;
  2. its analytic gradient agrees with mpmath.diff of its own LL to 1e-25 relative to the condition sum C_k on the small
     cases (at most 32 keys or H256; 50 digits carried, a first difference loses half), both taken of the smooth
     function (grad_partial quantize=False) -- except the e component AT
     e = 0, where the one-sided derivative of the continuous function has a term the piecewise definition TP(0, j) = 0
     leaves out;
  3. every point kept has a finite LL and no counted p_j below 1e-300, its sp is not within 1e-6 of 1, its tail term is in neither the graded nor the
     flip class of tests/parity_helpers.py _tail_slack (there the reference's own value hangs on the rounding of sp and
     the plain 1e-9 of assertion 1 does not apply), and
     1e-9 C_k >= |tail| D_k delta / (1 - sp)^2 with delta = 8 eps n_keys (tests/parity_helpers.py K_TAIL)
     for every component: candidates that fail are DROPPED and counted (before assertion 1).

Writes DATA ONLY: tests/golden/gradient.json.  Needs the built library for threshold_o (host code, no GPU).
Usage:  python tests/golden/make_golden_gradient.py     (COVEST_GOLDEN_PROCS worker processes, default 8)
"""
import json
import math
import multiprocessing
import os
import sys
import time

import mpmath
from mpmath import mp, mpf

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from covest_amd.models import BasicModel, RepeatsModel  # noqa: E402  (bounds, comb, fit_to_bounds, threshold_o: host code)
from parity_helpers import _tail_slack  # noqa: E402

mp.dps = 50
K_TAIL = 8.0
EPS = 2.0 ** -52
SMALL = mpf(1e-8)  # the double the extension compares with


def load(name):
    """The histogram `name`.hist -- or one given inline as {"keys": [...], "counts": [...]}, dictionary order as listed
    (tests/golden/make_golden_deriv_shapes.py)."""
    if not isinstance(name, str):
        return {int(j): h for j, h in zip(name["keys"], name["counts"])}
    hist = {}
    with open(os.path.join(HERE, name + ".hist")) as f:
        for line in f:
            if line.strip() and line[0] != "#":
                a, b = line.split()[:2]
                hist[int(a)] = int(b)
    return hist


def load_json(name):
    with open(os.path.join(HERE, name)) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- the restatement
def residual(x):
    """(n, xr): x = 200 n + xr with xr in (0, 200]."""
    if x <= 200:
        return 0, x
    n = mp.ceil(x / 200) - 1
    return n, x - 200 * n


def log_norm(x, quantize):
    if x <= SMALL:
        return mp.log(x)
    n, xr = residual(x)
    if xr <= SMALL:
        return 200 * n + mp.log(x)
    m = mp.expm1(xr)
    if quantize and xr < mpf(2) ** -10:
        m = mp.nint(m * mpf(2) ** 63) / mpf(2) ** 63  # expl(x) - 1 of the x87: e^x lies on the 2^-63 grid
    return 200 * n + mp.log(m)


def dlog_norm(x):
    if x <= SMALL:
        return 1 / x
    n, xr = residual(x)
    if xr <= SMALL:
        return 1 / x
    return 1 / (1 - mp.exp(-xr))


def class_rates(k, r, c, e, S):
    """lambda_s = ck 3^-s (1 - e)^(k - s) e^s for s < S, ck = c (r - k + 1) / r."""
    ck = c * (r - k + 1) / r
    return [ck * mpf(3) ** -s * (1 - e) ** (k - s) * e ** s for s in range(S)]


def weights(q1, q2, q, o):
    """b_o and its derivatives in q1, q2, q."""
    if o == 1:
        return q1, mpf(1), mpf(0), mpf(0)
    if o == 2:
        return (1 - q1) * q2, -q2, 1 - q1, mpf(0)
    w = (1 - q) ** (o - 3)
    dq = (1 - q1) * (1 - q2) * (mpf(1) if o == 3 else w - (o - 3) * q * (1 - q) ** (o - 4))
    return (1 - q1) * (1 - q2) * q * w, -(1 - q2) * q * w, -(1 - q1) * q * w, dq


def grad_partial(consts, theta, o_lo, o_hi, with_grad=True, quantize=True):
    """The copy numbers o_lo <= o < o_hi's share of p_j and of its five derivatives, for every evaluated key:
    a list of [p, dp/dc, dp/de, dp/dq1, dp/dq2, dp/dq] per key.
    quantize: the two roundings of the reference that the kernels reproduce because its VALUE hangs on them --
    n_os = comb_s (1 - exp(-x)) with exp(-x) rounded to a double first (for x ~ 1e-17 that is all of n_os, and comb_s is
    up to 2.5e8), and the 2^-63 grid under the normaliser of a small residual.  Both are step functions: rounding noise
    without a derivative, the derivatives below are those of the smooth expressions.  quantize=False is the smooth
    function itself, the one mpmath.diff can be asked about."""
    k, r, comb, repeats, keys = consts
    c, e = theta[0], theta[1]
    q1, q2, q = (theta[2], theta[3], theta[4]) if repeats else (mpf(1), mpf(0), mpf(0))
    S = len(comb)
    ck = c * (r - k + 1) / r
    lam, dlc, dle = class_rates(k, r, c, e, S), [], []
    for s in range(S):
        dlc.append(lam[s] / c)
        d = mpf(0)
        if s > 0:
            d += s * e ** (s - 1) * (1 - e) ** (k - s)
        if k - s > 0:
            d -= (k - s) * e ** s * (1 - e) ** (k - s - 1)
        dle.append(ck * mpf(3) ** -s * d)
    j_of = {}
    for at, j in enumerate(keys):
        j_of.setdefault(max(j, 0), []).append(at)  # (the extension's product loop is empty for j <= 0)
    j_max = max(j_of) if j_of else 0
    out = [[mpf(0)] * 6 for _ in keys]
    for o in range(o_lo, o_hi):
        x = [o * l for l in lam]
        ex = [mp.exp(-v) for v in x]
        n = [comb[s] * (1 - (mpf(float(ex[s])) if quantize else ex[s])) for s in range(S)]
        tot = mp.fsum(n)
        replaced = tot == 0
        if replaced:
            tot = mpf(1)
        a = [v / tot for v in n]
        dnc = [comb[s] * ex[s] * o * dlc[s] for s in range(S)]
        dne = [comb[s] * ex[s] * o * dle[s] for s in range(S)]
        sc, se = mp.fsum(dnc), mp.fsum(dne)
        dac = [mpf(0) if replaced else (dnc[s] - a[s] * sc) / tot for s in range(S)]
        dae = [mpf(0) if replaced else (dne[s] - a[s] * se) / tot for s in range(S)]
        inner = [[mpf(0)] * 3 for _ in keys]
        for s in range(S):
            if not x[s] > 0:
                continue  # TP(0, j) = 0 as the kernels have it
            z = mp.exp(-log_norm(x[s], quantize))
            dl = dlog_norm(x[s])
            A = a[s] * z
            alc = (dac[s] - a[s] * dl * o * dlc[s]) * z
            bec = a[s] * o * dlc[s] / x[s] * z
            ale = (dae[s] - a[s] * dl * o * dle[s]) * z
            bee = a[s] * o * dle[s] / x[s] * z
            if A == 0 and alc == 0 and ale == 0:
                continue
            u = mpf(1)
            for j in range(0, j_max + 1):
                if j > 0:
                    u = u * x[s] / j
                if j in j_of:
                    for at in j_of[j]:
                        row = inner[at]
                        row[0] += A * u
                        if with_grad:
                            row[1] += u * (alc + j * bec)
                            row[2] += u * (ale + j * bee)
        b, db1, db2, db3 = weights(q1, q2, q, o) if repeats else (mpf(1), mpf(0), mpf(0), mpf(0))
        for at in range(len(keys)):
            row, acc = inner[at], out[at]
            acc[0] += b * row[0]
            if with_grad:
                acc[1] += b * row[1]
                acc[2] += b * row[2]
                acc[3] += db1 * row[0]
                acc[4] += db2 * row[0]
                acc[5] += db3 * row[0]
    return out


def finish(rows, counts, tail, P):
    """(ll, sp, grad[P], C[P], D[P]) from the per-key [p, dp ...]."""
    sp = mp.fsum(row[0] for row in rows)
    tail_on = tail != 0 and sp < 1
    ll = mpf(0)
    for row, h in zip(rows, counts):
        if h != 0:
            ll += h * mp.log(row[0]) if row[0] > 0 else -mp.inf
    if tail_on:
        ll += tail * mp.log(1 - sp)
    grad, C, D = [], [], []
    for d in range(P):
        terms = [h * row[1 + d] / row[0] for row, h in zip(rows, counts) if h != 0 and row[0] > 0]
        dsp = mp.fsum(row[1 + d] for row in rows)
        t = tail * dsp / (1 - sp) if tail_on else mpf(0)
        grad.append(mp.fsum(terms) - t)
        C.append(mp.fsum(abs(v) for v in terms) + abs(t))
        D.append(abs(dsp))
    return ll, sp, grad, C, D


# ---------------------------------------------------------------------------------------------- cases
def make_model(spec):
    hist = load(spec["hist"])
    if spec["model"] == "repeats":
        m = RepeatsModel(spec["k"], spec["r"], hist, spec["tail"], max_error=spec["max_error"],
                         threshold=spec.get("threshold", 1e-8), min_single_copy_ratio=spec.get("min_single_copy_ratio", 0.3))
    else:
        m = BasicModel(spec["k"], spec["r"], hist, spec["tail"], max_error=spec["max_error"], max_cov=spec.get("max_cov"))
    return m, hist


def consts_of(spec):
    m, hist = make_model(spec)
    items = [(j, h) for j, h in hist.items() if spec["tail"] != 0 or h != 0]  # tail 0: keys with h = 0 weigh nothing
    keys = [j for j, _ in items]
    counts = [h for _, h in items]
    comb = [mpf(v) for v in m.comb[:m.max_error]]
    return m, (spec["k"], spec["r"], comb, spec["model"] == "repeats", keys), counts, len(hist)


def _task(args):
    spec, point, T, o_lo, o_hi = args
    mp.dps = 50
    m, consts, counts, n_keys = consts_of(spec)
    theta = [mpf(float(v)) for v in m.fit_to_bounds(point)]
    return grad_partial(consts, theta, o_lo, o_hi)


def ll_only(spec, theta, T):
    """The smooth function's value (see grad_partial)."""
    m, consts, counts, n_keys = consts_of(spec)
    rows = grad_partial(consts, theta, 1, T, with_grad=False, quantize=False)
    return finish(rows, counts, spec["tail"], 0)[0]


def fixture_cases():
    """[(spec, [(point, reference ll or None)])]"""
    out = []
    basic, rep = load_json("basic_ll.json")["cases"], load_json("repeats_ll.json")["cases"]

    def spec_of(case, model):
        s = {"model": model, "hist": case["hist"], "k": case["k"], "r": case["r"], "tail": case["tail"],
             "max_error": case["max_error"]}
        for key in ("max_cov", "threshold", "min_single_copy_ratio"):
            if key in case:
                s[key] = case[key]
        return s

    def pick(case, idx):
        return [(case["points"][i], case["ll"][i]) for i in idx if i < len(case["points"])]

    out.append((spec_of(basic[0], "basic"), pick(basic[0], range(0, 55, 6)), "basic_ll.json[0]"))
    out.append((spec_of(basic[1], "basic"), pick(basic[1], range(1, 55, 7)), "basic_ll.json[1]"))
    out.append((spec_of(basic[2], "basic"), pick(basic[2], (7, 23)), "basic_ll.json[2]"))
    out.append((spec_of(basic[12], "basic"), pick(basic[12], range(4)), "basic_ll.json[12]"))
    out.append((spec_of(basic[13], "basic"), pick(basic[13], range(0, 20, 5)), "basic_ll.json[13]"))
    out.append((spec_of(rep[0], "repeats"), pick(rep[0], range(0, 72, 7)), "repeats_ll.json[0]"))
    out.append((spec_of(rep[1], "repeats"), pick(rep[1], range(3, 72, 8)), "repeats_ll.json[1]"))
    out.append((spec_of(rep[2], "repeats"), pick(rep[2], (4, 17)), "repeats_ll.json[2]"))
    out.append((spec_of(rep[9], "repeats"), pick(rep[9], (2, 9, 16)), "repeats_ll.json[9]"))
    # the trimmed 10 000-key histograms with their tails: candidates of the arg-min (1 - sp ~ 1e-4 .. 1e-5) and seeded points
    c3 = load_json("c3_trim.json")
    axes = [c3["axes"][0], c3["axes"][1], c3["axes"][2], [c3["q2"]], c3["axes"][3]]

    def c3_point(flat):
        coord = []
        for a in reversed(axes):
            coord.append(a[flat % len(a)])
            flat //= len(a)
        return list(reversed(coord))

    cand = c3["candidates"]
    known = dict(zip(cand["flat_index"], cand["ll"]))
    known.update(zip(c3["flat_index"], c3["ll"]))
    chosen = [cand["reference_argmin_flat"], 149105, 157281, 132449] + list(c3["flat_index"][5:400:97])
    spec = {"model": "repeats", "hist": c3["hist"], "k": c3["k"], "r": c3["r"], "tail": c3["tail"], "max_error": c3["max_error"]}
    out.append((spec, [(c3_point(f), known[f]) for f in chosen], "c3_trim.json"))
    c2 = load_json("c2_trim.json")
    import numpy as np
    cs, es = np.linspace(2000.0, 6000.0, 1000), np.linspace(0.001, 0.1, 1000)
    cand = c2["candidates"]
    known = dict(zip(cand["flat_index"], cand["ll"]))
    known.update(zip(c2["flat_index"], c2["ll"]))
    chosen = [cand["reference_argmin_flat"], 500192, 496191, 530183] + list(c2["flat_index"][3:1024:170])
    spec = {"model": "basic", "hist": c2["hist"], "k": c2["k"], "r": c2["r"], "tail": c2["tail"], "max_error": c2["max_error"]}
    out.append((spec, [([float(cs[f // 1000]), float(es[f % 1000])], known[f]) for f in chosen], "c2_trim.json"))
    return out


def own_cases():
    opt = load_json("own_optimum.json")["models"]
    sim = {"hist": "sim_c10_e0.05", "k": 21, "r": 100, "tail": 0, "max_error": 8}
    b, rp = opt["basic"], opt["repeats"]
    out = [
        (dict(sim, model="basic"), [([b["coverage"], b["error_rate"]], None)], "own_optimum.json basic"),
        (dict(sim, model="repeats"), [([rp["coverage"], rp["error_rate"], rp["q1"], rp["q2"], rp["q"]], None),
                                      # the normaliser's pieces: o lambda_0 up to 329 (> 200) and just above 400
                                      ([30.0, 0.001, 0.5, 0.5, 0.05], None), ([36.5, 0.001, 0.5, 0.5, 0.05], None),
                                      # q near 0 and near 1, parameters on and outside their bounds
                                      ([10.0, 0.05, 0.6, 0.5, 0.001], None), ([10.0, 0.05, 0.6, 0.5, 0.999], None),
                                      ([10.0, 0.05, 0.3, 0.0, 1.0], None), ([10.0, 0.5, 1.0, 1.0, 0.0], None),
                                      ([0.001, 0.7, 0.1, -0.2, 1.3], None), ([9.0, 0.0, 0.8, 0.4, 0.3], None)],
         "own: sim_c10_e0.05, repeats"),
        ({"model": "basic", "hist": "H256", "k": 21, "r": 100, "tail": 0, "max_error": 8},
         [([100.0, 0.02], None), ([90.0, 0.03], None), ([400.0, 0.01], None), ([618.0, 0.01], None)], "own: H256"),
        ({"model": "basic", "hist": "H256", "k": 21, "r": 100, "tail": 25, "max_error": 8},
         [([100.0, 0.02], None), ([95.0, 0.025], None)], "own: H256 with a tail"),
        ({"model": "repeats", "hist": "H10k_rep", "k": 21, "r": 100, "tail": 0, "max_error": 8},
         [([24.0, 0.025, 0.6, 0.5, 0.1], None)], "own: the full H10k_rep, threshold_o in the hundreds"),
    ]
    return out


def main():
    procs = int(os.environ.get("COVEST_GOLDEN_PROCS", "8"))
    t0 = time.time()
    cases = fixture_cases() + own_cases()
    # ---- every point's partial sums, the long ones cut into runs of copy numbers
    tasks, where = [], []
    info = []
    for ci, (spec, pts, source) in enumerate(cases):
        m, consts, counts, n_keys = consts_of(spec)
        for pi, (point, ref) in enumerate(pts):
            clamped = m.fit_to_bounds(point)
            T = int(m.get_hist_threshold_values([clamped[2:5]])[0]) if spec["model"] == "repeats" else 2
            work = len(consts[4]) * max(T - 1, 1)
            n_cut = max(1, min(T - 1, int(work // 40000)))
            edges = [1 + (T - 1) * i // n_cut for i in range(n_cut + 1)]
            for lo, hi in zip(edges[:-1], edges[1:]):
                tasks.append((spec, point, T, lo, hi))
                where.append((ci, pi))
            info.append((ci, pi, T))
    print("%d points in %d tasks" % (len(info), len(tasks)), flush=True)
    with multiprocessing.Pool(procs) as pool:
        parts = pool.map(_task, tasks, chunksize=1)
    rows_of = {}
    for key, part in zip(where, parts):
        if key not in rows_of:
            rows_of[key] = part
        else:
            for acc, row in zip(rows_of[key], part):
                for d in range(6):
                    acc[d] += row[d]
    # ---- finish, assert, select
    out_cases, dropped, kept, checked_ref, checked_diff = [], 0, 0, 0, 0
    worst_ref, worst_diff = 0.0, 0.0
    for ci, (spec, pts, source) in enumerate(cases):
        m, consts, counts, n_keys = consts_of(spec)
        P = m.param_count
        rec = dict(spec, source=source, n_keys=n_keys, points=[], T=[], ll=[], sp=[], grad=[], C=[], D=[])
        for pi, (point, ref) in enumerate(pts):
            T = [t for c, p, t in info if (c, p) == (ci, pi)][0]
            ll, sp, grad, C, D = finish(rows_of[(ci, pi)], counts, spec["tail"], P)
            clamped = m.fit_to_bounds(point)
            moved = [float(a) != float(b) for a, b in zip(point, clamped)]
            grad = [mpf(0) if mv else g for g, mv in zip(grad, moved)]
            p_min = min([row[0] for row, h in zip(rows_of[(ci, pi)], counts) if h != 0] or [mpf(1)])
            if not mp.isfinite(ll) or p_min < mpf(10) ** -300 or (ref is not None and not math.isfinite(ref)):
                dropped += 1  # (a counted p_j that a double cannot hold: the value is -inf, or hangs on subnormal roundings)
                continue
            tail = spec["tail"]
            ok = True
            if tail != 0:  # rule 3, and the tail term's own conditioning (tests/parity_helpers.py: graded / flip)
                if abs(1 - sp) < 1e-6 or _tail_slack(tail, float(ll), float(sp), n_keys)[1] is not None:
                    ok = False
                elif sp < 1:
                    delta = K_TAIL * EPS * n_keys
                    for d in range(P):
                        if not moved[d] and not 1e-9 * C[d] >= abs(tail) * D[d] * delta / (1 - sp) ** 2:
                            ok = False
            if not ok:
                dropped += 1
                continue
            if ref is not None:  # assertion 1
                err = abs(float(ll) - ref) / abs(ref)
                worst_ref = max(worst_ref, err)
                assert err <= 1e-9, "value off the reference's: %s %r: %r vs %r (%.3g)" % (source, point, float(ll), ref, err)
                checked_ref += 1
            if len(consts[4]) <= 32 or spec["hist"] == "H256":  # assertion 2
                theta = [mpf(float(v)) for v in clamped]
                smooth = finish(grad_partial(consts, theta, 1, T, quantize=False), counts, spec["tail"], P)
                for d in range(P):
                    if moved[d] or (d == 1 and theta[1] == 0):
                        continue

                    def f(v, d=d):
                        th = list(theta)
                        th[d] = v
                        return ll_only(spec, th, T)

                    num = mp.diff(f, theta[d])
                    err = abs(num - smooth[2][d]) / C[d] if C[d] != 0 else abs(num - smooth[2][d])
                    worst_diff = max(worst_diff, float(err))
                    assert err <= mpf(10) ** -25, "gradient off mpmath.diff: %s %r component %d: %s vs %s" % (
                        source, point, d, mp.nstr(smooth[2][d], 30), mp.nstr(num, 30))
                    checked_diff += 1
            kept += 1
            rec["points"].append([float(v) for v in point])
            rec["T"].append(T)
            rec["ll"].append(float(ll))
            rec["sp"].append(float(sp))
            rec["grad"].append([float(g) for g in grad])
            rec["C"].append([float(v) for v in C])
            rec["D"].append([float(v) for v in D])
        if rec["points"]:
            out_cases.append(rec)
    print("kept %d points, dropped %d candidates; %d values checked against the reference's (worst %.3g), %d components "
          "against mpmath.diff (worst %.3g relative to C_k); %.0f s" % (kept, dropped, checked_ref, worst_ref, checked_diff,
                                                                        worst_diff, time.time() - t0), flush=True)
    out = {"_made_by": "tests/golden/make_golden_gradient.py",
           "what": "log-likelihood, sp = sum p_j and the analytic gradient (of what the kernels evaluate, after "
                   "fit_to_bounds, threshold_o = T fixed) restated in mpmath at 50 digits, with the condition sums "
                   "C_k = sum |h dp/p| + |tail sum dp / (1 - sp)| and D_k = |sum dp| per component",
           "k_tail": K_TAIL, "kept": kept, "dropped": dropped, "cases": out_cases,
           "env": {"mpmath": mpmath.__version__, "dps": mp.dps}}
    path = os.path.join(HERE, "gradient.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
