#!/usr/bin/env python3
"""tests/golden/math_primitives.json: inputs, expected bits and 50-digit values for the device's scalar math
(covest_amd/csrc/fastmath.h, point_fetch.h, grad_common.h; evaluated through covest_math_probe).

    python tests/golden/make_golden_math.py

Data only.  A column of doubles is ONE string of 16 hex digits a value (the IEEE bit pattern: -0.0, inf and NaN survive,
and a packed column is a sixth shorter than a list).  `bits` columns hold what the bit-exact restatements of
tests/math_reference.py give; `ref` columns the 50-digit value (mpmath) rounded to a double, and `resid` the rest of it
as an integer count of ulp(ref) / 4096 -- an integer, not a double, because below the smallest normal the rest is finer
than any double.  Sections (the inputs are those the accuracy of each function can break at; seeded where random):

  exp             per scale sc in {0, 540}: x with x + sc ln 2 across [-760, 720]; the neighbours of the underflow to 0
                  (-745.13), of the smallest normal (-708.4) and of the overflow (709.78); x log2(e) within 2 ulp of
                  half-integers (rint's ties, |t| at its largest); +-0, -inf, NaN, +inf; +-1100, 5000, 1e6, 1e20, 1e300
  exp_neg_rn      0, 1e-300, 2^-60 .. 2^-7, 2 000 seeded mantissas at exponents -60 .. -7, 2^-6 and its neighbours, a few
                  arguments from 2^-6 on (want: exp_fast(-x)'s bits); want below 2^-6: the correctly rounded exp(-x)
  log             per table interval its lower edge, the double below the next edge and the centre; 1 and 0.5; seeded
                  mantissas at exponents -1022 .. 1023; subnormals (fast_log and fast_log_n only, listed last)
  log_trunc_norm  the piece boundaries of the normaliser and a geometric spread, with the derivatives
  rates, weights  every class of k in {1, 8, 21, 31, 63} x S in {8, 16} x e in {0, 1e-9, 0.03, 0.5, 1}; copy numbers
                  {1, 2, 3, 4, 17, 16384} x (q1, q2, q) in {0, 0.01, 0.5, 1}^3

What a rule re-creates is NOT stored (math_reference.compact / expand): the seeded and rule-made inputs, the `bits`
columns, exp_neg_rn's `want` (an exact rational series gives the same doubles as mpmath: asserted) and the S = 8 rates
(the first eight classes of the S = 16 rows); the log table is stored, so that a test needs no mpmath to restate a log.
Before anything is written the restatements are held to the 50-digit values within the bars of math_reference.py, and
expand(compact(everything)) must give everything back.
"""
import json
import math
import os
import random
import sys
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import math_reference as R  # noqa: E402

OUT = os.path.join(HERE, "math_primitives.json")
N_EXP = 400  # seeded arguments a scale (math_reference.seeded_exp)


def neighbours(x, n):
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def exp_inputs(sc, rng):
    m = R.mp()
    shift = float(sc * R.LN2)
    xs = R.seeded_exp(sc, N_EXP)
    for power in (-1075, -1074, -1022, 1024):  # 2^-1075: the tie between 0 and the smallest subnormal
        xs += neighbours(float(m.log(2) * power) - shift, 3)
    l2e = R._EXP_L2E
    halves = [0.5, -0.5, 1.5, -1.5, 100.5, -100.5, 1000.5, -1000.5, 1023.5, -1074.5]
    halves += [rng.getrandbits(11) - 1024 + 0.5 for _ in range(24)]
    for h in halves:
        xs += neighbours(h / l2e - (shift if rng.getrandbits(1) else 0.0), 2)
    xs += [0.0, -0.0, -math.inf, math.nan, math.inf]
    for mag in (1100.0, 5000.0, 1e6, 1e20, 1e300):
        xs += [mag, -mag]
    return xs


def exp_section(sc, rng):
    m = R.mp()
    xs = exp_inputs(sc, rng)
    got, ref, resid = [], [], []
    for x in xs:
        got.append(R.exp_scaled(x, sc))
        if x != x:
            r, d = math.nan, 0
        elif x == math.inf or x > 2000:
            r, d = math.inf, 0
        elif x == -math.inf or x < -2000:
            r, d = 0.0, 0
        else:
            r, d = R.split(R.mpf_fraction(m.exp(m.mpf(x))) * Fraction(2) ** sc)
        ref.append(r)
        resid.append(d)
    return {"x": R.pack(xs), "n_seeded": N_EXP, "bits": R.pack(got), "ref": R.pack(ref), "resid": resid}


def exp_neg_rn_section():
    m = R.mp()
    small = [0.0, 1e-300] + [2.0 ** -e for e in range(60, 6, -1)] + [math.nextafter(2.0 ** -6, 0.0)]
    n_fixed = len(small)
    small += R.seeded_exp_neg(2000)
    assert all(x < 2.0 ** -6 for x in small)
    large = [2.0 ** -6, math.nextafter(2.0 ** -6, 1.0), 0.02, 0.1, 1.0, 10.0, 199.5, 745.0, 800.0]
    want = [R.round_fraction(R.mpf_fraction(m.exp(-m.mpf(x)))) for x in small] + [R.exp_scaled(-x, 0) for x in large]
    return {"x": R.pack(small + large), "want": R.pack(want), "n_small": len(small), "n_fixed": n_fixed, "n_seeded": 2000}


LOG_NAMES = ["fast_log"] + list(R.LOG_VARIANTS)


def log_section():
    xs, n_normal = R.log_inputs()
    ref, resid = zip(*(R.split(R.mp_log_fraction(x)) for x in xs))
    bits = {name: R.pack(R.log_variant(name, x) for x in (xs if name == "fast_log" else xs[:n_normal]))
            for name in LOG_NAMES}
    return {"x": R.pack(xs), "n_normal": n_normal, "ref": R.pack(ref), "resid": list(resid), "bits": bits}


def log_trunc_norm_section():
    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, 0.0))
    xs = [1e-12, 1e-8, up(1e-8), dn(2.0 ** -10), 2.0 ** -10, up(2.0 ** -10), dn(1.0), 1.0, up(1.0), 199.9]
    for v in (200.0, 400.0, 11400.0):
        xs += [dn(v), v, up(v)]
    for n in (1, 2, 57):
        xs += [200.0 * n + 1e-9, 200.0 * n + 1e-8, 200.0 * n + 1e-7]
    xs += [400.00008, 200.5, 11400.03]  # (the last two: a residual in [2^-10, 1) behind a chunk)
    xs += [1e-9 * (2e4 / 1e-9) ** (i / 63.0) for i in range(64)]
    cols = {k: [] for k in ("piece", "y", "ref", "resid", "step", "d1", "d1_resid", "d2", "d2_resid")}
    for x in xs:
        piece, v, step = R.mp_log_trunc_norm(x)
        _, d1, d2 = R.mp_trunc_norm_dlog(x)
        cols["piece"].append(piece)
        cols["y"].append(R.round_fraction(R.mp_log_fraction(x)))
        for name, q in (("ref", v), ("d1", d1), ("d2", d2)):
            d, rest = R.split(q)
            cols[name].append(d)
            cols[name + "_resid" if name != "ref" else "resid"].append(rest)
        cols["step"].append(float(step))
    seen = set(cols["piece"])
    assert seen == {"by_x", "grid", "expm1", "log1p", "chunk_by_x", "chunk_grid", "chunk_expm1", "chunk_log1p"}, seen
    out = {"x": R.pack(xs)}
    for k, v in cols.items():
        out[k] = v if k == "piece" or k.endswith("resid") else R.pack(v)
    return out


RATE_K, RATE_R, RATE_C, RATE_E = (1, 8, 21, 31, 63), 100, 17.3, (0.0, 1e-9, 0.03, 0.5, 1.0)


def rates_section():
    groups = []
    for k in RATE_K:
        for S in (8, 16):
            c, e, s_list, ref, resid, got = [], [], [], [], [], []
            for err in RATE_E:
                lam = R.error_class_rates(k, RATE_R, RATE_C, err, S)
                for s in range(S):
                    assert R.same_bits(lam[s], R.error_class_rate_mul(k, RATE_R, RATE_C, err, s, S))
                    d, rest = R.split(R.mp_rate(k, RATE_R, RATE_C, err, s))
                    c.append(RATE_C), e.append(err), s_list.append(s), ref.append(d), resid.append(rest), got.append(lam[s])
            grp = {"k": k, "r": RATE_R, "S": S, "c": R.pack([RATE_C]), "e": R.pack(RATE_E), "ref": R.pack(ref),
                   "resid": resid, "bits": R.pack(got)}  # rows: for e, for s in 0 .. S - 1 (math_reference.rate_rows)
            assert R.rate_rows(grp) == list(zip(c, e, s_list))
            groups.append(grp)
    return groups


def weights_section():
    q1, q2, q, o, ref, resid, got = [], [], [], [], [], [], []
    vals = (0.0, 0.01, 0.5, 1.0)
    for a in vals:
        for b in vals:
            for c in vals:
                for copies in (1, 2, 3, 4, 17, 16384):  # o_values below
                    d, rest = R.split(R.mp_weight(a, b, c, copies))
                    q1.append(a), q2.append(b), q.append(c), o.append(copies), ref.append(d), resid.append(rest)
                    got.append(R.copy_number_weight_by_squaring(a, b, c, copies))
    sec = {"q_values": R.pack(vals), "o_values": [1, 2, 3, 4, 17, 16384], "ref": R.pack(ref), "resid": resid,
           "bits": R.pack(got)}  # rows: for q1, for q2, for q, for o (math_reference.weight_rows)
    assert R.weight_rows(sec) == list(zip(q1, q2, q, o))
    return sec


def build():
    m = R.mp()
    with m.workdps(70):
        assert abs(R.mpf_fraction(m.log(2)) - R.LN2) < Fraction(1, 10 ** 59)
        for s in range(64):  # the host's pow gives the correctly rounded 3^-s: the rates' references hang on it
            assert R.pow3neg(s) == R.round_fraction(Fraction(1, 3 ** s)), s
    R._TABLE = None  # the table by its rule, whatever a fixture installed before
    rng = random.Random(R.SEED)  # (the half-integers of the exponential's inputs; stored)
    table = [v for row in R.log_table() for v in row]
    doc = {"what": "inputs, bit-exact expectations and 50-digit values of the device's scalar math; "
                   "tests/golden/make_golden_math.py",
           "env": {"mpmath": m.__version__, "dps": m.mp.dps, "seed": R.SEED}, "log_table": R.pack(table), "ln2": R.LN2_TEXT, "resid_unit": R.RESID_UNIT,
           "exp": {str(sc): exp_section(sc, rng) for sc in (0, R.SCALE_BITS)},
           "exp_neg_rn": exp_neg_rn_section(), "log": log_section(),
           "log_trunc_norm": log_trunc_norm_section(), "rates": rates_section(), "weights": weights_section()}
    return doc


def dumps(doc):
    return json.dumps(doc, separators=(",", ":"), sort_keys=True).replace('],"', '],\n"').replace('","', '",\n"') + "\n"


def build_compact():
    """(the fixture as committed, the same with every row in place)."""
    doc = build()
    small = R.compact(doc)
    for sec in doc["exp"].values():
        del sec["n_seeded"]
    del doc["exp_neg_rn"]["n_fixed"], doc["exp_neg_rn"]["n_seeded"]
    # the rules re-create every input and every restated bit, and the exact series the 50-digit exp(-x) rounded
    assert R.expand(small) == doc
    return small, doc


def main():
    small, doc = build_compact()
    for line in R.check_restatements(doc):  # what tests/test_math_reference_cpu.py runs again
        print(line)
    text = dumps(small)
    assert len(text) <= 323569, len(text)  # no larger than the largest fixture before this one
    with open(OUT, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (os.path.basename(OUT), len(text)))


if __name__ == "__main__":
    main()
