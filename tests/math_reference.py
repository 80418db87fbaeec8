"""The references the device's scalar math is held to (tests/test_math_reference_cpu.py, tests/test_gpu_math.py).

(a) Bit-exact restatements of the primitives of covest_amd/csrc/fastmath.h whose every operation is explicit -- an fma,
    an asm v_fma / v_mul / v_add, rint, ldexp, or a lone multiply or add that feeds or follows an fma -- so that IEEE 754
    fixes the result whatever the surrounding code is: exp_scaled / exp_fast and the fast_log family.  Every fused
    operation here is an EXACT a * b + c in rational arithmetic, rounded once (fma below); a lone multiply or add is
    Python's float operation, which is the same single rounding.  The table is made by the rule of
    tools/gen_log_table.py, restated in log_table(); it is not read from log_table.h.
    The helpers of point_fetch.h that only multiply (error_class_rate_mul, error_class_rates<S>,
    copy_number_weight_by_squaring) are restated in float arithmetic: a product has nothing to contract.
(b) 50-digit values (mpmath): exp, the correctly rounded exp(-x), log, the reference's truncated-Poisson normaliser as
    the comment of log_trunc_norm gives it, its derivatives piece by piece, the rates and the weights.
(c) The bars of the accuracy checks, derived in the docstrings below, and the fixture's coding (packed hex doubles, and
    residuals in 1/4096 of the rounded value's ulp).  The committed fixture is COMPACT: what a rule re-creates is not
    stored -- seeded and rule-made inputs (seeded_exp, seeded_exp_neg, log_inputs), the restatements' bits, the exact
    exp(-x) -- and expand() puts it back, so that the tests see every row.

Nothing here needs a GPU, and only section (b) needs mpmath: the GPU tests read section (b)'s numbers from
tests/golden/math_primitives.json and compare in exact rational arithmetic.
"""
import copy
import math
import random
import struct
from fractions import Fraction

INF = math.inf
LN2_DOUBLE = 0.693147180559945309417232121458  # the literal of fastmath.h: the double nearest ln 2
# ln 2 to 60 digits, as a rational: the test side's own constant (mpmath.log(2) at 60 digits; checked by the generator)
LN2_TEXT = "0.693147180559945309417232121458176568075500134360255254120680"
LN2 = Fraction(LN2_TEXT)
LN2_ERR = abs(Fraction(LN2_DOUBLE) - LN2)  # |fl(ln 2) - ln 2|, about 2.3e-17
SCALE_BITS = 540   # tiles.h kScaleBits
BASIC_SHIFT = 64   # tiles.h kBasicShift
RESID_UNIT = 4096  # a residual is an integer count of ulp(value) / 4096


# ---- bits, exact arithmetic -----------------------------------------------------------------------------------------

def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def hexbits(x):
    return "%016x" % bits(x)


def pack(values):
    """Doubles as one string of 16 hex digits each (the IEEE bit pattern, so -0.0, inf and NaN survive)."""
    return "".join(hexbits(v) for v in values)


def unpack(text):
    assert len(text) % 16 == 0
    return [from_bits(int(text[i:i + 16], 16)) for i in range(0, len(text), 16)]


def same_bits(a, b):
    """Bit equality; any NaN equals any NaN (the payload is not part of any claim)."""
    return (a != a and b != b) or bits(a) == bits(b)


def round_fraction(q, negative_zero=False):
    """The double nearest the rational q, ties to even, subnormals included (int / int is correctly rounded)."""
    if q == 0:
        return -0.0 if negative_zero else 0.0
    try:
        return q.numerator / q.denominator
    except OverflowError:
        return INF if q > 0 else -INF


def fma(a, b, c):
    """a * b + c rounded once, by IEEE 754's rules for the specials and the sign of an exact zero."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        if math.isfinite(a) and math.isfinite(b):
            return c  # finite product: +-inf or NaN as c is (a * b may not overflow on its way)
        return a * b + c
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        prod_neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        if Fraction(a) * Fraction(b) == 0 and c == 0:
            return -0.0 if (prod_neg and math.copysign(1.0, c) < 0) else 0.0
        return 0.0  # x + (-x) is +0 in round-to-nearest
    return round_fraction(q)


def ldexp_exact(p, n):
    """p 2^n as v_ldexp_f64 rounds it: once, to nearest even, onto the subnormal grid where the result lies there."""
    if p != p or math.isinf(p) or p == 0.0:
        return p
    return round_fraction(Fraction(p) * Fraction(2) ** n, negative_zero=p < 0)


def rint(v):
    if v != v or math.isinf(v) or abs(v) >= 2.0 ** 52:
        return v
    r = float(round(v))  # Python rounds halves to even, as v_rndne_f64
    return math.copysign(r, v)


def ulp_of(v):
    """The spacing of the doubles at |v| (2^-1074 at and below the smallest normal)."""
    return Fraction(math.ulp(abs(v))) if math.isfinite(v) else Fraction(0)


# ---- (a) exp_scaled -------------------------------------------------------------------------------------------------

_EXP_L2E = float.fromhex("0x1.71547652b82fep+0")
_EXP_LN2_HI = float.fromhex("0x1.62e42fefa39efp-1")
_EXP_LN2_LO = float.fromhex("0x1.abc9e3b39803fp-56")
_EXP_C11 = float.fromhex("0x1.ade156a5dcb37p-26")
_EXP_C10 = float.fromhex("0x1.28af3fca7ab0cp-22")
_EXP_COEF = [float.fromhex(h) for h in (
    "0x1.71dee623fde64p-19", "0x1.a01997c89e6b0p-16", "0x1.a01a014761f6ep-13", "0x1.6c16c1852b7b0p-10",
    "0x1.1111111122322p-7", "0x1.55555555502a1p-5", "0x1.5555555555511p-3", "0x1.000000000000bp-1")]


def exp_reduce(x):
    """(dn, t) of exp_scaled: x = dn ln 2 + t by Cody-Waite."""
    dn = rint(x * _EXP_L2E)
    t = fma(-dn, _EXP_LN2_HI, x)
    t = fma(-dn, _EXP_LN2_LO, t)
    return dn, t


def exp_scaled(x, sc=0):
    dn, t = exp_reduce(x)
    p = t * _EXP_C11      # v_mul_f64
    p = p + _EXP_C10      # v_add_f64
    for c in _EXP_COEF:
        p = fma(t, p, c)
    p = fma(t, p, 1.0)
    p = fma(t, p, 1.0)
    if dn != dn:
        n = -4096  # fmax(NaN, -4096) is -4096
    else:
        n = int(min(max(dn, -4096.0), 4096.0))
    z = ldexp_exact(p, n + sc)
    return 0.0 if x == -INF else z


# ---- (a) the fast_log family ----------------------------------------------------------------------------------------

_TABLE = None


def log_table():
    """[(1/c, log c')] for the 256 intervals of the mantissa in [0.5, 1): the rule of tools/gen_log_table.py 256."""
    global _TABLE
    if _TABLE is None:
        import mpmath
        n = 256
        rows = []
        with mpmath.workdps(60):
            for i in range(n):
                c = Fraction(1, 2) + Fraction(2 * i + 1, 4 * n)
                invc = float(1 / c)
                cp = 1 / Fraction(invc)
                rows.append((invc, float(mpmath.log(mpmath.mpf(cp.numerator) / mpmath.mpf(cp.denominator)))))
        _TABLE = rows
    return _TABLE


def use_log_table(rows):
    """The table as the fixture carries it (the GPU tests need no mpmath); the CPU tests hold it to the rule above."""
    global _TABLE
    _TABLE = [tuple(r) for r in rows]


_LOG_D3 = -(0.5 + 0.20710678118654752 * 2.0 ** -18)


def _log_core(m, e, deg):
    """fma(e, ln 2, log c') + log1p(r) with log1p to r^deg, as fast_log / fast_log_bits_n form it."""
    invc, logc = log_table()[(bits(m) >> 44) & 0xFF]
    r = fma(m, invc, -1.0)
    if deg == 5:
        q = fma(r, 0.2, -0.25)
        q = fma(r, q, 1.0 / 3.0)
        q = fma(r, q, -0.5)
    elif deg == 4:
        q = fma(r, -0.25, 1.0 / 3.0)
        q = fma(r, q, -0.5)
    else:
        q = fma(r, 1.0 / 3.0, _LOG_D3)
    lp = fma(r * r, q, r)
    return fma(float(e), LN2_DOUBLE, logc) + lp


def fast_log(x):
    """fast_log and fast_log_n: v_frexp_mant / v_frexp_exp split (subnormals included; 0 gives mantissa 0, exponent 0)."""
    m, e = math.frexp(x)
    return _log_core(m, e, 5)


def raw_exponent(x):
    return bits(x) >> 52  # hi >> 20 of a positive double


def log_bias(sc):
    """kLogRawBias<SC>: (double)(1022 + SC) * fl(ln 2), one rounding."""
    return float(1022 + sc) * LN2_DOUBLE


def log_bias_error(sc):
    """(|kLogRawBias<SC> - (1022 + SC) ln 2|, its bound): half an ulp of the product and the constant's error
    (1022 + SC) times -- 6.97e-14 against 1.50e-13 at SC = 540, per log, the same for every key of a sum."""
    b = log_bias(sc)
    return abs(Fraction(b) - (1022 + sc) * LN2), ulp_of(b) / 2 + (1022 + sc) * LN2_ERR


def fast_log_bits(x, deg, sc, raw=False):
    """fast_log_bits_n<N, deg, sc, raw> of a positive NORMAL double: log(x 2^-sc) (+ log_bias(sc) if raw)."""
    assert x > 0 and raw_exponent(x) not in (0, 2047)
    m, _ = math.frexp(x)
    e = raw_exponent(x) if raw else raw_exponent(x) - (1022 + sc)
    return _log_core(m, e, deg)


LOG_VARIANTS = {  # name in covest_amd._capi.MATH_PROBE_FN: (deg, sc, raw); fast_log and fast_log_n4: frexp's exponent
    "log_bits_1_5_basic": (5, BASIC_SHIFT, False),
    "log_bits_4_5_scale": (5, SCALE_BITS, False),
    "log_bits_4_3_scale_raw": (3, SCALE_BITS, True),
    "log_bits_4_4_scale": (4, SCALE_BITS, False),
}


def log_variant(name, x):
    if name in ("fast_log", "fast_log_n4"):
        return fast_log(x)
    deg, sc, raw = LOG_VARIANTS[name]
    return fast_log_bits(x, deg, sc, raw)


# ---- (c) the logs' bar ----------------------------------------------------------------------------------------------

T5 = Fraction(1, 6) * Fraction(2) ** -54
T4 = Fraction(1, 5) * Fraction(2) ** -45 + T5
T3 = (Fraction(1, 4) - Fraction("0.20710678118654752")) * Fraction(2) ** -36 + Fraction(1, 5) * Fraction(2) ** -45 + T5
LOG_T = {5: T5, 4: T4, 3: T3}


def log_want_and_bar(name, x, log_x):
    """(want, bar, exponent) of a log variant at x, log_x the exact (rational) log x.

    want = log x - SC ln 2 (+ the RAW bias).  bar = T_DEG + 2^-52 |want| + |fl(ln 2) - ln 2| |e| + 2^-53:
      T_DEG       the truncation of log1p(r), |r| <= 2^-9: r^6 / 6 (T5), plus r^5 / 5 at degree 4, plus the
                  equioscillating (1/4 - d) r^4 with d = 0.2071... at degree 3 (about 6.30e-13 in all)
      2^-52|want| the two roundings at the result's magnitude (the fma of the exponent, the final add)
      |e| term    the constant fl(ln 2)'s own error, once per unit of the exponent e that multiplies it
      2^-53       the table entry's rounding (|log c'| < 1).
    RAW: the bias in `want` is the REAL (1022 + SC) ln 2 -- what the un-biased exponent e multiplies, so that the |e|
    term is the whole of the constant's part.  The double kLogRawBias<SC> that a caller takes off again is off that real
    number by its own rounding and by (1022 + SC) |fl(ln 2) - ln 2|: log_bias_error() below, held to its own bound."""
    if name in ("fast_log", "fast_log_n4"):
        deg, e, want = 5, math.frexp(x)[1], log_x
    else:
        deg, sc, raw = LOG_VARIANTS[name]
        e = raw_exponent(x) if raw else raw_exponent(x) - (1022 + sc)
        want = log_x - sc * LN2 + ((1022 + sc) * LN2 if raw else 0)
    bar = LOG_T[deg] + Fraction(2) ** -52 * abs(want) + LN2_ERR * abs(e) + Fraction(2) ** -53
    return want, bar, e


def exact_value(ref, resid):
    """The 50-digit value a fixture row holds: its rounding to a double and the rest in ulp(ref) / 4096."""
    return Fraction(ref) + Fraction(resid, RESID_UNIT) * ulp_of(ref)


def error_in_ulps(got, exact):
    """|got - exact| in units of the spacing of the doubles at |exact| (2^-1074 where exact is subnormal or 0)."""
    if exact == 0:
        unit = Fraction(2) ** -1074
    else:
        e = exact.numerator.bit_length() - exact.denominator.bit_length()  # 2^(e-1) <= |exact| < 2^(e+1)
        if abs(exact) < Fraction(2) ** e:
            e -= 1
        unit = Fraction(2) ** max(e - 52, -1074)
    return abs(Fraction(got) - exact) / unit


# ---- restatements in float arithmetic: products only (point_fetch.h) ---------------------------------------------------

def pow3neg(s):
    return 3.0 ** -s  # libm pow on the host, as covest_model_create forms DevModel::pow3neg


def error_class_rates(k, r, c, err, S):
    ck = c * float(r - k + 1) / float(r)
    q = 1.0 - err
    n = max(k - (S - 1), 0)
    pw, sq = 1.0, q
    while n > 0:
        if n & 1:
            pw *= sq
        sq *= sq
        n >>= 1
    qp = [0.0] * S
    for s in range(S - 1, -1, -1):
        qp[s] = pw
        if k - s >= 0:
            pw *= q
    lam, pe = [], 1.0
    for s in range(S):
        lam.append(((ck * pow3neg(s)) * qp[s]) * pe)
        pe *= err
    return lam


def error_class_rate_mul(k, r, c, err, s, S):
    ck = c * float(r - k + 1) / float(r)
    q = 1.0 - err
    n = max(k - (S - 1), 0)
    pw, sq = 1.0, q
    while n > 0:
        if n & 1:
            pw *= sq
        sq *= sq
        n >>= 1
    for t in range(S - 1, s, -1):
        if k - t >= 0:
            pw *= q
    pe = 1.0
    for _ in range(s):
        pe *= err
    return ((ck * pow3neg(s)) * pw) * pe


def copy_number_weight_by_squaring(q1, q2, q, o):
    if o == 1:
        return q1
    if o == 2:
        return (1.0 - q1) * q2
    ph, pl, sh, sl, n = 1.0, 0.0, 1.0 - q, 0.0, o - 3
    while n:  # (hi, lo) pairs, every operation as point_fetch.h writes it
        if n & 1:
            h = ph * sh
            lo = fma(ph, sh, -h) + fma(ph, sl, pl * sh)
            s = h + lo
            ph, pl = s, lo - (s - h)
        h = sh * sh
        lo = fma(sh, sh, -h) + (sh + sh) * sl
        s = h + lo
        sh, sl = s, lo - (s - h)
        n >>= 1
    return (1.0 - q1) * (1.0 - q2) * q * ph


def copy_number_weight_plain_squaring(q1, q2, q, o):
    """The same with the squares and the product in plain doubles: what point_fetch.h did before the pairs, kept to
    show what they are for -- every squaring doubles the relative error it inherits, about (o - 3) 2^-53 in all."""
    if o < 3:
        return copy_number_weight_by_squaring(q1, q2, q, o)
    pw, sq, n = 1.0, 1.0 - q, o - 3
    while n:
        if n & 1:
            pw = pw * sq
        sq *= sq
        n >>= 1
    return (1.0 - q1) * (1.0 - q2) * q * pw


def exp_neg_rn_uncontracted(x):
    """exp_neg_rn's small-argument branch (x < 2^-6) with every operation rounded on its own: what the source says if
    the compiler contracts nothing.  NOT a bit-exact claim about the device (the polynomial is plain C++ and may be
    contracted); the claim tested on the device is the function's own -- the correctly rounded exp(-x)."""
    p = x * x
    pe = fma(x, x, -p)
    tail = (p * x) * (-1.0 / 6 + x * (1.0 / 24 + x * (-1.0 / 120 + x * (1.0 / 720 + x * (
        -1.0 / 5040 + x * (1.0 / 40320 + x * (-1.0 / 362880)))))))
    mx, hp = -x, 0.5 * p
    s = mx + hp
    bb = s - mx
    e = (mx - (s - bb)) + (hp - bb)
    lo = e + (0.5 * pe + tail)
    r = 1.0 + s
    bb = r - 1.0
    e2 = (1.0 - (r - bb)) + (s - bb)
    return r + (e2 + lo)


def exp_neg_correctly_rounded(x):
    """The double nearest exp(-x) for 0 <= x < 1, in exact rational arithmetic: the partial sums of the alternating series
    bracket the value (its terms fall), so once two consecutive sums round to the same double that double is it."""
    q, term, s, k = Fraction(x), Fraction(1), Fraction(1), 0
    while True:
        k += 1
        term = term * -q / k
        if k >= 2 and round_fraction(s) == round_fraction(s + term):
            return round_fraction(s)
        s += term


# ---- inputs made by a rule: not stored in the fixture ---------------------------------------------------------------------

SEED = 20240611


def _mantissa(rng):
    """A seeded double in [0.5, 1)."""
    return from_bits((1022 << 52) | rng.getrandbits(52))


def seeded_exp(sc, n):
    """n arguments with x + sc ln 2 spread over [-760, 720]."""
    rng, shift = random.Random(SEED + 1 + sc), float(sc * LN2)
    return [-760.0 + 1480.0 * rng.random() - shift for _ in range(n)]


def seeded_exp_neg(n):
    """n seeded mantissas at exponents -60 .. -7."""
    rng = random.Random(SEED + 2)
    return [math.ldexp(_mantissa(rng), -59 + rng.getrandbits(16) % 54) for _ in range(n)]


def log_inputs():
    """(xs, n_normal): per table interval its lower edge, the double below the next edge and the centre, at exponent 0;
    1 and 0.5; 200 seeded mantissas at frexp exponents -1021 .. 0 and 100 at 1 .. 1024; the largest and the smallest
    normal double; then, for fast_log and fast_log_n only, subnormals (the extremes, 30 seeded, padding to four)."""
    rng = random.Random(SEED + 3)
    xs = []
    for i in range(256):
        xs += [0.5 + i / 512.0, math.nextafter(0.5 + (i + 1) / 512.0, 0.0), 0.5 + (2 * i + 1) / 1024.0]
    xs += [1.0, 0.5]
    xs += [math.ldexp(_mantissa(rng), -1021 + rng.getrandbits(16) % 1022) for _ in range(200)]
    xs += [math.ldexp(_mantissa(rng), 1 + rng.getrandbits(16) % 1024) for _ in range(100)]
    xs += [math.nextafter(math.inf, 0.0), 2.2250738585072014e-308]
    n_normal = len(xs)
    xs += [5e-324, math.nextafter(2.2250738585072014e-308, 0.0)]
    xs += [from_bits(rng.getrandbits(52) >> (rng.getrandbits(16) % 52)) or 5e-324 for _ in range(30)]
    while (len(xs) - n_normal) % 4:
        xs.append(5e-324)
    assert n_normal % 4 == 0 and all(raw_exponent(x) not in (0, 2047) for x in xs[:n_normal])
    return xs, n_normal


def compact(doc):
    """The fixture as it is committed: without what expand() re-creates."""
    out = copy.deepcopy(doc)
    for sc_text, sec in out["exp"].items():
        n = sec.pop("n_seeded")
        assert unpack(sec["x"])[:n] == seeded_exp(int(sc_text), n)
        sec["x"], sec["seeded"] = sec["x"][16 * n:], n
        del sec["bits"]
    sec = out["exp_neg_rn"]
    xs, fixed, n = unpack(sec["x"]), sec.pop("n_fixed"), sec.pop("n_seeded")
    assert xs[fixed:fixed + n] == seeded_exp_neg(n) and sec["n_small"] == fixed + n
    out["exp_neg_rn"] = {"x_small": pack(xs[:fixed]), "seeded": n, "x_large": pack(xs[fixed + n:])}
    sec = out["log"]
    assert (unpack(sec["x"]), sec["n_normal"]) == log_inputs()
    for key in ("x", "n_normal", "bits"):
        del sec[key]
    out["rates"] = [dict(grp) for grp in out["rates"] if grp["S"] == 16]
    for grp in out["rates"]:
        del grp["bits"], grp["S"]
    del out["weights"]["bits"]
    return out


def expand(doc):
    """The fixture with every row in place: inputs made by their rules, the restatements' bits, the correctly rounded
    exp(-x); the rates of S = 8 are the first eight classes of the S = 16 rows (the value does not depend on S)."""
    out = copy.deepcopy(doc)
    use_log_table(zip(*[iter(unpack(out["log_table"]))] * 2))
    for sc_text, sec in out["exp"].items():
        xs = seeded_exp(int(sc_text), sec.pop("seeded")) + unpack(sec["x"])
        sec["x"], sec["bits"] = pack(xs), pack(exp_scaled(x, int(sc_text)) for x in xs)
    sec = out["exp_neg_rn"]
    small = unpack(sec["x_small"]) + seeded_exp_neg(sec["seeded"])
    large = unpack(sec["x_large"])
    want = [exp_neg_correctly_rounded(x) for x in small] + [exp_scaled(-x, 0) for x in large]
    out["exp_neg_rn"] = {"x": pack(small + large), "want": pack(want), "n_small": len(small)}
    sec = out["log"]
    xs, n_normal = log_inputs()
    sec["x"], sec["n_normal"] = pack(xs), n_normal
    sec["bits"] = {name: pack(log_variant(name, x) for x in (xs if name == "fast_log" else xs[:n_normal]))
                   for name in ["fast_log"] + list(LOG_VARIANTS)}
    groups = []
    for grp in out["rates"]:
        ref, resid = unpack(grp["ref"]), grp["resid"]
        for S in (8, 16):
            keep = [i for i in range(len(ref)) if i % 16 < S]
            g = dict(grp, S=S, ref=pack(ref[i] for i in keep), resid=[resid[i] for i in keep])
            g["bits"] = pack(error_class_rate_mul(g["k"], g["r"], c, e, s, S) for c, e, s in rate_rows(g))
            groups.append(g)
    out["rates"] = groups
    sec = out["weights"]
    sec["bits"] = pack(copy_number_weight_by_squaring(*row) for row in weight_rows(sec))
    return out


# ---- (c) bars of the rates and weights ------------------------------------------------------------------------------

def rate_mul_bar(k, S):
    """Relative: (2 ceil(log2 k) + S + 4) 2^-53 -- the squarings and multiplies of (1 - e)^n_low, one multiply a class
    above it and one a power of e (S in all), and the four roundings of ck and the three products."""
    return Fraction(2 * math.ceil(math.log2(k)) + S + 4) * Fraction(2) ** -53


WEIGHT_SQ_BAR = Fraction(2 * 14 + 4) * Fraction(2) ** -53  # 14 squarings and as many multiplies, four more products
# The device library documents pow to 1 ulp (2^-52 relative); held here to twice that a call, plus the roundings around:
RATE_POW_BAR = Fraction(2 * 4 + 5) * Fraction(2) ** -53    # two pows; ck's two roundings and three products
WEIGHT_POW_BAR = Fraction(4 + 5) * Fraction(2) ** -53      # one pow; 1 - q1, 1 - q2 and three products


# ---- (b) 50-digit values --------------------------------------------------------------------------------------------

def mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def mpf_fraction(v):
    sign, man, exp, _ = v._mpf_
    q = Fraction(int(man)) * Fraction(2) ** int(exp)
    return -q if sign else q


def split(q):
    """(double nearest q, residual in 1/4096 ulp of it, rounded to an integer)."""
    d = round_fraction(q)
    if math.isinf(d):
        return d, 0
    u = ulp_of(d)
    return d, int(round((q - Fraction(d)) / u * RESID_UNIT))


def mp_exp_fraction(x, sc=0):
    m = mp()
    return mpf_fraction(m.exp(m.mpf(x))) * Fraction(2) ** sc


def mp_log_fraction(x):
    m = mp()
    return mpf_fraction(m.log(m.mpf(x)))


def trunc_norm_piece(x):
    """(piece, n, xr) of log_trunc_norm's definition: 200 is taken off x while it exceeds 200 (exactly: every partial
    difference is a multiple of ulp(x) below x), so xr in (0, 200] and n the number of chunks.
      by_x    x <= 1e-8: the normaliser is x itself                      -> log x
      chunk_by_x  a residual <= 1e-8: it is the ORIGINAL x               -> 200 n + log x
      grid    xr < 2^-10: e^xr rounded to the 2^-63 grid before the - 1  -> 200 n + log(grid(e^xr) - 1)
      expm1   2^-10 <= xr < 1                                           -> 200 n + log(e^xr - 1)
      log1p   xr >= 1                                                   -> 200 n + xr + log(1 - e^-xr)
    with the prefix chunk_ where n > 0."""
    if x <= 1e-8:
        return "by_x", 0, x
    q = Fraction(x)
    n = 0
    if q > 200:
        n = math.ceil(q / 200) - 1
    xr = q - 200 * n
    assert 0 < xr <= 200
    xr_d = float(xr)
    assert Fraction(xr_d) == xr, x
    pre = "chunk_" if n else ""
    if xr_d <= 1e-8:
        return "chunk_by_x", n, xr_d
    if xr_d < 2.0 ** -10:
        return pre + "grid", n, xr_d
    if xr_d < 1.0:
        return pre + "expm1", n, xr_d
    return pre + "log1p", n, xr_d


def mp_log_trunc_norm(x):
    """(piece, value as a rational, grid step) -- the grid step 2^-63 / expm1(xr) where the piece rounds onto the grid
    (the rounding may fall either way on the device: its expm1 is rounded to a double first), else 0."""
    m = mp()
    piece, n, xr = trunc_norm_piece(x)
    step = Fraction(0)
    if piece.endswith("by_x"):
        v = m.log(m.mpf(x))
    elif piece.endswith("grid"):
        e = mpf_fraction(m.exp(m.mpf(xr)))
        g = Fraction(round(e * 2 ** 63), 2 ** 63)  # the 64-bit significand of a long double in [1, 2)
        d = g - 1
        v = m.log(m.mpf(d.numerator) / m.mpf(d.denominator))
        step = Fraction(2) ** -63 / mpf_fraction(m.expm1(m.mpf(xr)))
    else:
        v = m.log(m.expm1(m.mpf(xr)))
    return piece, 200 * n + mpf_fraction(v), step


def mp_trunc_norm_dlog(x):
    """(piece, L', L'') inside the piece: 1 / x and -1 / x^2 on the two branches that divide by x itself,
    1 / (1 - e^-xr) and -e^-xr / (1 - e^-xr)^2 otherwise."""
    m = mp()
    piece, _, xr = trunc_norm_piece(x)
    if piece.endswith("by_x"):
        d1 = 1 / m.mpf(x)
        d2 = -d1 * d1
    else:
        em = m.exp(-m.mpf(xr))
        d1 = 1 / (1 - em)
        d2 = -em * d1 * d1
    return piece, mpf_fraction(d1), mpf_fraction(d2)


def mp_rate(k, r, c, err, s, literal_exponent=False):
    """ck 3^-s q^max(k - s, 0) e^s with q the DOUBLE fl(1 - e) and 3^-s the double pow3neg(s): what is left to the
    device is multiplications, and the bar counts those.  ck = c (r - k + 1) / r exactly.  literal_exponent: q^(k - s)
    as error_class_rate's pow takes it (the same for s <= k)."""
    q = Fraction(1.0 - err)
    n = k - s if literal_exponent else max(k - s, 0)
    return Fraction(c) * (r - k + 1) / r * Fraction(pow3neg(s)) * q ** n * Fraction(err) ** s


def mp_weight(q1, q2, q, o):
    if o == 1:
        return Fraction(q1)
    if o == 2:
        return Fraction(1.0 - q1) * Fraction(q2)
    return Fraction(1.0 - q1) * Fraction(1.0 - q2) * Fraction(q) * Fraction(1.0 - q) ** (o - 3)


# ---- (c) the checks, shared by the CPU tests (on the restatements) and the GPU tests (on the device's outputs) --------

# exp_scaled is asserted up to this |x|; beyond it the remainder t = x - dn ln 2 is no longer small (fastmath.h)
EXP_REACH = 1e15


def exp_worst_ulps(sec, got, scale_back=0):
    """(worst error in ulps, its x) of `got` against the section's 50-digit values, over the rows with a finite x of
    magnitude <= EXP_REACH.  A row whose value is beyond the doubles counts only if got is not +inf (then: inf).
    scale_back = sc: `got` is exp(x) itself, the section's values are exp(x) 2^sc -- rows whose scaled value is not a
    finite normal double are left out (their rest is too coarse to take the scale off)."""
    worst, at = Fraction(0), None
    for x, g, ref, resid in zip(unpack(sec["x"]), got, unpack(sec["ref"]), sec["resid"]):
        if not math.isfinite(x) or abs(x) > EXP_REACH:
            continue
        if math.isinf(ref):
            if scale_back:
                continue
            err = Fraction(0) if g == INF else None
        else:
            exact = exact_value(ref, resid)
            if scale_back:
                if abs(ref) < 2.2250738585072014e-308:
                    continue
                exact = exact / Fraction(2) ** scale_back
            err = error_in_ulps(g, exact) if math.isfinite(g) else None
        if err is None:
            return INF, x
        if err > worst:
            worst, at = err, x
    return float(worst), at


def log_check(sec, name, got):
    """(worst |got - want|, worst |got - want| / bar, x of the latter) of a log variant over its rows."""
    xs = unpack(sec["x"])
    if name not in ("fast_log", "fast_log_n4"):
        xs = xs[:sec["n_normal"]]
    assert len(got) == len(xs)
    worst, ratio, at = Fraction(0), Fraction(0), None
    for x, g, ref, resid in zip(xs, got, unpack(sec["ref"]), sec["resid"]):
        want, bar, _ = log_want_and_bar(name, x, exact_value(ref, resid))
        if not math.isfinite(g):
            return INF, INF, x
        err = abs(Fraction(g) - want)
        worst = max(worst, err)
        if err / bar > ratio:
            ratio, at = err / bar, x
    return float(worst), float(ratio), at


def fast_log_bar_at(m):
    """The logs' bar for fast_log at the (device-formed) argument m: what the table form of log_trunc_norm substitutes."""
    return log_want_and_bar("fast_log", m, Fraction(math.log(m)))[1]


def trunc_norm_plain_bar(value):
    """A priori, for log_trunc_norm WITHOUT the table: the device library documents log, log1p and expm1 to 1 ulp.  An
    argument off by 2^-52 relative moves its log by 2^-52; the log's own ulp and the two additions (xr +, base +) are
    at most 3 x 2^-53 of the larger of the value and 1 -- 2^-51 max(1, |value|) covers them."""
    return Fraction(2) ** -51 * max(Fraction(1), abs(value))


def trunc_norm_errors(sec, got):
    """[(piece, x, |got - value|, value, grid step, argument of the substituted log or None)] a row."""
    out = []
    cols = zip(unpack(sec["x"]), sec["piece"], got, unpack(sec["ref"]), sec["resid"], unpack(sec["step"]))
    for x, piece, g, ref, resid, step in cols:
        value = exact_value(ref, resid)
        err = abs(Fraction(g) - value) if math.isfinite(g) else INF
        _, _, xr = trunc_norm_piece(x)
        arg = None
        if piece.endswith(("grid", "expm1")):
            arg = math.expm1(xr)
        elif piece.endswith("log1p"):
            arg = 1.0 - math.exp(-xr)
        out.append((piece, x, err, value, Fraction(step), arg))
    return out


def worst_by_piece(rows, measure):
    worst = {}
    for row in rows:
        worst[row[0]] = max(worst.get(row[0], 0.0), float(measure(row)))
    return worst


def relative_errors(got, ref, resid):
    """|got / value - 1| a row; a value of exactly 0 wants exactly 0 (else inf)."""
    out = []
    for g, d, rest in zip(got, ref, resid):
        value = exact_value(d, rest)
        if not math.isfinite(g):
            out.append(INF)
        elif value == 0:
            out.append(0.0 if g == 0.0 else INF)
        else:
            out.append(abs(Fraction(g) / value - 1))
    return out


def rate_rows(grp):
    """[(c, e, s)] of a rates group: for every e, every class."""
    c = unpack(grp["c"])[0]
    return [(c, e, s) for e in unpack(grp["e"]) for s in range(grp["S"])]


def weight_rows(sec):
    """[(q1, q2, q, o)] of the weights section: the product of the q values three times over, and the copy numbers."""
    qs = unpack(sec["q_values"])
    return [(a, b, c, o) for a in qs for b in qs for c in qs for o in sec["o_values"]]


def check_restatements(doc):
    """The restatements alone, on the whole fixture: every `bits` column reproduced, and inside every bar against the
    50-digit values.  Returns the lines of a report; raises AssertionError."""
    lines = []
    for sc_text, sec in sorted(doc["exp"].items()):
        sc = int(sc_text)
        got = [exp_scaled(x, sc) for x in unpack(sec["x"])]
        assert all(same_bits(a, b) for a, b in zip(got, unpack(sec["bits"])))
        worst, at = exp_worst_ulps(sec, got)
        lines.append("exp_scaled(x, %d): worst %.4f ulp at x = %r (%d rows)" % (sc, worst, at, len(got)))
        assert worst <= 1.0, (sc, worst, at)  # the device library documents its exp to 1 ulp; the GPU test measures it
    sec = doc["exp_neg_rn"]
    xs, want = unpack(sec["x"]), unpack(sec["want"])
    n_small = sec["n_small"]
    wrong = [x for x, w in zip(xs[:n_small], want) if not same_bits(exp_neg_rn_uncontracted(x), w)]
    lines.append("exp_neg_rn: the uncontracted source is correctly rounded at %d of %d arguments below 2^-6"
                 % (n_small - len(wrong), n_small))
    assert not wrong, wrong[:5]
    assert all(same_bits(exp_scaled(-x), w) for x, w in zip(xs[n_small:], want[n_small:]))
    sec = doc["log"]
    for name in ["fast_log"] + list(LOG_VARIANTS):
        rows = unpack(sec["x"]) if name == "fast_log" else unpack(sec["x"])[:sec["n_normal"]]
        got = [log_variant(name, x) for x in rows]
        assert all(same_bits(a, b) for a, b in zip(got, unpack(sec["bits"][name]))), name
        worst, ratio, at = log_check(sec, name, got)
        lines.append("%s: worst absolute error %.4g, %.3f of its bar at x = %r (%d rows)" % (name, worst, ratio, at, len(got)))
        assert ratio <= 1.0, (name, worst, ratio, at)
    for grp in doc["rates"]:
        k, r, S = grp["k"], grp["r"], grp["S"]
        rows = rate_rows(grp)
        got = [error_class_rate_mul(k, r, c, e, s, S) for c, e, s in rows]
        assert all(same_bits(a, b) for a, b in zip(got, unpack(grp["bits"])))
        rel = relative_errors(got, unpack(grp["ref"]), grp["resid"])
        bar = rate_mul_bar(k, S)
        lines.append("rates by multiplication, k = %d, S = %d: worst relative %.3g (bar %.3g)" % (k, S, max(rel), bar))
        assert max(rel) <= bar, (k, S, float(max(rel)))
    sec = doc["weights"]
    rows = weight_rows(sec)
    got = [copy_number_weight_by_squaring(*row) for row in rows]
    assert all(same_bits(a, b) for a, b in zip(got, unpack(sec["bits"])))
    rel = relative_errors(got, unpack(sec["ref"]), sec["resid"])
    worst = max(range(len(rel)), key=lambda i: rel[i])
    lines.append("weights by squaring: worst relative %.3g at %r (bar %.3g)" % (rel[worst], rows[worst], WEIGHT_SQ_BAR))
    assert rel[worst] <= WEIGHT_SQ_BAR, (rows[worst], float(rel[worst]))
    return lines
