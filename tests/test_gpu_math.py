"""The device's scalar math on its own (covest_math_probe over csrc/math_probe.hip): exp_scaled / exp_fast, exp_neg_rn,
the fast_log family and its table, log_trunc_norm in both forms and its derivatives, the error classes' rates and the
copy numbers' weights -- the layer every likelihood, gradient and posterior of the library stands on, which the other
tests reach only through sums held to 1e-9.

Everything comes from tests/golden/math_primitives.json (tests/golden/make_golden_math.py) -- the 50-digit values, the
fixed inputs and the log table; the seeded and rule-made inputs and the restatements' bits are re-created from their
rules by math_reference.expand, in exact arithmetic, no mpmath -- and each function takes one launch of at most a few
thousand elements.  Three kinds of claim:
  bit equality   exp_scaled and every log instantiation against the restatement in exact arithmetic
                 (tests/math_reference.py); exp_neg_rn against the correctly rounded exp(-x); functions that must agree
                 with each other (fast_log_n<4> and fast_log, error_class_rate_mul and error_class_rates<S>,
                 trunc_norm_dlog and the first output of trunc_norm_dlog2)
  accuracy       against the 50-digit value within a bar that is derived (math_reference.py: the logs, the multiplied
                 rates, the squared weight, log_trunc_norm), or measured in the same run against the device library
                 (exp_scaled: the library's own worst error on the same inputs plus half an ulp)
  pinned         what exp_scaled returns beyond the range it is good for (fastmath.h): recorded, equal to the restatement

The range of exp_scaled that callers can reach (fastmath.h states it): exp_scaled(a0, 540) is USED only where the
log-term a0 lies in the window, a0 > -760 (streams.h), and a0 <= ln of a mixture term, far below 709.78 - 374.3;
exp_fast(-xr) in log_trunc_norm has xr in [1, 200]; exp_neg_rn(x) has x = o lambda_s >= 2^-6 with o <= 16384 and
lambda_s <= c, the coverage -- bounded by max_cov in the basic model and by nothing in the repeats model (clamp_point: its
upper bound is None), so in principle any finite double.  The normaliser itself is defined up to x = 200 x 2^53 = 1.8e18
(log_trunc_norm forms x / 200 in a double; covest_truncated_poisson accepts any rate), and the reference does not return
at all beyond 2^61.  Inside |x| <= 1e15 the specials are ASSERTED here: +0 with its sign below the range, +inf above.
Between 1e15 and 1.8e18 the one deviation is the sign of the zero of exp_fast(-x) (pinned at -1e20 below), which its only
consumer there, 1.0 - exp_neg_rn(x), cannot see.
"""
import math
from fractions import Fraction

import pytest

import math_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

_DOC = R.expand(load_golden("math_primitives.json"))  # every row in place (math_reference.expand)
LOG_NAMES = ["fast_log", "fast_log_n4"] + list(R.LOG_VARIANTS)

# trunc_norm_dlog / trunc_norm_dlog2 against the 50-digit derivatives, measured on an MI355X (profiles/
# math_primitives.txt): the worst relative error of L' and of L''.  The bar is twice each, and must stay below 1e-14.
DLOG_MEASURED = {"d1": 1.41e-16, "d2": 2.73e-16}
DLOG_CEILING = 1e-14


@pytest.fixture(scope="module")
def probe(hip_lib):
    from covest_amd import _capi

    def run(name, x, **kw):
        return [float(v) for v in _capi.math_probe(name, x, **kw)]
    return run


def _mismatches(got, want):
    return [i for i, (a, b) in enumerate(zip(got, want)) if not R.same_bits(a, b)]


@pytest.mark.parametrize("sc", [0, R.SCALE_BITS])
def test_exp_scaled(probe, sc):
    """Bit equality with the restatement on every row -- subnormal results, the IEEE specials and the rows beyond the
    asserted range included -- and the worst error in ulps inside the library's own on the same inputs plus 0.5."""
    sec = _DOC["exp"][str(sc)]
    xs = R.unpack(sec["x"])
    got = probe("exp_scaled", xs, iarg=[sc] * len(xs))
    bad = _mismatches(got, R.unpack(sec["bits"]))
    assert not bad, [(xs[i], got[i], R.unpack(sec["bits"])[i]) for i in bad[:5]]
    if sc == 0:
        assert not _mismatches(probe("exp_fast", xs), got)
    library = probe("exp_library", xs)
    base, base_at = R.exp_worst_ulps(sec, library, scale_back=sc)
    worst, at = R.exp_worst_ulps(sec, got)
    print("math: exp_scaled(x, %d): worst %.4f ulp at x = %r; the device library's exp on the same inputs: %.4f ulp at "
          "x = %r (%d rows)" % (sc, worst, at, base, base_at, len(xs)))
    assert worst <= base + 0.5, (worst, at, base)


@pytest.mark.parametrize("sc", [0, R.SCALE_BITS])
def test_exp_scaled_specials(probe, sc):
    """-inf gives +0, NaN gives NaN; inside |x| <= 1e15 overflow gives +inf and underflow +0, sign checked.  Beyond
    that range the returned values are recorded and pinned to the restatement (fastmath.h says what they are)."""
    shift = sc * math.log(2.0)
    inside = [m for m in (1100.0, 5000.0, 1e6, 1e9, 1e12, 1e15)]
    xs = [-math.inf, math.nan, 0.0, -0.0] + inside + [-m for m in inside]
    got = probe("exp_scaled", xs, iarg=[sc] * len(xs))
    assert R.same_bits(got[0], 0.0) and got[1] != got[1]
    assert got[2] == got[3] == math.ldexp(1.0, sc)
    for x, g in zip(xs[4:], got[4:]):
        if x + shift > 709.79:
            assert g == math.inf, (x, g)
        elif x + shift < -745.14:
            assert R.same_bits(g, 0.0), (x, g)  # +0: the sign too
        else:  # exp(-1100) 2^540, a subnormal double
            assert 0.0 < g < 2.2250738585072014e-308, (x, g)
    beyond = [1e20, -1e20, 1e300, -1e300, math.inf]
    out = probe("exp_scaled", beyond, iarg=[sc] * len(beyond))
    print("math: exp_scaled(x, %d) beyond the range: %s" % (sc, ", ".join("%r -> %r" % p for p in zip(beyond, out))))
    assert not _mismatches(out, [R.exp_scaled(x, sc) for x in beyond])


def test_exp_neg_rn(probe):
    """The correctly rounded exp(-x) below 2^-6 -- 0, 1e-300, every power of two from 2^-60, 2 000 seeded arguments --
    and exp_fast(-x)'s bits from 2^-6 on."""
    sec = _DOC["exp_neg_rn"]
    xs, want = R.unpack(sec["x"]), R.unpack(sec["want"])
    got = probe("exp_neg_rn", xs)
    bad = _mismatches(got, want)
    small = [i for i in bad if i < sec["n_small"]]
    print("math: exp_neg_rn: correctly rounded at %d of %d arguments below 2^-6; exp_fast(-x)'s bits at %d of %d from 2^-6"
          % (sec["n_small"] - len(small), sec["n_small"], len(xs) - sec["n_small"] - (len(bad) - len(small)),
             len(xs) - sec["n_small"]))
    assert not bad, [(xs[i], got[i], want[i]) for i in bad[:5]]


@pytest.fixture(scope="module")
def logs(probe):
    """Every log variant over its rows, once; shared, not changed."""
    sec = _DOC["log"]
    xs = R.unpack(sec["x"])
    return {name: probe(name, xs if name in ("fast_log", "fast_log_n4") else xs[:sec["n_normal"]]) for name in LOG_NAMES}


@pytest.mark.parametrize("name", LOG_NAMES)
def test_log_variant(logs, name):
    """Bit equality with the restatement (table, Horner steps, the exponent's fma, the final add), and the error
    against the 50-digit log inside T_DEG + 2^-52 |want| + |fl(ln 2) - ln 2| |e| + 2^-53."""
    sec = _DOC["log"]
    got = logs[name]
    want = R.unpack(sec["bits"]["fast_log" if name == "fast_log_n4" else name])
    bad = _mismatches(got, want)
    xs = R.unpack(sec["x"])
    assert not bad, [(xs[i], got[i], want[i]) for i in bad[:5]]
    worst, ratio, at = R.log_check(sec, name, got)
    print("math: %s: worst absolute error %.4g; worst share of the bar %.3f at x = %r (%d rows)"
          % (name, worst, ratio, at, len(got)))
    assert ratio <= 1.0, (name, worst, ratio, at)


def test_log_family_agrees(logs, probe):
    """fast_log_n<4> is fast_log element by element; fast_log(0) is finite; the constant a caller of the RAW log takes
    off again is within its own bound of the real 1562 ln 2 the RAW bar is stated for."""
    assert not _mismatches(logs["fast_log_n4"], logs["fast_log"])
    assert all(math.isfinite(v) for v in probe("fast_log", [0.0]) + probe("fast_log_n4", [0.0, 0.0, 0.0, 0.0]))
    err, bound = R.log_bias_error(R.SCALE_BITS)
    assert err <= bound


def test_log_trunc_norm(probe):
    """Piece by piece against the reference's normaliser at 50 digits.  Without the table: inside 2^-51 max(1, |value|)
    (math_reference.trunc_norm_plain_bar), plus one step of the 2^-63 grid where the residual is below 2^-10.  With
    the table: inside the plain form's worst error of that piece, measured here, plus the logs' bar for the one
    fast_log it substitutes, plus the same grid step."""
    sec = _DOC["log_trunc_norm"]
    xs, ys = R.unpack(sec["x"]), R.unpack(sec["y"])
    plain = R.trunc_norm_errors(sec, probe("log_trunc_norm", xs, y=ys))
    table = R.trunc_norm_errors(sec, probe("log_trunc_norm_table", xs, y=ys))
    plain_worst = R.worst_by_piece(plain, lambda row: row[2])
    table_worst = R.worst_by_piece(table, lambda row: row[2])
    for piece in sorted(plain_worst):
        print("math: log_trunc_norm, piece %-12s worst absolute error %.4g without the table, %.4g with it"
              % (piece + ":", plain_worst[piece], table_worst[piece]))
    for piece, x, err, value, step, _ in plain:
        assert err <= R.trunc_norm_plain_bar(value) + step, (piece, x, float(err))
    for piece, x, err, value, step, arg in table:
        bar = Fraction(plain_worst[piece]) + step + (R.fast_log_bar_at(arg) if arg is not None else 0)
        assert err <= bar, (piece, x, float(err), float(bar))


def test_trunc_norm_derivatives(probe):
    """L' and L'' against the 50-digit derivatives inside each piece: within twice the measured worst, below 1e-14
    relative; the first output of trunc_norm_dlog2 is trunc_norm_dlog bit for bit."""
    sec = _DOC["log_trunc_norm"]
    xs = R.unpack(sec["x"])
    d1 = probe("trunc_norm_dlog", xs)
    first, second = probe("trunc_norm_dlog2_first", xs), probe("trunc_norm_dlog2_second", xs)
    assert not _mismatches(first, d1)
    for key, got in (("d1", d1), ("d2", second)):
        rel = R.relative_errors(got, R.unpack(sec[key]), sec[key + "_resid"])
        by_piece = R.worst_by_piece(list(zip(sec["piece"], rel)), lambda row: row[1])
        print("math: trunc_norm_dlog %s: worst relative error %.4g; by piece: %s"
              % (key, max(rel), ", ".join("%s %.3g" % p for p in sorted(by_piece.items()))))
        bar = 2 * DLOG_MEASURED[key]
        assert bar <= DLOG_CEILING
        worst = max(range(len(rel)), key=lambda i: rel[i])
        assert rel[worst] <= bar, (key, xs[worst], float(rel[worst]))


def test_error_class_rates(probe):
    """error_class_rate_mul(s, S) is error_class_rates<S>[s] bit for bit, class by class; both within
    (2 ceil(log2 k) + S + 4) 2^-53 relative of the 50-digit rate formed from the double 1 - e; the pow form within its
    own count of roundings (two calls of the library's pow at 2 ulp each)."""
    worst_pow = 0.0
    for grp in _DOC["rates"]:
        k, r, S = grp["k"], grp["r"], grp["S"]
        rows = R.rate_rows(grp)
        c, e, s = [list(col) for col in zip(*rows)]
        mul = probe("rate_mul_%d" % S, c, y=e, iarg=s, k=k, r=r)
        all_classes = probe("rates_%d" % S, c, y=e, iarg=s, k=k, r=r)
        assert not _mismatches(mul, all_classes), (k, S)
        rel = R.relative_errors(mul, R.unpack(grp["ref"]), grp["resid"])
        same = len(rows) - len(_mismatches(mul, R.unpack(grp["bits"])))
        print("math: rates by multiplication, k = %d, S = %d: worst relative error %.3g (bar %.3g); %d of %d rows carry "
              "the float restatement's bits" % (k, S, max(rel), R.rate_mul_bar(k, S), same, len(rows)))
        assert max(rel) <= R.rate_mul_bar(k, S), (k, S, float(max(rel)))
        if S == 16:  # the pow form where its exponent k - s is not negative
            keep = [i for i, row in enumerate(rows) if row[2] <= k]
            got = probe("rate_pow", [c[i] for i in keep], y=[e[i] for i in keep], iarg=[s[i] for i in keep], k=k, r=r)
            ref, resid = R.unpack(grp["ref"]), grp["resid"]
            rel = R.relative_errors(got, [ref[i] for i in keep], [resid[i] for i in keep])
            worst_pow = max(worst_pow, float(max(rel)))
            assert max(rel) <= R.RATE_POW_BAR, (k, float(max(rel)))
    print("math: rates by pow: worst relative error %.3g (bar %.3g)" % (worst_pow, R.RATE_POW_BAR))


def test_copy_number_weights(probe):
    """copy_number_weight_by_squaring within (2 * 14 + 4) 2^-53 relative of the 50-digit weight formed from the doubles
    1 - q1, 1 - q2 and 1 - q, at o up to 16384, and equal to the restatement of its (hi, lo) pairs bit for bit; the pow
    form within its own count of roundings."""
    sec = _DOC["weights"]
    rows = R.weight_rows(sec)
    q1, q2, q, o = [list(col) for col in zip(*rows)]
    ref, resid = R.unpack(sec["ref"]), sec["resid"]
    got = probe("weight_squaring", q1, y=q2, z=q, iarg=o)
    rel = R.relative_errors(got, ref, resid)
    worst = max(range(len(rel)), key=lambda i: rel[i])
    by_pow = R.relative_errors(probe("weight_pow", q1, y=q2, z=q, iarg=o), ref, resid)
    print("math: weights by squaring: worst relative error %.3g at %r (bar %.3g); by pow: %.3g (bar %.3g)"
          % (rel[worst], rows[worst], R.WEIGHT_SQ_BAR, max(by_pow), R.WEIGHT_POW_BAR))
    assert rel[worst] <= R.WEIGHT_SQ_BAR, (rows[worst], float(rel[worst]))
    assert max(by_pow) <= R.WEIGHT_POW_BAR
    bad = _mismatches(got, R.unpack(sec["bits"]))
    assert not bad, [(rows[i], got[i]) for i in bad[:5]]
