"""The yardstick of tests/test_gpu_math.py, checked where no GPU is needed: the bit-exact restatements of the device's
scalar math (tests/math_reference.py) stay inside every bar against the 50-digit values of
tests/golden/math_primitives.json -- so a failure on the device is the device's --, the table the restatement uses is the
table the kernels use (tools/gen_log_table.py 256 reproduces covest_amd/csrc/log_table.h byte for byte), and the fixture's
generator reproduces the committed file."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import pytest

import math_reference as R
from conftest import GOLDEN, REPO, load_golden

sys.path.insert(0, GOLDEN)

_DOC = R.expand(load_golden("math_primitives.json"))


def test_restatements_inside_every_bar():
    """exp_scaled within 1 ulp (the bound the device library documents for its exp, which the GPU test measures beside
    it); every log variant inside T_DEG + 2^-52 |want| + |fl(ln 2) - ln 2| |e| + 2^-53; the multiplied rates and the
    squared weight inside their counts of roundings; the uncontracted source of exp_neg_rn correctly rounded at every
    argument below 2^-6; every `bits` column of the fixture reproduced."""
    for line in R.check_restatements(_DOC):
        print(line)


def test_raw_bias_constant():
    """kLogRawBias<540>, the double a caller of the RAW log takes off again, against the real 1562 ln 2 that the RAW
    log's bar is stated for: its own rounding and 1562 times the error of fl(ln 2)."""
    err, bound = R.log_bias_error(R.SCALE_BITS)
    print("kLogRawBias<540> - 1562 ln 2: %.4g (bound %.4g)" % (err, bound))
    assert err <= bound
    assert bound < Fraction(2, 10 ** 13)


def test_plain_squaring_is_what_the_pairs_are_for():
    """The squared weight in plain doubles misses the bar of (2 * 14 + 4) 2^-53 by a factor of about 40 at o = 16384,
    q = 0.01 -- a squaring doubles the relative error it inherits -- and the (hi, lo) pairs of point_fetch.h meet it."""
    row = (0.01, 0.01, 0.01, 16384)
    want = R.mp_weight(*row)
    plain = abs(Fraction(R.copy_number_weight_plain_squaring(*row)) / want - 1)
    pairs = abs(Fraction(R.copy_number_weight_by_squaring(*row)) / want - 1)
    print("weight at o = 16384, q = 0.01: plain doubles %.3g relative, pairs %.3g (bar %.3g)"
          % (plain, pairs, R.WEIGHT_SQ_BAR))
    assert pairs <= R.WEIGHT_SQ_BAR < plain


def test_exp_reach():
    """Up to |x| = EXP_REACH the remainder of the Cody-Waite reduction stays where the polynomial is positive, so the
    final ldexp alone decides: +0 below the doubles' range, +inf above it.  (|t| <= ln 2 / 2 + |x| 2.3e-16: 0.58 at
    1e15.)  Beyond, the restatement shows what the header now says: -0.0, -inf or NaN."""
    for x in (1100.0, 5000.0, 1e6, 1e12, R.EXP_REACH):
        for sc in (0, R.SCALE_BITS):
            if x == 1100.0 and sc:
                continue  # exp(-1100) 2^540 = 6.8e-316 is a subnormal double, not 0 (a row of the fixture)
            assert abs(R.exp_reduce(x)[1]) < 0.58 and abs(R.exp_reduce(-x)[1]) < 0.58
            assert R.same_bits(R.exp_scaled(-x, sc), 0.0), (x, sc)
            assert R.exp_scaled(x, sc) == R.INF, (x, sc)
    assert R.same_bits(R.exp_scaled(-1e20, 0), -0.0)
    assert R.exp_scaled(R.INF, 0) != R.exp_scaled(R.INF, 0)  # NaN


def test_log_table_header_is_the_generator_output(monkeypatch):
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_log_table.py"), "256"], capture_output=True,
                         check=True).stdout
    with open(os.path.join(REPO, "covest_amd", "csrc", "log_table.h"), "rb") as f:
        assert f.read() == out
    # ... and the restated rule gives the same 512 doubles (read from the generator's output, not from the header)
    pairs = re.findall(r"^\s+(\S+), (\S+), //", out.decode(), flags=re.M)
    assert len(pairs) == 256
    rule = [(float.fromhex(a), float.fromhex(b)) for a, b in pairs]
    assert R.log_table() == rule  # (the fixture's copy, which expand() installed: what the GPU tests restate with)
    monkeypatch.setattr(R, "_TABLE", None)
    assert R.log_table() == rule  # the rule as math_reference restates it


def test_fixture_is_reproducible():
    import make_golden_math
    small, full = make_golden_math.build_compact()  # (asserts that expand() re-creates every stored-out column, and
    text = make_golden_math.dumps(small)            # with it that the exact series gives mpmath's rounded exp(-x))
    with open(os.path.join(GOLDEN, "math_primitives.json")) as f:
        assert f.read() == text
    assert full == _DOC
    assert len(text) <= 323569  # tests/golden/kmer_hist.json, the largest fixture before this one


def test_probe_names_match_the_header():
    """covest_amd._capi.MATH_PROBE_FN against the numbered list in include/covest_amd.h."""
    from covest_amd import _capi
    assert sorted(_capi.MATH_PROBE_FN.values()) == list(range(22))
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    assert re.search(r"\b21 copy_number_weight_by_squaring", text) and re.search(r"\b0 exp_fast\(x\)", text)


@pytest.mark.parametrize("name", ["fast_log"] + list(R.LOG_VARIANTS))
def test_a_wrong_table_entry_is_seen(name, monkeypatch):
    """What the bars are for: one table entry off by 1e-12 -- three orders below the 1e-9 the likelihoods are held to --
    leaves every variant's bar, the degree-3 one (6.3e-13) included, at the rows of that interval."""
    sec = _DOC["log"]
    table = list(R.log_table())
    i = 100
    monkeypatch.setattr(R, "_TABLE", table[:i] + [(table[i][0], table[i][1] + 1e-12)] + table[i + 1:])
    rows = R.unpack(sec["x"]) if name == "fast_log" else R.unpack(sec["x"])[:sec["n_normal"]]
    got = [R.log_variant(name, x) for x in rows]
    assert R.log_check(sec, name, got)[1] > 1.0


def test_probe_argument_checks(hip_lib):
    """The probe's argument checks come before any device work, so they are tested here: COVEST_E_INVALID for an
    unknown function, too many elements, a missing array and an iarg or k out of range; n == 0 returns at once."""
    import numpy as np
    from covest_amd import _capi
    x = np.ones(4)
    out = np.empty(4)
    call = lambda fn, n, y, ia, k=0, r=0: hip_lib.covest_math_probe(  # noqa: E731
        -1, fn, n, x.ctypes.data, y, None, ia, k, r, out.ctypes.data)
    fn = _capi.MATH_PROBE_FN
    assert call(99, 4, None, None) == _capi.COVEST_E_INVALID
    assert call(fn["exp_fast"], 65537, None, None) == _capi.COVEST_E_INVALID
    assert call(fn["log_trunc_norm"], 4, None, None) == _capi.COVEST_E_INVALID
    bad = np.array([0, 1, 2, 8], dtype=np.int32)
    assert call(fn["rate_mul_8"], 4, x.ctypes.data, bad.ctypes.data, 21, 100) == _capi.COVEST_E_INVALID
    assert call(fn["rate_mul_8"], 4, x.ctypes.data, bad.ctypes.data, 64, 100) == _capi.COVEST_E_INVALID
    assert call(fn["exp_fast"], 0, None, None) == 0
