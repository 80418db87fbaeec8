"""The truncated-Poisson pmf on the GPU (covest_amd.poisson over tp_eval.hip) against the reference's own vectors:
tests/golden/tp_table.json (519 rows), tp_bitwise.json (3 000 rows, 21 edges) and, in the log domain, tp_log.json.

The tolerance is the project's plain 1e-9 relative against the reference's values.  On the double grid:
|got - ref| <= 1e-9 ref + g, g = 4.94e-324 (one grid step) where ref is subnormal or 0 -- a single term is rounded once,
one step is all the reference's cast can differ by -- and g = 0 otherwise.  Printed while passing: the worst relative
error of each route against the reference rows, and the worst table-versus-pairs difference."""
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist

pytestmark = pytest.mark.gpu

TOL = 1e-9
STEP = 4.94065645841246544e-324
TINY = 2.2250738585072014e-308
EPS = 2.0 ** -52

_TABLE = load_golden("tp_table.json")
_BITWISE = load_golden("tp_bitwise.json")
_LOG = load_golden("tp_log.json")
# the whole list: 519 + 3 000 + 21 pairs
_ROWS = [tuple(r) for r in _TABLE["rows"]] + [tuple(r) for r in _BITWISE["rows"]] + [tuple(r) for r in _BITWISE["edges"]]
_L = np.array([r[0] for r in _ROWS], dtype=np.float64)
_J = np.array([r[1] for r in _ROWS], dtype=np.int64)
_REF = np.array([r[2] for r in _ROWS], dtype=np.float64)
_LOG_AT = {(r[0], r[1]): r[2] for r in _LOG["rows"]}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bound(ref):
    """1e-9 ref + g per entry (module docstring)."""
    ref = np.asarray(ref, dtype=np.float64)
    return TOL * ref + np.where(ref < TINY, STEP, 0.0)


def _worst_rel(got, ref):
    """The largest |got / ref - 1| over the entries whose reference is a finite normal double."""
    ok = np.isfinite(ref) & (ref >= TINY)
    return float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0


@pytest.fixture(scope="module")
def pairs(hip_lib):
    """The whole list through the pairs entry once per mode; shared, not changed."""
    from covest_amd import poisson
    return {mode: poisson.truncated_poisson_many(_L, _J, mode) for mode in ("reference", "value", "log")}


def test_pairs_reference_mode(pairs):
    """Every row of tp_table.json, every row and edge of tp_bitwise.json: finite rows to the bound, the 5 +inf rows
    exactly +inf, everything >= 0 and no NaN."""
    got = pairs["reference"]
    assert len(got) == 3540 and not np.isnan(got).any() and (got >= 0.0).all()
    inf = np.isinf(_REF)
    assert inf.sum() == 5 and (got[inf] == math.inf).all()
    assert not np.isinf(got[~inf]).any()
    diff = np.abs(got[~inf] - _REF[~inf])
    print("pairs, reference mode: worst relative error against the reference rows %.3g (%d finite normal rows, "
          "%d subnormal, %d zeros)" % (_worst_rel(got, _REF), int((np.isfinite(_REF) & (_REF >= TINY)).sum()),
                                       int(((_REF > 0) & (_REF < TINY)).sum()), int((_REF == 0).sum())))
    worst = int(np.argmax(diff - _bound(_REF[~inf])))
    assert (diff <= _bound(_REF[~inf])).all(), (_L[~inf][worst], _J[~inf][worst], got[~inf][worst], _REF[~inf][worst])


def test_pairs_value_mode(pairs):
    """The reference mode's bits wherever the reference is finite; finite where it is +inf, and there
    |ln got - tp_log| <= 1e-9, or got == 0 with tp_log < -745."""
    got, ref_mode = pairs["value"], pairs["reference"]
    inf = np.isinf(_REF)
    assert (_bits(got[~inf]) == _bits(ref_mode[~inf])).all()
    assert np.isfinite(got).all() and (got >= 0.0).all()
    for i in np.nonzero(inf)[0]:
        want = _LOG_AT[(_L[i], int(_J[i]))]
        if got[i] == 0.0:
            assert want < -745.0, (_L[i], _J[i], want)
        else:
            assert abs(math.log(got[i]) - want) <= TOL, (_L[i], _J[i], got[i], want)


def test_pairs_log_mode(pairs, hip_lib):
    """Against tp_log.json: |got - want| <= 1e-9, the value's relative bar expressed in the log; where |want| > 1e4,
    1e-9 + 4 eps |want| (the exponent's own rounding is a few ulps of a number near 9e4).  Finite for every l > 0 of the
    whole list; -inf at l == 0; and the value modes' 0.0 at l == 0 and NaN."""
    from covest_amd import poisson
    got = pairs["log"]
    assert (_L > 0).all() and np.isfinite(got).all()
    at = {(l, int(j)): v for l, j, v in zip(_L.tolist(), _J.tolist(), got.tolist())}
    worst = 0.0
    for l, j, want, _ in _LOG["rows"]:
        bound = TOL + (4 * EPS * abs(want) if abs(want) > 1e4 else 0.0)
        err = abs(at[(l, j)] - want)
        worst = max(worst, err)
        assert err <= bound, (l, j, at[(l, j)], want)
    print("pairs, log mode: worst |got - want| %.3g over %d rows" % (worst, len(_LOG["rows"])))
    # the log is the exponent the value modes feed to exp
    fin = np.isfinite(_REF) & (_REF >= TINY)
    assert np.allclose(np.exp(got[fin]), pairs["value"][fin], rtol=1e-13, atol=0)
    edge_l, edge_j = [0.0, float("nan"), 0.0, float("nan"), 3.0], [1, 1, 700, 9000, 2]
    for mode in ("value", "reference"):
        v = poisson.truncated_poisson_many(edge_l, edge_j, mode)
        assert (_bits(v[:4]) == 0).all() and v[4] > 0  # +0.0 exactly (the extension's early return)
    lg = poisson.truncated_poisson_many(edge_l, edge_j, "log")
    assert lg[0] == -math.inf and lg[2] == -math.inf and math.isfinite(lg[4])
    assert lg[1] == -math.inf and lg[3] == -math.inf  # NaN: the log of the 0.0 the value modes return


# ---- the table route -------------------------------------------------------------------------------------------

def _against_pairs(rates, keys):
    """The table of (rates x keys) by the recurrence, every entry held to the bound against the pairs entry in value
    mode; returns the table and the worst relative difference over the normal entries."""
    from covest_amd import poisson
    rates, keys = np.asarray(rates, dtype=np.float64), np.asarray(keys, dtype=np.int64)
    tab = poisson.truncated_poisson_table(rates, keys)
    assert tab.shape == (len(rates), len(keys))
    want = poisson.truncated_poisson_many(rates[:, None], keys[None, :], "value")
    assert not np.isnan(tab).any() and (tab >= 0).all() and np.isfinite(tab).all()
    diff, bound = np.abs(tab - want), _bound(want)
    if not (diff <= bound).all():
        i, b = np.unravel_index(int(np.argmax(diff - bound)), diff.shape)
        raise AssertionError("table %r vs pairs %r at l = %r, j = %d (n_l = %d, %d keys from %d)"
                             % (tab[i, b], want[i, b], rates[i], keys[b], len(rates), len(keys), keys[0]))
    return tab, _worst_rel(tab.ravel(), want.ravel())


def test_table_against_the_reference_rows_and_the_pairs_entry(hip_lib):
    """Rates: the distinct l > 0 of tp_table.json; keys: its distinct j (417 x 244; this test's table stays
    within 420 x 270).  Every entry with a finite reference row to the bound; the table is the value mode, so the two
    entries where the extension overflows are finite and are held to tp_log.json as test_pairs_value_mode holds them
    (|ln got - tp_log| <= 1e-9, or got == 0 with tp_log < -745); every entry against the pairs entry."""
    rates = sorted({r[0] for r in _TABLE["rows"] if r[0] > 0})
    keys = sorted({r[1] for r in _TABLE["rows"]})
    assert len(rates) <= 420 and len(keys) <= 270
    tab, worst_pairs = _against_pairs(rates, keys)
    ri, kj = {l: i for i, l in enumerate(rates)}, {j: b for b, j in enumerate(keys)}
    got = np.array([tab[ri[l], kj[j]] for l, j, _ in _TABLE["rows"]])
    ref = np.array([r[2] for r in _TABLE["rows"]])
    fin = np.isfinite(ref)
    assert fin.sum() == len(ref) - 2
    print("table: worst relative error against the reference rows %.3g (%d rows); worst relative difference "
          "table vs pairs %.3g (%d entries)" % (_worst_rel(got, ref), int(fin.sum()), worst_pairs, tab.size))
    diff = np.abs(got[fin] - ref[fin])
    worst = int(np.argmax(diff - _bound(ref[fin])))
    assert (diff <= _bound(ref[fin])).all(), (np.array(_TABLE["rows"])[fin][worst], got[fin][worst])
    for (l, j, want_v), v in zip(_TABLE["rows"], got.tolist()):
        if not math.isfinite(want_v):
            want = _LOG_AT[(l, j)]
            if v == 0.0:
                assert want < -745.0, (l, j, want)
            else:
                assert abs(math.log(v) - want) <= TOL, (l, j, v, want)


def _some_rates(n):
    """n rates, fixed: the specials of the normaliser first, then a geometric spread over 1e-9 .. 2e4."""
    special = [199.9, 200.0, 200.1, 400.0, 1e-12, 1e-8, 2e-8, 0.5, 37.0, 450.0, 1100.0, 11400.0]
    spread = np.geomspace(1e-9, 2e4, 129)[::-1]
    return np.array((special + spread.tolist())[:n], dtype=np.float64)


_KEY_LISTS = {
    "one key": [5],
    "32 consecutive": list(range(7, 39)),
    "33 consecutive": list(range(7, 40)),
    "65 consecutive": list(range(7, 72)),
    "gapped": [1, 2, 3, 500, 501, 9000],
    "starts at 16384": [16384],
    "ends at 16384": list(range(16384 - 40, 16385)),
    "bridged gaps": [10, 11, 14, 27, 28, 60, 61],  # gaps of up to 12 keys are walked through filler keys
}


@pytest.mark.parametrize("name", sorted(_KEY_LISTS))
def test_table_shapes(hip_lib, name):
    """n_l in {1, 63, 64, 65, 129} (a lane per rate, a workgroup per 64) against key lists that end inside, at and
    beyond a tile of 32 keys, with gaps that start a new run and gaps that are bridged, and at the top of the range."""
    worst = 0.0
    for n_l in (1, 63, 64, 65, 129):
        worst = max(worst, _against_pairs(_some_rates(n_l), _KEY_LISTS[name])[1])
    print("table, %s: worst relative difference table vs pairs %.3g" % (name, worst))


def test_table_first_key_beyond_the_mode(hip_lib):
    """Rates of 0.5 .. 200 against keys from 300 on: every stream is anchored past its mode and only falls."""
    rates = np.concatenate([np.linspace(0.5, 200.0, 65), [199.9, 200.0, 37.0]])
    tab, worst = _against_pairs(rates, list(range(300, 300 + 70)))
    assert (tab[-1] > 0).any() and (np.diff(tab[-1]) <= 0).all()
    print("table, first key beyond the mode: worst relative difference table vs pairs %.3g" % worst)


def test_table_streams_that_start_below_the_window(hip_lib):
    """Rates for which ln x k0 - D(x) + ln 2^540 lies in (-745, -708) at the first key (k0 = 1: x of about 1083 ..
    1119), so that the stream may not be anchored there and comes on inside a later tile --
    the values cross the subnormal range near key 100 -- and is anchored afresh behind the gap."""
    rates = np.linspace(1090.0, 1119.0, 65)
    for k0 in (0.0, 1.0):  # at the key the anchor is taken at (k0 - 1 = 0: -D(x) = -x alone), and at the first key itself
        first = np.log(rates) * k0 - rates + 540 * math.log(2.0)
        assert ((first > -745.0) & (first < -708.0)).all()
    keys = list(range(1, 161)) + list(range(1000, 1200))
    tab, worst = _against_pairs(rates, keys)
    assert (tab[:, :60] == 0.0).all() and (tab[:, 159] > TINY).all() and (tab[:, -1] > 1e-6).all()
    assert ((tab > 0) & (tab < TINY)).any()
    print("table, streams below the window: worst relative difference table vs pairs %.3g" % worst)


# ---- repeatability, independence, the scalar ---------------------------------------------------------------------

def test_a_pairs_bits_do_not_depend_on_the_call(pairs, hip_lib):
    """Call sizes 1, 256, 257 (either side of the in-place boundary), 3 021 (all of tp_bitwise.json) and 3 540 (the
    whole list); a repeated call; the scalar entry."""
    from covest_amd import poisson
    for mode in ("reference", "value", "log"):
        whole = pairs[mode]
        assert (_bits(poisson.truncated_poisson_many(_L, _J, mode)) == _bits(whole)).all()
        for first, n in ((0, 256), (300, 257), (3540 - 256, 256), (1000, 257), (519, 3021)):
            part = poisson.truncated_poisson_many(_L[first:first + n], _J[first:first + n], mode)
            assert (_bits(part) == _bits(whole[first:first + n])).all(), (mode, first, n)
        for i in (0, 255, 256, 518, 519, 2000, 3539):
            one = poisson.truncated_poisson_many(_L[i:i + 1], _J[i:i + 1], mode)
            assert _bits(one)[0] == _bits(whole)[i], (mode, i)
    inf_at = int(np.nonzero(np.isinf(_REF))[0][0])
    for i in (0, 7, 518, inf_at, 3539):
        v = poisson.truncated_poisson(float(_L[i]), int(_J[i]))
        assert isinstance(v, float) and _bits([v])[0] == _bits(pairs["reference"])[i]


def test_tie_to_the_likelihood_kernels(hip_lib):
    """A basic model with max_error = 1, k = r = 1 at e = 0 has ONE mixture component of weight 1 and rate c: its
    compute_probabilities(c, 0) is the pmf itself through K-direct, and equals the pairs entry bit for bit."""
    from covest_amd import BasicModel, poisson
    hist = load_hist("H256")
    m = BasicModel(1, 1, hist, 0, max_error=1)
    keys = list(hist.keys())
    for c in (0.5, 37.0, 450.0):
        p = m.compute_probabilities(c, 0)
        got = np.array([p[j] for j in keys])
        want = poisson.truncated_poisson_many(np.full(len(keys), c), keys, "value")
        assert (got > 0).any()
        assert (_bits(got) == _bits(want)).all(), c
    m.close()
