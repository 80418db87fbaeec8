"""The analytic gradient of a histogram batch on the device (HistogramBatch.loglikelihood_gradient_cross / _pairs,
score_table) against the 50-digit restatement of tests/golden/batch_grad.json
(tests/golden/make_golden_batch_grad.py; the shapes are tests/batch_grad_shapes.py's), against the batch's value methods,
against a twin model through the derivative kernel, and its conventions: the dead key, NaN, the clamp, chunks, and that a
result does not depend on what else is in the call.  The bounds are the derivative tests' own (tests/parity_helpers.py):
1e-9 relative for the value, 1e-9 Cg_k plus the tail term's first-order slack per gradient component."""
import functools
import math

import numpy as np
import pytest

import batch_grad_shapes as S
from conftest import load_golden, rel_err
from parity_helpers import TOL, _grad_bound, _model, _tail_delta

pytestmark = pytest.mark.gpu

NAMES = list(S.SHAPES)
TOL_KERNELS = 1e-11  # between the derivative kernel's value and K-direct's (tests/test_gpu_deriv_shapes.py)
CHUNK_POINTS_256 = (1 << 28) // (3 * 256 * 8)  # batch_host.h batch_points_per_chunk at 3 rows a point: basic model, 256 keys


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_golden("batch_grad.json")


def _open(name, counts=None, tails=None):
    """(model, batch) of a shape; the caller closes both."""
    from covest_amd import HistogramBatch
    case = S.shape(name)
    hist = case["spec"]["hist"]
    m = _model(case["spec"], hist=dict(zip(hist["keys"], hist["counts"])))
    return m, HistogramBatch(m, case["counts"] if counts is None else counts, case["tails"] if tails is None else tails)


_CROSS = {}


def _cross(name):
    """Computed once per shape and shared, never changed: (ll (B, n), grad (B, n, P)) of the shape's batch at its points."""
    if name not in _CROSS:
        m, batch = _open(name)
        _CROSS[name] = batch.loglikelihood_gradient_cross(S.shape(name)["points"])
        batch.close()
        m.close()
    return _CROSS[name]


def _rows_match(name):
    case, g = S.shape(name), _fixture()["shapes"][name]
    assert np.array_equal(case["points"], np.array(g["points"])) and case["counts"].sum(axis=1).tolist() == g["row_sums"]
    assert case["tails"].tolist() == g["tails"]
    return case, g


def _check_entry(name, g, case, b, i, ll, grad, worst):
    """One (b, i) of a shape against the fixture; returns 1 if it was compared."""
    what = (name, b, i)
    if [b, i] in g["special"]:
        assert ll == -math.inf and np.all(np.isnan(grad)), (what, ll, grad)
        return 1
    if any(d[0] == b and d[1] == i for d in g["dropped"]):
        return 0
    e = rel_err(float(ll), g["ll"][b][i])
    worst["ll"] = max(worst["ll"], e)
    assert e <= TOL, (what, float(ll), g["ll"][b][i])
    delta = _tail_delta(g["n_keys"])
    for k, want in enumerate(g["grad"][b][i]):
        C = g["Cg"][b][i][k]
        bound = _grad_bound(case["tails"][b], g["sp"][i], C, g["D"][i][k], delta)
        diff = abs(float(grad[k]) - want)
        if C > 0:
            worst["g"] = max(worst["g"], diff / C)
        assert diff <= bound, (what, k, float(grad[k]), want, diff, bound)
    return 1


@pytest.mark.parametrize("name", NAMES)
def test_cross_against_the_fixture(hip_lib, name):
    """Every kept (b, i): ll to 1e-9 relative, every component within _grad_bound; the dead-key entry -inf and NaN.  The
    uncompensated MFMA sum costs at most n_keys 2^-53 Cg (3e-14 Cg at 257 keys): the bounds are not loosened for it."""
    case, g = _rows_match(name)
    ll, grad = _cross(name)
    assert ll.shape == (g["B"], g["n"]) and grad.shape == (g["B"], g["n"], len(case["points"][0]))
    worst, n = {"ll": 0.0, "g": 0.0}, 0
    for b in range(g["B"]):
        for i in range(g["n"]):
            n += _check_entry(name, g, case, b, i, ll[b, i], grad[b, i], worst)
    assert n == g["B"] * g["n"] - len(g["dropped"])
    print("%s: %d entries, worst ll rel %.3g, worst |dg| / Cg %.3g" % (name, n, worst["ll"], worst["g"]))


def _requests(name):
    """Every (b, i) of the shape in a seeded shuffle, the first seven once more at the end."""
    g = _fixture()["shapes"][name]
    cells = [(b, i) for b in range(g["B"]) for i in range(g["n"])]
    order = np.random.default_rng([S.SEED, 11, NAMES.index(name)]).permutation(len(cells))
    cells = [cells[at] for at in order]
    return cells + cells[:7]


@pytest.mark.parametrize("name", NAMES)
def test_pairs_against_the_fixture_and_against_cross(hip_lib, name):
    """The pairs form with the fixture's bounds; and entry by entry against the cross form within 4 n_keys 2^-53 C,
    C = sum_j h_bj |row_j| + tail_b |t|, formed on the host from score_table: two orders of one sum.  Specials exact."""
    case, g = _rows_match(name)
    m, batch = _open(name)
    cells = _requests(name)
    pts = case["points"][[i for _, i in cells]]
    ll, grad = batch.loglikelihood_gradient_pairs([b for b, _ in cells], pts)
    log_p, score, tail = batch.score_table(case["points"])
    batch.close()
    m.close()
    P = pts.shape[1]
    assert ll.shape == (len(cells),) and grad.shape == (len(cells), P)
    worst, n = {"ll": 0.0, "g": 0.0}, 0
    for at, (b, i) in enumerate(cells):
        n += _check_entry(name, g, case, b, i, ll[at], grad[at], worst)
    cross_ll, cross_grad = _cross(name)
    H, tails = case["counts"], case["tails"]
    unit = 4.0 * g["n_keys"] * 2.0 ** -53
    worst_pair = 0.0
    for at, (b, i) in enumerate(cells):
        got = np.concatenate([[ll[at]], grad[at]])
        ref = np.concatenate([[cross_ll[b, i]], cross_grad[b, i]])
        if not np.all(np.isfinite(ref)):
            assert np.array_equal(got, ref, equal_nan=True), (name, b, i, got, ref)
            continue
        rows = np.concatenate([log_p[i][None, :], score[i]], axis=0)
        C = np.abs(rows) @ H[b] + tails[b] * np.abs(tail[i])
        assert np.all(np.abs(got - ref) <= unit * C), (name, b, i, got, ref, unit * C)
        worst_pair = max(worst_pair, float(np.max(np.abs(got - ref) / np.where(C > 0, C, 1.0))))
    print("%s: %d requests, against the fixture worst ll rel %.3g, |dg| / Cg %.3g; pairs against cross worst |d| / C %.3g" % (
        name, len(cells), worst["ll"], worst["g"], worst_pair))


@pytest.mark.parametrize("name", [n for n in NAMES if "zero_tail1" in S.shape(n)["rows"]])
def test_the_zero_row_with_tail_one_is_the_tail_array(hip_lib, name):
    case = S.shape(name)
    m, batch = _open(name)
    _, _, tail = batch.score_table(case["points"])
    batch.close()
    m.close()
    ll, grad = _cross(name)
    b = case["rows"]["zero_tail1"]
    assert ll[b].tobytes() == np.ascontiguousarray(tail[:, 0]).tobytes()
    assert grad[b].tobytes() == np.ascontiguousarray(tail[:, 1:]).tobytes()
    if "zero_tail0" in case["rows"]:
        assert not ll[case["rows"]["zero_tail0"]].any() and not grad[case["rows"]["zero_tail0"]].any()


@pytest.mark.parametrize("name", NAMES)
def test_the_value_is_the_value_methods_to_1e_11(hip_lib, name):
    """Value and gradient come from one table, the derivative kernel's: its value is K-direct's table's to 1e-11
    relative on every finite entry, the specials in the same places."""
    case = S.shape(name)
    m, batch = _open(name)
    value = batch.loglikelihood_cross(case["points"])
    cells = _requests(name)
    idx, pts = [b for b, _ in cells], case["points"][[i for _, i in cells]]
    value_pairs = batch.loglikelihood_pairs(idx, pts)
    grad_pairs = batch.loglikelihood_gradient_pairs(idx, pts)[0]
    batch.close()
    m.close()
    worst = 0.0
    for got, want in ((_cross(name)[0], value), (grad_pairs, value_pairs)):
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        for a, b in zip(got.reshape(-1), want.reshape(-1)):
            e = rel_err(float(a), float(b))
            worst = max(worst, e)
            assert e <= TOL_KERNELS, (name, float(a), float(b))
    print("%s: value against loglikelihood_cross / _pairs, worst rel %.3g" % (name, worst))


@pytest.mark.parametrize("name", NAMES)
def test_the_own_row_against_a_twin_model(hip_lib, name):
    """The own-counts row is the model's own histogram and tail: model.loglikelihood_gradient_points gives the same value
    to 1e-11 relative and the same gradient within the fixture's bound."""
    case, g = _rows_match(name)
    hist = case["spec"]["hist"]
    m = _model(case["spec"], hist=dict(zip(hist["keys"], hist["counts"])))
    ll_m, grad_m = m.loglikelihood_gradient_points(case["points"])
    m.close()
    ll, grad = _cross(name)
    b = case["rows"]["own"]
    delta = _tail_delta(g["n_keys"])
    for i in range(g["n"]):
        if not math.isfinite(ll_m[i]):
            assert ll[b, i] == ll_m[i] and np.all(np.isnan(grad[b, i])) and np.all(np.isnan(grad_m[i]))
            continue
        assert rel_err(float(ll[b, i]), float(ll_m[i])) <= TOL_KERNELS, (name, i, ll[b, i], ll_m[i])
        if any(d[0] == b and d[1] == i for d in g["dropped"]):
            continue
        for k in range(grad.shape[2]):
            bound = _grad_bound(case["tails"][b], g["sp"][i], g["Cg"][b][i][k], g["D"][i][k], delta)
            assert abs(float(grad[b, i, k]) - float(grad_m[i, k])) <= bound, (name, i, k, grad[b, i, k], grad_m[i, k], bound)


@pytest.mark.parametrize("name", ["basic-dead", "repeats-dead"])
def test_the_dead_key(hip_lib, name):
    """The row that counts the dead key gets -inf and NaN, the row with that count zeroed is finite and within the
    fixture's bounds, the zero row is untouched (0 x +0.0 = 0), and the finite points beside the dead one in the same call
    are, bit for bit, what they are in a call without it."""
    case, g = _rows_match(name)
    ll, grad = _cross(name)
    rows = case["rows"]
    assert ll[rows["dead"], 0] == -math.inf and np.all(np.isnan(grad[rows["dead"], 0]))
    assert g["special"] == [[rows["dead"], 0]] and g["log10_dead_p"] < -400
    assert math.isfinite(ll[rows["alive"], 0]) and np.all(np.isfinite(grad[rows["alive"], 0]))
    assert not any(d[0] == rows["alive"] and d[1] == 0 for d in g["dropped"])
    worst = {"ll": 0.0, "g": 0.0}
    assert _check_entry(name, g, case, rows["alive"], 0, ll[rows["alive"], 0], grad[rows["alive"], 0], worst) == 1
    assert np.all(np.isfinite(ll[:, 1:])) and np.all(np.isfinite(grad[:, 1:]))
    m, batch = _open(name)
    without = batch.loglikelihood_gradient_cross(case["points"][1:])
    info = batch.info()
    log_p, score, _ = batch.score_table(case["points"][:1])
    batch.close()
    m.close()
    assert info["dead_points"] == 0
    assert without[0].tobytes() == np.ascontiguousarray(ll[:, 1:]).tobytes()
    assert without[1].tobytes() == np.ascontiguousarray(grad[:, 1:]).tobytes()
    at = case["spec"]["hist"]["keys"].index(S.ISOLATED)
    dead_keys = np.flatnonzero((log_p[0] == 0.0) & ~np.signbit(log_p[0]))
    assert at in dead_keys and not np.signbit(score[0, :, at]).any() and not score[0][:, dead_keys].any()


@pytest.mark.parametrize("name", ["basic-k65-B5-n22", "repeats-k65-B15-n11"])
def test_nan_and_the_clamp(hip_lib, name):
    """A NaN parameter gives NaN everywhere for that point and nowhere else; a point outside the bounds gives exactly 0.0
    for each parameter the clamp moved (and the fixture has such points: its last two)."""
    case, g = _rows_match(name)
    ll, grad = _cross(name)
    n = g["n"]
    assert any(g["moved"][n - 2]) and any(g["moved"][n - 1]) and not any(any(mv) for mv in g["moved"][:n - 2])
    for i in (n - 2, n - 1):
        for k, mv in enumerate(g["moved"][i]):
            if mv:
                assert not grad[:, i, k].any() and not np.signbit(grad[:, i, k]).any(), (name, i, k, grad[:, i, k])
            else:
                assert grad[case["rows"]["own"], i, k] != 0.0
    pts = case["points"].copy()
    pts[3, 0 if case["kind"] == "basic" else 4] = math.nan
    m, batch = _open(name)
    ll_n, grad_n = batch.loglikelihood_gradient_cross(pts)
    idx = np.arange(n) % g["B"]
    pll_n, pgrad_n = batch.loglikelihood_gradient_pairs(idx, pts)
    batch.close()
    m.close()
    assert np.all(np.isnan(ll_n[:, 3])) and np.all(np.isnan(grad_n[:, 3])) and math.isnan(pll_n[3]) and np.all(np.isnan(pgrad_n[3]))
    keep = np.arange(n) != 3
    assert ll_n[:, keep].tobytes() == ll[:, keep].tobytes() and grad_n[:, keep].tobytes() == grad[:, keep].tobytes()
    assert np.all(np.isfinite(pll_n[keep])) and np.all(np.isfinite(pgrad_n[keep]))


@pytest.mark.parametrize("name", ["basic-k63-B15-n21", "repeats-k257-B15-n10"])
def test_a_result_does_not_depend_on_the_call(hip_lib, name):
    """A pairs request alone equals, bit for bit, the same request inside a list of 300; a cross entry equals, bit for
    bit, the same histogram and point in a batch of B = 1 evaluated at n = 1."""
    from covest_amd import HistogramBatch
    case = S.shape(name)
    rng = np.random.default_rng([S.SEED, 13, NAMES.index(name)])
    B, n = case["counts"].shape[0], len(case["points"])
    idx, at = rng.integers(0, B, 300), rng.integers(0, n, 300)
    m, batch = _open(name)
    ll, grad = batch.loglikelihood_gradient_pairs(idx, case["points"][at])
    for r in (0, 63, 64, 150, 299):
        one = batch.loglikelihood_gradient_pairs([idx[r]], case["points"][at[r]][None, :])
        assert one[0].tobytes() == ll[r:r + 1].tobytes() and one[1].tobytes() == grad[r:r + 1].tobytes(), r
    cross_ll, cross_grad = _cross(name)
    for b, i in ((0, 0), (B - 1, n - 1), (7, n // 2)):
        single = HistogramBatch(m, case["counts"][b:b + 1], case["tails"][b:b + 1])
        one = single.loglikelihood_gradient_cross(case["points"][i:i + 1])
        single.close()
        assert one[0].tobytes() == cross_ll[b:b + 1, i:i + 1].tobytes(), (b, i)
        assert one[1].tobytes() == np.ascontiguousarray(cross_grad[b:b + 1, i:i + 1]).tobytes(), (b, i)
    batch.close()
    m.close()


def test_a_pairs_list_of_more_than_one_chunk(hip_lib):
    """Basic model, 256 keys: a chunk of the gradient's table holds 2^28 / (3 * 256 * 8) = 43 690 points; a pairs list
    one chunk plus 21 points long.  The 21 points on either side of the cut are the fixture's: within its bounds, and bit
    for bit what the same requests give alone."""
    name = "basic-k256-B5-n21"
    case, g = _rows_match(name)
    assert CHUNK_POINTS_256 == 43690 and g["n"] == 21
    total = CHUNK_POINTS_256 + 21
    rng = np.random.default_rng([S.SEED, 17])
    filler = case["points"][rng.integers(0, g["n"] - 2, total)] * np.array([1.0, 1.0]) * rng.uniform(0.97, 1.03, (total, 2))
    pts = np.ascontiguousarray(filler)
    idx = rng.integers(0, g["B"], total)
    lo = CHUNK_POINTS_256 - 21
    pts[lo:lo + 21] = case["points"]
    pts[lo + 21:lo + 42] = case["points"]
    m, batch = _open(name)
    ll, grad = batch.loglikelihood_gradient_pairs(idx, pts)
    info = batch.info()
    alone = batch.loglikelihood_gradient_pairs(idx[lo:], pts[lo:])
    assert batch.info()["table_chunks"] == 1
    batch.close()
    m.close()
    assert info["table_chunks"] == 2 and info["points_tabled"] == total and info["pairs_requests"] == total
    assert alone[0].tobytes() == ll[lo:].tobytes() and alone[1].tobytes() == grad[lo:].tobytes()
    worst, n = {"ll": 0.0, "g": 0.0}, 0
    for r in range(42):
        n += _check_entry(name, g, case, int(idx[lo + r]), r % 21, ll[lo + r], grad[lo + r], worst)
    assert n >= 40
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(grad))
    print("chunks: %d requests, %d of the fixture's at the cut, worst ll rel %.3g, |dg| / Cg %.3g" % (total, n, worst["ll"], worst["g"]))


def test_the_table_is_shared_and_the_counters(hip_lib):
    """B = 17 histograms at n = 11 points: 11 points are tabled, not 17 x 11 (and not 6 x 11 rows)."""
    from covest_amd import HistogramBatch
    case = S.shape("repeats-k65-B15-n11")
    m, batch = _open("repeats-k65-B15-n11")
    batch.close()
    rng = np.random.default_rng([S.SEED, 19])
    batch = HistogramBatch(m, rng.integers(0, 1000, (17, 65)).astype(np.float64), rng.integers(0, 50, 17).astype(np.float64))
    ll, grad = batch.loglikelihood_gradient_cross(case["points"])
    info = batch.info()
    assert ll.shape == (17, 11) and grad.shape == (17, 11, 5)
    assert info["points_tabled"] == 11 and info["table_chunks"] == 1 and info["pairs_requests"] == 0
    assert info["cross_tiles"] == 2 * ((6 * 11 + 15) // 16) and info["table_ns"] > 0 and info["contraction_ns"] > 0
    batch.loglikelihood_gradient_pairs([3, 16, 0, 3, 9], case["points"][:5])
    info = batch.info()
    assert info["points_tabled"] == 5 and info["pairs_requests"] == 5 and info["cross_tiles"] == 0
    batch.score_table(case["points"][:4])
    assert batch.info()["points_tabled"] == 4
    batch.close()
    m.close()


def test_empty_and_edge_calls(hip_lib):
    from covest_amd import HistogramBatch
    case = S.shape("basic-k63-B15-n21")
    m, batch = _open("basic-k63-B15-n21")
    ll, grad = batch.loglikelihood_gradient_cross(np.empty((0, 2)))
    assert ll.shape == (15, 0) and grad.shape == (15, 0, 2)
    ll, grad = batch.loglikelihood_gradient_pairs([], np.empty((0, 2)))
    assert ll.shape == (0,) and grad.shape == (0, 2)
    log_p, score, tail = batch.score_table(np.empty((0, 2)))
    assert log_p.shape == (0, 63) and score.shape == (0, 2, 63) and tail.shape == (0, 3)
    with pytest.raises(ValueError):
        batch.loglikelihood_gradient_pairs([15], case["points"][:1])  # outside 0 .. 14
    with pytest.raises(ValueError):
        batch.loglikelihood_gradient_pairs([0], case["points"][:2])  # one index per point
    with pytest.raises(ValueError):
        batch.loglikelihood_gradient_pairs([0.5], case["points"][:1])
    empty = HistogramBatch(m, np.empty((0, 63)))
    ll, grad = empty.loglikelihood_gradient_cross(case["points"])
    assert ll.shape == (0, 21) and grad.shape == (0, 21, 2)
    with pytest.raises(ValueError):
        empty.loglikelihood_gradient_pairs([0], case["points"][:1])
    assert empty.score_table(case["points"][:2])[2].tobytes() == batch.score_table(case["points"][:2])[2].tobytes()
    empty.close()
    batch.close()
    for call in (lambda: batch.loglikelihood_gradient_cross(case["points"]), lambda: batch.score_table(case["points"]),
                 lambda: batch.loglikelihood_gradient_pairs([0], case["points"][:1])):
        with pytest.raises(ValueError, match="closed"):
            call()
    m.close()
