"""The closed-form Hessian of a histogram batch on the device (HistogramBatch.loglikelihood_hessian_cross / _pairs,
score_table(order=2)) against the 50-digit restatement of tests/golden/batch_hess.json
(tests/golden/make_golden_batch_hess.py; the shapes are tests/batch_hess_shapes.py's), its value and gradient against
tests/golden/batch_grad.json, the pairs form against the cross form, the own row against K-hess on a twin model, its
conventions (symmetry, the clamp, the dead key, NaN, the tail array, empty calls), two table chunks, and that a result does
not depend on what else is in the call.  The bounds are tests/test_gpu_hessian.py's (tests/parity_helpers.py): 1e-9 C_kl
plus the tail term's first-order slack per entry."""
import functools
import math

import numpy as np
import pytest

import batch_hess_shapes as S
from conftest import load_golden, load_hist, rel_err
from parity_helpers import TOL, _grad_bound, _hess_bound, _model, _tail_delta

pytestmark = pytest.mark.gpu

NAMES = list(S.SHAPES)
TOL_KERNELS = 1e-11  # between the derivative kernel's value and K-direct's (tests/test_gpu_deriv_shapes.py)


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_golden("batch_hess.json")


@functools.lru_cache(maxsize=None)
def _grad_fixture():
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
    """Computed once per shape and shared, never changed: (ll (B, n), grad (B, n, P), hess (B, n, P, P))."""
    if name not in _CROSS:
        m, batch = _open(name)
        _CROSS[name] = batch.loglikelihood_hessian_cross(S.shape(name)["points"])
        batch.close()
        m.close()
    return _CROSS[name]


def _packed(hess):
    """(..., P, P) -> (..., P (P + 1) / 2): the upper triangle, k <= l row by row."""
    k, l = np.triu_indices(hess.shape[-1])
    return hess[..., k, l]


def _entry(ll, grad, hess):
    """The R2 numbers of one (b, i) as the entry points lay them out."""
    return np.concatenate([[ll], grad, _packed(hess)])


def _rows_match(name):
    case, g = S.shape(name), _fixture()["shapes"][name]
    assert np.array_equal(case["points"], np.array(g["points"])) and case["counts"].sum(axis=1).tolist() == g["row_sums"]
    assert case["tails"].tolist() == g["tails"] and g["rows"] == S.stored_rows(name)
    return case, g


def _hess_bounds(g, case, at, b, i):
    """Bound 1 for every packed entry of stored row `at` (histogram b) at point i."""
    delta = _tail_delta(g["n_keys"])
    P = len(g["D"][i])
    out = []
    for k in range(P):
        for l in range(k, P):
            q = len(out)
            out.append(_hess_bound(case["tails"][b], g["sp"][i], g["C"][at][i][q], g["D2"][i][q], g["D"][i][k], g["D"][i][l], delta))
    return np.array(out)


def _check_entry(name, g, case, at, b, i, ll, grad, hess, worst):
    """One stored (b, i) against the two fixtures; returns 1 if its Hessian was compared."""
    what = (name, b, i)
    if [b, i] in g["special"]:
        assert ll == -math.inf and np.all(np.isnan(grad)) and np.all(np.isnan(hess)), (what, ll, grad, hess)
        return 1
    base = _grad_fixture()["shapes"][g["base"]]
    if not any(d[0] == b and d[1] == i for d in base["dropped"]):  # value and gradient: batch_grad.json's, by its bounds
        assert rel_err(float(ll), base["ll"][b][i]) <= TOL, (what, float(ll), base["ll"][b][i])
        delta = _tail_delta(g["n_keys"])
        for k, want in enumerate(base["grad"][b][i]):
            bound = _grad_bound(case["tails"][b], base["sp"][i], base["Cg"][b][i][k], base["D"][i][k], delta)
            assert abs(float(grad[k]) - want) <= bound, (what, k, float(grad[k]), want, bound)
    if any(d[0] == b and d[1] == i for d in g["dropped"]):
        return 0
    got, want, bound = _packed(hess), np.array(g["hess"][at][i]), _hess_bounds(g, case, at, b, i)
    worst["bound"] = max(worst.get("bound", 0.0), float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0))))
    assert np.all(np.abs(got - want) <= bound), (what, got, want, bound)
    C = np.array(g["C"][at][i])
    worst["h"] = max(worst["h"], float(np.max(np.abs(got - want) / np.where(C > 0, C, 1.0))))
    return 1


@pytest.mark.parametrize("name", NAMES)
def test_cross_against_the_fixture(hip_lib, name):
    """Every kept entry of every stored row: |H_kl - want| <= 1e-9 C_kl + s_kl; value and gradient of the same call
    against batch_grad.json; the dead-key entry -inf and NaN.  The number compared is the fixture's kept count."""
    case, g = _rows_match(name)
    ll, grad, hess = _cross(name)
    P = case["points"].shape[1]
    assert ll.shape == (g["B"], g["n"]) and grad.shape == (g["B"], g["n"], P) and hess.shape == (g["B"], g["n"], P, P)
    worst, n = {"h": 0.0}, 0
    for at, b in enumerate(g["rows"]):
        for i in range(g["n"]):
            n += _check_entry(name, g, case, at, b, i, ll[b, i], grad[b, i], hess[b, i], worst)
    assert n == len(g["rows"]) * g["n"] - len(g["dropped"])
    print("%s: %d entries, worst |dH| / C %.3g, worst |dH| / bound %.3g" % (name, n, worst["h"], worst.get("bound", 0.0)))


def test_the_fixture_counts_add_up():
    g = _fixture()
    assert sum(len(r["rows"]) * r["n"] - len(r["dropped"]) for r in g["shapes"].values()) == g["entries"] - g["dropped"]


def _requests(name):
    """Every (b, i) of the shape in a seeded shuffle, the first seven once more at the end."""
    case = S.shape(name)
    cells = [(b, i) for b in range(case["counts"].shape[0]) for i in range(len(case["points"]))]
    order = np.random.default_rng([S.SEED, 23, NAMES.index(name)]).permutation(len(cells))
    cells = [cells[at] for at in order]
    return cells + cells[:7]


@pytest.mark.parametrize("name", NAMES)
def test_pairs_against_cross(hip_lib, name):
    """Every (b, i) as a pairs request: each of the R2 numbers within 4 n_keys 2^-53 of its condition sum
    C = sum_j h_bj |row_j| + tail_b |t|, formed on the host from score_table(order=2): two orders of one sum.  Specials
    exact; the stored rows within the fixture's bounds."""
    case, g = _rows_match(name)
    m, batch = _open(name)
    cells = _requests(name)
    pts = case["points"][[i for _, i in cells]]
    ll, grad, hess = batch.loglikelihood_hessian_pairs([b for b, _ in cells], pts)
    log_p, score, curv, tail = batch.score_table(case["points"], order=2)
    batch.close()
    m.close()
    P = pts.shape[1]
    R2 = S.rows_per_point(case["kind"])
    assert ll.shape == (len(cells),) and grad.shape == (len(cells), P) and hess.shape == (len(cells), P, P)
    assert curv.shape == (g["n"], R2 - 1 - P, g["n_keys"]) and tail.shape == (g["n"], R2)
    assert np.ascontiguousarray(hess.swapaxes(1, 2)).tobytes() == hess.tobytes()
    cross_ll, cross_grad, cross_hess = _cross(name)
    H, tails = case["counts"], case["tails"]
    unit = 4.0 * g["n_keys"] * 2.0 ** -53
    worst_pair, worst = 0.0, {"h": 0.0}
    for at, (b, i) in enumerate(cells):
        got = _entry(ll[at], grad[at], hess[at])
        ref = _entry(cross_ll[b, i], cross_grad[b, i], cross_hess[b, i])
        if b in g["rows"]:
            _check_entry(name, g, case, g["rows"].index(b), b, i, ll[at], grad[at], hess[at], worst)
        if not np.all(np.isfinite(ref)):
            assert np.array_equal(got, ref, equal_nan=True), (name, b, i, got, ref)
            continue
        rows = np.concatenate([log_p[i][None, :], score[i], curv[i]], axis=0)
        C = np.abs(rows) @ H[b] + tails[b] * np.abs(tail[i])
        assert np.all(np.abs(got - ref) <= unit * C), (name, b, i, got, ref, unit * C)
        worst_pair = max(worst_pair, float(np.max(np.abs(got - ref) / np.where(C > 0, C, 1.0))))
    print("%s: %d requests, pairs against cross worst |d| / C %.3g (bound %.3g)" % (name, len(cells), worst_pair, unit))


@pytest.mark.parametrize("name", NAMES)
def test_the_own_row_against_k_hess_and_the_other_tables(hip_lib, name):
    """The own-counts row with the model's own tail: the Hessian within twice bound 1 of loglikelihood_hessian_points, the
    value within 1e-11 relative of loglikelihood_cross, value and gradient the bits of loglikelihood_gradient_cross."""
    case, g = _rows_match(name)
    hist = case["spec"]["hist"]
    m, batch = _open(name)
    ll_m, grad_m, hess_m = m.loglikelihood_hessian_points(case["points"])
    value = batch.loglikelihood_cross(case["points"])
    ll_g, grad_g = batch.loglikelihood_gradient_cross(case["points"])
    batch.close()
    m.close()
    ll, grad, hess = _cross(name)
    b = case["rows"]["own"]
    at = g["rows"].index(b)
    assert case["tails"][b] == case["spec"]["tail"] and case["counts"][b].tolist() == hist["counts"]
    # every row, not the own one alone: the first-order arithmetic is the same expressions at both orders, and the two walks
    # return the same bits on gfx950 (bit equality held, the 1e-11 fall-back was not needed)
    assert ll.tobytes() == ll_g.tobytes() and grad.tobytes() == grad_g.tobytes()
    assert np.array_equal(np.isfinite(ll), np.isfinite(value))
    for a, v in zip(ll.reshape(-1), value.reshape(-1)):
        assert rel_err(float(a), float(v)) <= TOL_KERNELS, (name, float(a), float(v))
    for i in range(g["n"]):
        if not math.isfinite(ll_m[i]):
            assert ll[b, i] == ll_m[i] and np.all(np.isnan(hess[b, i])) and np.all(np.isnan(hess_m[i]))
            continue
        assert rel_err(float(ll[b, i]), float(ll_m[i])) <= TOL_KERNELS, (name, i, ll[b, i], ll_m[i])
        if any(d[0] == b and d[1] == i for d in g["dropped"]):
            continue
        bound = 2 * _hess_bounds(g, case, at, b, i)
        assert np.all(np.abs(_packed(hess[b, i]) - _packed(hess_m[i])) <= bound), (name, i, hess[b, i], hess_m[i], bound)


@pytest.mark.parametrize("name", [n for n in NAMES if "zero_tail1" in S.shape(n)["rows"]])
def test_the_zero_row_with_tail_one_is_the_tail_array(hip_lib, name):
    case = S.shape(name)
    m, batch = _open(name)
    tail = batch.score_table(case["points"], order=2)[3]
    tail1 = batch.score_table(case["points"])[2]
    batch.close()
    m.close()
    ll, grad, hess = _cross(name)
    b = case["rows"]["zero_tail1"]
    P = grad.shape[2]
    got = np.concatenate([ll[b][:, None], grad[b], _packed(hess[b])], axis=1)
    assert got.tobytes() == tail.tobytes()
    assert np.ascontiguousarray(tail[:, :1 + P]).tobytes() == tail1.tobytes()  # (the first-order coefficients: the old table's)
    if "zero_tail0" in case["rows"]:
        z = case["rows"]["zero_tail0"]
        assert not ll[z].any() and not grad[z].any() and not hess[z].any()


@pytest.mark.parametrize("name", NAMES)
def test_results_are_symmetric_to_the_bit(hip_lib, name):
    hess = _cross(name)[2]
    assert np.ascontiguousarray(hess.swapaxes(2, 3)).tobytes() == hess.tobytes()


@pytest.mark.parametrize("name", ["basic-k65-B5-n22", "repeats-k65-B15-n11"])
def test_nan_and_the_clamp(hip_lib, name):
    """A point outside the bounds: the row and the column of each parameter the clamp moved are +0.0, everything else the
    bits of the point ON the bound.  A NaN parameter: the whole entry NaN, and nothing else in the call changes."""
    case, g = _rows_match(name)
    ll, grad, hess = _cross(name)
    n, B = g["n"], g["B"]
    assert any(g["moved"][n - 2]) and any(g["moved"][n - 1]) and not any(any(mv) for mv in g["moved"][:n - 2])
    m, batch = _open(name)
    on_bound = np.array([m.fit_to_bounds([float(v) for v in case["points"][i]]) for i in (n - 2, n - 1)], dtype=np.float64)
    ll_b, grad_b, hess_b = batch.loglikelihood_hessian_cross(on_bound)
    pts = case["points"].copy()
    pts[3, 0 if case["kind"] == "basic" else 4] = math.nan
    ll_n, grad_n, hess_n = batch.loglikelihood_hessian_cross(pts)
    pll_n, pgrad_n, phess_n = batch.loglikelihood_hessian_pairs(np.arange(n) % B, pts)
    batch.close()
    m.close()
    own = case["rows"]["own"]
    for at, i in enumerate((n - 2, n - 1)):
        mv = np.array(g["moved"][i])
        assert ll[:, i].tobytes() == ll_b[:, at].tobytes()
        assert not grad[:, i][:, mv].any() and not np.signbit(grad[:, i][:, mv]).any()
        assert not hess[:, i][:, mv, :].any() and not hess[:, i][:, :, mv].any() and not np.signbit(hess[:, i][:, mv, :]).any()
        keep = ~mv
        assert np.ascontiguousarray(grad[:, i][:, keep]).tobytes() == np.ascontiguousarray(grad_b[:, at][:, keep]).tobytes()
        assert (np.ascontiguousarray(hess[:, i][:, keep][:, :, keep]).tobytes()
                == np.ascontiguousarray(hess_b[:, at][:, keep][:, :, keep]).tobytes())
        assert np.all(hess[own, i][np.ix_(keep, keep)].diagonal() != 0.0)
        assert hess_b[own, at][mv].any()  # (on the bound the parameter is not moved: its row is the derivative's)
    assert np.all(np.isnan(ll_n[:, 3])) and np.all(np.isnan(grad_n[:, 3])) and np.all(np.isnan(hess_n[:, 3]))
    assert math.isnan(pll_n[3]) and np.all(np.isnan(pgrad_n[3])) and np.all(np.isnan(phess_n[3]))
    keep = np.arange(n) != 3
    assert ll_n[:, keep].tobytes() == ll[:, keep].tobytes() and grad_n[:, keep].tobytes() == grad[:, keep].tobytes()
    assert hess_n[:, keep].tobytes() == hess[:, keep].tobytes()
    assert np.all(np.isfinite(pll_n[keep])) and np.all(np.isfinite(phess_n[keep]))


@pytest.mark.parametrize("name", ["basic-dead", "repeats-dead"])
def test_the_dead_key(hip_lib, name):
    """The row that counts the dead key: value -inf and all R2 - 1 other entries NaN, cross and pairs; the row with that
    count zeroed is finite; the table's curvature rows are +0.0 at the dead keys."""
    case, g = _rows_match(name)
    ll, grad, hess = _cross(name)
    rows = case["rows"]
    assert g["special"] == [[rows["dead"], 0]]
    assert ll[rows["dead"], 0] == -math.inf and np.all(np.isnan(grad[rows["dead"], 0])) and np.all(np.isnan(hess[rows["dead"], 0]))
    assert math.isfinite(ll[rows["alive"], 0]) and np.all(np.isfinite(hess[rows["alive"], 0]))
    assert np.all(np.isfinite(ll[:, 1:])) and np.all(np.isfinite(hess[:, 1:]))
    m, batch = _open(name)
    pll, pgrad, phess = batch.loglikelihood_hessian_pairs([rows["dead"], rows["alive"]], case["points"][[0, 0]])
    info = batch.info()
    log_p, score, curv, _ = batch.score_table(case["points"][:1], order=2)
    without = batch.loglikelihood_hessian_cross(case["points"][1:])
    assert batch.info()["dead_points"] == 0
    batch.close()
    m.close()
    assert info["pairs_requests"] == 2 and info["dead_points"] == 2  # (the dead point tabled once a request)
    assert pll[0] == -math.inf and np.all(np.isnan(pgrad[0])) and np.all(np.isnan(phess[0]))
    assert math.isfinite(pll[1]) and np.all(np.isfinite(phess[1]))
    assert without[2].tobytes() == np.ascontiguousarray(hess[:, 1:]).tobytes()  # the finite points: what they are without it
    at = case["spec"]["hist"]["keys"].index(S.ISOLATED)
    dead_keys = np.flatnonzero((log_p[0] == 0.0) & ~np.signbit(log_p[0]))
    assert at in dead_keys and not curv[0][:, dead_keys].any() and not np.signbit(curv[0][:, dead_keys]).any()


def test_empty_and_edge_calls(hip_lib):
    from covest_amd import HistogramBatch
    case = S.shape("basic-k63-B15-n21")
    m, batch = _open("basic-k63-B15-n21")
    ll, grad, hess = batch.loglikelihood_hessian_cross(np.empty((0, 2)))
    assert ll.shape == (15, 0) and grad.shape == (15, 0, 2) and hess.shape == (15, 0, 2, 2)
    ll, grad, hess = batch.loglikelihood_hessian_pairs([], np.empty((0, 2)))
    assert ll.shape == (0,) and grad.shape == (0, 2) and hess.shape == (0, 2, 2)
    log_p, score, curv, tail = batch.score_table(np.empty((0, 2)), order=2)
    assert log_p.shape == (0, 63) and score.shape == (0, 2, 63) and curv.shape == (0, 3, 63) and tail.shape == (0, 6)
    with pytest.raises(ValueError):
        batch.loglikelihood_hessian_pairs([15], case["points"][:1])  # outside 0 .. 14
    empty = HistogramBatch(m, np.empty((0, 63)))
    ll, grad, hess = empty.loglikelihood_hessian_cross(case["points"])
    assert ll.shape == (0, 21) and grad.shape == (0, 21, 2) and hess.shape == (0, 21, 2, 2)
    with pytest.raises(ValueError):
        empty.loglikelihood_hessian_pairs([0], case["points"][:1])
    assert empty.score_table(case["points"][:2], order=2)[3].tobytes() == batch.score_table(case["points"][:2], order=2)[3].tobytes()
    empty.close()
    batch.close()
    with pytest.raises(ValueError, match="closed"):
        batch.loglikelihood_hessian_cross(case["points"])
    m.close()


def test_the_table_is_shared_and_the_counters(hip_lib):
    """B = 17 histograms at n = 4 points of the repeat model: 4 points are tabled (not 17 x 4, not 84 rows), the
    contraction covers 2 x ceil(84 / 16) tiles, and a pairs call counts its requests."""
    from covest_amd import HistogramBatch
    case = S.shape("repeats-k65-B5-n4")
    m, batch = _open("repeats-k65-B5-n4")
    batch.close()
    rng = np.random.default_rng([S.SEED, 29])
    batch = HistogramBatch(m, rng.integers(0, 1000, (17, 65)).astype(np.float64), rng.integers(0, 50, 17).astype(np.float64))
    ll, grad, hess = batch.loglikelihood_hessian_cross(case["points"])
    info = batch.info()
    assert hess.shape == (17, 4, 5, 5)
    assert info["points_tabled"] == 4 and info["table_chunks"] == 1 and info["pairs_requests"] == 0
    assert info["cross_tiles"] == 2 * ((21 * 4 + 15) // 16) and info["table_ns"] > 0 and info["contraction_ns"] > 0
    batch.loglikelihood_hessian_pairs([3, 16, 0], case["points"][:3])
    info = batch.info()
    assert info["points_tabled"] == 3 and info["pairs_requests"] == 3 and info["cross_tiles"] == 0
    batch.close()
    m.close()


@pytest.mark.parametrize("name", ["basic-k63-B15-n21", "repeats-k257-B15-n10"])
def test_a_result_does_not_depend_on_its_company(hip_lib, name):
    """One (b, i) alone -- a batch of one histogram at one point, and one pairs request --, then among 16 and among 65
    others: the same bytes."""
    from covest_amd import HistogramBatch
    case = S.shape(name)
    rng = np.random.default_rng([S.SEED, 31, NAMES.index(name)])
    B, n = case["counts"].shape[0], len(case["points"])
    b0, i0 = 7, n // 2
    m, batch = _open(name)
    single = HistogramBatch(m, case["counts"][b0:b0 + 1], case["tails"][b0:b0 + 1])
    alone = single.loglikelihood_hessian_cross(case["points"][i0:i0 + 1])
    single.close()
    alone_pair = batch.loglikelihood_hessian_pairs([b0], case["points"][i0:i0 + 1])
    batch.close()
    for others, at_b, at_i in ((16, 5, 11), (65, 64, 65)):
        rows = rng.integers(0, B, others + 1)
        at = rng.integers(0, n, others + 1)
        rows[at_b], at[at_i] = b0, i0
        company = HistogramBatch(m, case["counts"][rows], case["tails"][rows])
        got = company.loglikelihood_hessian_cross(case["points"][at])
        idx = rng.integers(0, others + 1, others + 1)
        idx[at_i] = at_b
        pair = company.loglikelihood_hessian_pairs(idx, case["points"][at])
        company.close()
        for a, c, p, q in zip(alone, got, alone_pair, pair):
            assert np.ascontiguousarray(c[at_b, at_i]).tobytes() == np.ascontiguousarray(a[0, 0]).tobytes(), (name, others)
            assert np.ascontiguousarray(q[at_i]).tobytes() == np.ascontiguousarray(p[0]).tobytes(), (name, others)
    m.close()


# ---------------------------------------------------------------------------------------------- two table chunks
# (the shape of tests/test_gpu_batch_chunks.py: the basic model on 256 keys of H256, lists of filler around a few points of
# interest either side of the cut, every expected value the SAME call on the short list of those points alone)
K, R, MAX_ERROR, N_KEYS = 21, 100, 8, 256
FILLER = [300.0, 0.3]
DEAD_POINT = [0.5, 0.02]  # coverage 0.5: p underflows to 0 at the upper keys
PER_HESS = (1 << 28) // (6 * N_KEYS * 8)  # 21845 points a chunk at R2 = 6 rows a point
INSIDE = np.array([[380.0, 0.0020], [400.0, 0.0030], [420.0, 0.0010], [440.0, 0.0025], [460.0, 0.0015]])
_CHUNK_MODEL = []


def _chunk_model(hip_lib):
    if not _CHUNK_MODEL:
        from covest_amd import BasicModel
        hist = load_hist("H256")
        keys = list(hist)[:N_KEYS]
        _CHUNK_MODEL.append(BasicModel(K, R, (keys, [hist[j] for j in keys]), 0, max_error=MAX_ERROR))
    return _CHUNK_MODEL[0]


@pytest.fixture(scope="module", autouse=True)
def _close_chunk_model():
    yield
    for m in _CHUNK_MODEL:
        m.close()  # (and its batches)
    _CHUNK_MODEL.clear()


def _histograms(B, seed):
    rng = np.random.default_rng([20250601, seed])
    counts = rng.integers(0, 10 ** 6 + 1, size=(B, N_KEYS)).astype(np.float64)
    counts[rng.random((B, N_KEYS)) < 1.0 / 3.0] = 0.0
    tails = np.where(np.arange(B) % 2 == 1, rng.integers(1, 10 ** 5, size=B), 0).astype(np.float64)
    return counts, tails


def test_hessian_cross_over_two_chunks(hip_lib):
    """A dead-key point in the SECOND chunk: the dead list's entry i R2 of a chunk with first > 0, the fix-up and the
    specials pass on rows of length nc R2, and the read-back into rows of length n R2.  B = 17: a second histogram tile
    with one row in it."""
    from covest_amd import HistogramBatch
    n, B = PER_HESS + 21, 17
    at = np.array([PER_HESS - 1, PER_HESS, n - 1, PER_HESS + 10])  # chunk 1's last, chunk 2's first and last, the dead point
    counts, tails = _histograms(B, 2)
    probe = HistogramBatch(_chunk_model(hip_lib), counts[:1])
    log_p = probe.score_table([DEAD_POINT], order=2)[0]
    probe.close()
    dead = np.flatnonzero((log_p[0] == 0.0) & ~np.signbit(log_p[0]))
    assert len(dead), "coverage 0.5 must underflow at the upper keys"
    alive_row, dead_row = 2, 16  # (the dead row alone in the second tile)
    counts[alive_row, dead] = 0.0
    counts[dead_row] = counts[alive_row]
    counts[dead_row, dead[len(dead) // 2]] = 12345.0
    batch = HistogramBatch(_chunk_model(hip_lib), counts, tails)
    pts = np.tile(np.array([FILLER]), (n, 1))
    pts[at[:3]], pts[at[3]] = INSIDE[:3], DEAD_POINT
    ll, grad, hess = batch.loglikelihood_hessian_cross(pts)
    info = batch.info()
    assert ll.shape == (B, n) and grad.shape == (B, n, 2) and hess.shape == (B, n, 2, 2)
    assert info["table_chunks"] == 2 and info["points_tabled"] == n and info["dead_points"] >= 1
    want = batch.loglikelihood_hessian_cross(pts[at])
    assert batch.info()["table_chunks"] == 1
    assert want[0][dead_row, 3] == -math.inf and np.all(np.isnan(want[1][dead_row, 3])) and np.all(np.isnan(want[2][dead_row, 3]))
    assert math.isfinite(want[0][alive_row, 3]) and np.all(np.isfinite(want[2][alive_row, 3]))
    assert np.all(np.isfinite(want[0][:, :3])) and np.all(np.isfinite(want[2][:, :3])) and want[2][:, :3].all()
    for got, ref in zip((ll, grad, hess), want):
        assert np.array_equal(got[:, at], ref, equal_nan=True)
    filler = batch.loglikelihood_hessian_cross([FILLER])
    for got, ref in zip((ll, grad, hess), filler):  # ... and the filler, everywhere
        rest = np.delete(got, at, axis=1)
        assert np.array_equal(rest, np.broadcast_to(ref, rest.shape), equal_nan=True)
    batch.close()


def test_hessian_pairs_over_two_chunks(hip_lib):
    """The request's histogram number is index[first + i] for point i of the chunk that begins at `first`."""
    from covest_amd import HistogramBatch
    n = PER_HESS + 40
    at = np.array([3, 77, PER_HESS - 1, PER_HESS, PER_HESS + 39])
    counts, tails = _histograms(6, 1)
    batch = HistogramBatch(_chunk_model(hip_lib), counts, tails)
    pts = np.tile(np.array([FILLER]), (n, 1))
    index = np.zeros(n, dtype=np.int64)
    pts[at], index[at] = INSIDE, [1, 2, 3, 4, 5]
    got = batch.loglikelihood_hessian_pairs(index, pts)
    info = batch.info()
    assert info["table_chunks"] == 2 and info["points_tabled"] == info["pairs_requests"] == n and info["cross_tiles"] == 0
    short = np.concatenate([at, [0, n - 2]])  # ... and a filler request of either chunk
    want = batch.loglikelihood_hessian_pairs(index[short], pts[short])
    assert batch.info()["table_chunks"] == 1
    assert np.all(np.isfinite(want[2][:5])) and len({v.tobytes() for v in want[2][:5]}) == 5
    for g, w in zip(got, want):
        assert np.array_equal(g[short], w, equal_nan=True)
        rest = g[index == 0]
        assert np.array_equal(rest, np.broadcast_to(w[5], rest.shape), equal_nan=True)
    batch.close()


def test_score_table2_over_two_chunks(hip_lib):
    """Rows and tail coefficients of the points either side of the cut.  The whole table is 268 MB on the host: one array,
    filled by the entry point itself (the method would copy it apart), and dropped."""
    from covest_amd import HistogramBatch, _capi
    n = PER_HESS + 21
    at = np.array([PER_HESS - 1, PER_HESS, n - 1, PER_HESS + 10])
    batch = HistogramBatch(_chunk_model(hip_lib), np.zeros((1, N_KEYS)))
    pts = np.tile(np.array([FILLER]), (n, 1))
    pts[at[:3]], pts[at[3]] = INSIDE[:3], DEAD_POINT
    rows = np.empty((n, 6, N_KEYS), dtype=np.float64)
    tail = np.empty((n, 6), dtype=np.float64)
    _capi.check(_capi.lib().covest_batch_score_table2(batch._open(), n, pts.ctypes.data, rows.ctypes.data, tail.ctypes.data),
                "covest_batch_score_table2")
    info = batch.info()
    got_rows, got_tail = rows[at].copy(), tail[at].copy()
    del rows
    assert info["table_chunks"] == 2 and info["points_tabled"] == n and info["contraction_ns"] == 0
    log_p, score, curv, want_tail = batch.score_table(pts[at], order=2)
    assert np.array_equal(got_rows[:, 0, :], log_p, equal_nan=True) and np.array_equal(got_rows[:, 1:3, :], score, equal_nan=True)
    assert np.array_equal(got_rows[:, 3:, :], curv, equal_nan=True) and np.array_equal(got_tail, want_tail, equal_nan=True)
    assert np.array_equal(np.signbit(got_rows), np.signbit(np.concatenate([log_p[:, None, :], score, curv], axis=1)))
    assert len(np.unique(got_tail[:3, 3])) == 3 and np.any((log_p[3] == 0.0) & ~np.signbit(log_p[3]))
    batch.close()


FORMS = {  # name -> (the call on (batch, index, points), does it contract)
    "hessian_cross": (lambda b, idx, pts: b.loglikelihood_hessian_cross(pts), True),
    "hessian_pairs": (lambda b, idx, pts: b.loglikelihood_hessian_pairs(idx, pts), True),
    "score_table2": (lambda b, idx, pts: b.score_table(pts, order=2), False),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_time_fields_after_each_new_form(hip_lib, form):
    """table_ns covers the order-2 table's kernels; contraction_ns the kernels of the two forms that contract, and is 0
    after the table alone, whatever the call before it left."""
    from covest_amd import HistogramBatch
    counts, tails = _histograms(3, 3)
    batch = HistogramBatch(_chunk_model(hip_lib), counts, tails)
    index = np.array([0, 2, 1, 1, 0])
    batch.loglikelihood_cross(INSIDE)  # (a contraction before the form under test)
    assert batch.info()["contraction_ns"] > 0
    call, contracts = FORMS[form]
    call(batch, index, INSIDE)
    info = batch.info()
    assert info["points_tabled"] == 5 and info["table_chunks"] == 1 and info["table_ns"] > 0
    assert (info["contraction_ns"] > 0) if contracts else (info["contraction_ns"] == 0)
    assert info["pairs_requests"] == (5 if form == "hessian_pairs" else 0)
    batch.close()
