"""Histogram batches: the places the one walk over table chunks (abi_batch.cpp walk_chunks) makes
reachable for every form -- a pairs call, a gradient cross call and the score table over TWO chunks -- and the time
fields of covest_batch_info after each form.

The table budget is a constant of the build (256 MiB), so the lists are long enough for two chunks of the basic model on
256 keys: 131072 points a chunk at one row a point, 43690 at three.  Every list is filler ([300.0, 0.3], as in
test_gpu_batch.py::test_argmin_carries_the_minimum_across_table_chunks) around a few points of interest either side of
the cut, and every expected value is the SAME call on the short list of those points alone: chunking changes no value and
a result does not depend on what else is in the call (include/covest_amd.h), so the comparison is np.array_equal."""
import functools
import math

import numpy as np
import pytest

from conftest import load_hist

pytestmark = pytest.mark.gpu

K, R, MAX_ERROR = 21, 100, 8
N_KEYS = 256
FILLER = [300.0, 0.3]
DEAD_POINT = [0.5, 0.02]  # coverage 0.5: p underflows to 0 at the upper keys (tests/test_gpu_batch.py)
PER_VALUE = (1 << 28) // (N_KEYS * 8)     # 131072 points a chunk of the value table
PER_GRAD = (1 << 28) // (3 * N_KEYS * 8)  # 43690 of the gradient's, P + 1 = 3 rows a point
# distinct, in bounds; the error-free class's rate lies beyond the largest key, so that 1 - sum p_j is far from 0 and the
# tail coefficients are not all 0
INSIDE = np.array([[380.0, 0.0020], [400.0, 0.0030], [420.0, 0.0010], [440.0, 0.0025], [460.0, 0.0015]])


@functools.lru_cache(maxsize=None)
def _keys():
    hist = load_hist("H256")
    keys = list(hist)[:N_KEYS]
    return keys, [hist[j] for j in keys]


_MODEL = []


def _model(hip_lib):
    if not _MODEL:
        from covest_amd import BasicModel
        _MODEL.append(BasicModel(K, R, _keys(), 0, max_error=MAX_ERROR))
    return _MODEL[0]


@pytest.fixture(scope="module", autouse=True)
def _close_model():
    yield
    for m in _MODEL:
        m.close()  # (and its batches)
    _MODEL.clear()


def _histograms(B, seed):
    rng = np.random.default_rng([20250601, seed])
    counts = rng.integers(0, 10 ** 6 + 1, size=(B, N_KEYS)).astype(np.float64)
    counts[rng.random((B, N_KEYS)) < 1.0 / 3.0] = 0.0
    tails = np.where(np.arange(B) % 2 == 1, rng.integers(1, 10 ** 5, size=B), 0).astype(np.float64)
    return counts, tails


def _dead_keys(batch):
    """The keys the derivative kernel's table marks dead at DEAD_POINT: +0.0 in the value row and nowhere else."""
    log_p, _, _ = batch.score_table([DEAD_POINT])
    dead = np.flatnonzero((log_p[0] == 0.0) & ~np.signbit(log_p[0]))
    assert len(dead), "coverage 0.5 must underflow at the upper keys"
    return dead


def test_value_pairs_over_two_chunks(hip_lib):
    """The request's histogram number is index[first + i] for point i of the chunk that begins at `first`."""
    from covest_amd import HistogramBatch
    n = PER_VALUE + 40
    at = np.array([3, 77, PER_VALUE - 1, PER_VALUE, PER_VALUE + 39])  # two in the first chunk, its last, the second's ends
    counts, tails = _histograms(6, 1)
    batch = HistogramBatch(_model(hip_lib), counts, tails)
    pts = np.tile(np.array([FILLER]), (n, 1))
    index = np.zeros(n, dtype=np.int64)
    pts[at], index[at] = INSIDE, [1, 2, 3, 4, 5]
    got = batch.loglikelihood_pairs(index, pts)
    info = batch.info()
    assert info["table_chunks"] == 2 and info["points_tabled"] == info["pairs_requests"] == n and info["cross_tiles"] == 0
    short = np.concatenate([at, [0, n - 2]])  # ... and a filler request of either chunk
    want = batch.loglikelihood_pairs(index[short], pts[short])
    assert batch.info()["table_chunks"] == 1
    assert np.all(np.isfinite(want[:5])) and len(set(want[:5].tolist())) == 5
    assert np.array_equal(got[short], want, equal_nan=True)
    assert np.array_equal(got[np.flatnonzero(index == 0)], np.full(n - 5, want[5]), equal_nan=True)  # the filler, everywhere
    batch.close()


def test_gradient_cross_over_two_chunks(hip_lib):
    """A dead-key point in the SECOND chunk: the dead list's entry i R of a chunk with first > 0, the fix-up and the
    specials pass on rows of length nc R, and the read-back into rows of length n R.  B = 17: a second histogram tile
    with one row in it."""
    from covest_amd import HistogramBatch
    n, B = PER_GRAD + 21, 17
    at = np.array([PER_GRAD - 1, PER_GRAD, n - 1, PER_GRAD + 10])  # chunk 1's last, chunk 2's first and last, the dead point
    counts, tails = _histograms(B, 2)
    probe = HistogramBatch(_model(hip_lib), counts[:1])
    dead = _dead_keys(probe)
    probe.close()
    alive_row, dead_row = 2, 16  # (the dead row alone in the second tile)
    counts[alive_row, dead] = 0.0
    counts[dead_row] = counts[alive_row]
    counts[dead_row, dead[len(dead) // 2]] = 12345.0
    batch = HistogramBatch(_model(hip_lib), counts, tails)
    pts = np.tile(np.array([FILLER]), (n, 1))
    pts[at[:3]], pts[at[3]] = INSIDE[:3], DEAD_POINT
    ll, grad = batch.loglikelihood_gradient_cross(pts)
    info = batch.info()
    assert ll.shape == (B, n) and grad.shape == (B, n, 2)
    assert info["table_chunks"] == 2 and info["points_tabled"] == n and info["dead_points"] >= 1
    want_ll, want_grad = batch.loglikelihood_gradient_cross(pts[at])
    assert batch.info()["table_chunks"] == 1
    assert want_ll[dead_row, 3] == -math.inf and np.all(np.isnan(want_grad[dead_row, 3]))
    assert math.isfinite(want_ll[alive_row, 3]) and np.all(np.isfinite(want_grad[alive_row, 3]))
    assert np.all(np.isfinite(want_ll[:, :3])) and np.all(np.isfinite(want_grad[:, :3]))
    assert np.array_equal(ll[:, at], want_ll, equal_nan=True)
    assert np.array_equal(grad[:, at], want_grad, equal_nan=True)
    batch.close()


def test_score_table_over_two_chunks(hip_lib):
    """Rows and tail coefficients of the points either side of the cut.  The whole table is 268 MB on the host: one
    array, filled by the entry point itself (the method would copy it apart), and dropped."""
    from covest_amd import HistogramBatch, _capi
    n = PER_GRAD + 21
    at = np.array([PER_GRAD - 1, PER_GRAD, n - 1, PER_GRAD + 10])
    batch = HistogramBatch(_model(hip_lib), np.zeros((1, N_KEYS)))
    pts = np.tile(np.array([FILLER]), (n, 1))
    pts[at[:3]], pts[at[3]] = INSIDE[:3], DEAD_POINT
    rows = np.empty((n, 3, N_KEYS), dtype=np.float64)
    tail = np.empty((n, 3), dtype=np.float64)
    _capi.check(_capi.lib().covest_batch_score_table(batch._open(), n, pts.ctypes.data, rows.ctypes.data, tail.ctypes.data),
                "covest_batch_score_table")
    info = batch.info()
    got_rows, got_tail = rows[at].copy(), tail[at].copy()
    del rows
    assert info["table_chunks"] == 2 and info["points_tabled"] == n and info["contraction_ns"] == 0
    log_p, score, want_tail = batch.score_table(pts[at])
    assert np.array_equal(got_rows[:, 0, :], log_p, equal_nan=True) and np.array_equal(got_rows[:, 1:, :], score, equal_nan=True)
    assert np.array_equal(got_tail, want_tail, equal_nan=True)
    assert np.array_equal(np.signbit(got_rows[:, 0, :]), np.signbit(log_p))  # (+0.0 marks a dead key, -0.0 is p = 1)
    assert len(np.unique(got_tail[:3, 0])) == 3 and np.any((log_p[3] == 0.0) & ~np.signbit(log_p[3]))
    batch.close()


FORMS = {  # name -> (the call on (batch, index, points), does it contract)
    "cross": (lambda b, idx, pts: b.loglikelihood_cross(pts), True),
    "pairs": (lambda b, idx, pts: b.loglikelihood_pairs(idx, pts), True),
    "argmin_cross": (lambda b, idx, pts: b.argmin_cross(pts), True),
    "gradient_cross": (lambda b, idx, pts: b.loglikelihood_gradient_cross(pts), True),
    "gradient_pairs": (lambda b, idx, pts: b.loglikelihood_gradient_pairs(idx, pts), True),
    "score_table": (lambda b, idx, pts: b.score_table(pts), False),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_time_fields_after_each_form(hip_lib, form):
    """table_ns covers every form's table kernels; contraction_ns the kernels of every form that contracts -- the value
    pairs form included -- and is 0 after the score table, which contracts nothing, whatever the call before it left."""
    from covest_amd import HistogramBatch
    counts, tails = _histograms(3, 3)
    batch = HistogramBatch(_model(hip_lib), counts, tails)
    index = np.array([0, 2, 1, 1, 0])
    batch.loglikelihood_cross(INSIDE)  # (a contraction before the form under test)
    assert batch.info()["contraction_ns"] > 0
    call, contracts = FORMS[form]
    call(batch, index, INSIDE)
    info = batch.info()
    assert info["points_tabled"] == 5 and info["table_chunks"] == 1
    assert info["table_ns"] > 0
    assert (info["contraction_ns"] > 0) if contracts else (info["contraction_ns"] == 0)
    batch.close()
