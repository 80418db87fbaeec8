"""Histogram batches on the device (covest_amd.batch): every histogram of a batch at every point
of a list (cross), histogram b_i at point i (pairs), the per-histogram arg-min, the draw of replicates into a batch --
against the oracle, against the existing device path (a twin model per histogram through K-direct), and against the
public probabilities.

The shapes are the smallest that cross every edge of the contraction's 16 x 16 x 4 tile, of its loop over 16 keys and
of a wave's 64 points: n_keys in {1, 3, 4, 5, 63, 64, 65, 256}, B in {1, 15, 16, 17, 33}, n in {1, 15, 16, 17, 35}, a
covering subset of the product in which every value of each axis appears with both models.

Points: a seeded draw inside the bounds.  The coverage is drawn so that the rate of the error-free class lies between
1.0 and 1.6 times the largest key, and from 63 keys on the error rate stays below 0.004 -- at a high coverage every
error class saturates and the classes' weights go with comb(k, s) 3^s, which leaves the error-free class a thousandth --
so that mass beyond the keys keeps 1 - sum p_j away from 0, where the tail term is ill-conditioned (the checks against
the oracle and the public probabilities leave out points with 1 - sum p_j < 1e-3, and assert that at most a quarter of
the sampled tail entries go that way).  Two points per model lie outside the
bounds (the clamp), and the 256-key shapes carry one point of coverage 0.5, where p_j underflows to 0 at the upper
keys (the dead-key rule)."""
import functools
import math

import numpy as np
import pytest

from conftest import load_hist, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9           # the project's bound against the oracle (IEEE specials exact)
TOL_KERNELS = 1e-10  # between two kernels of the library
SEED = 20240815
K, R, MAX_ERROR = 21, 100, 8
DEAD_POINT = {"basic": [0.5, 0.02], "repeats": [0.5, 0.02, 0.6, 0.5, 0.8]}
# (model, n_keys, B, n): every value of each axis with both models; the B = 33, n = 35 shapes serve the sharing check
SHAPES = [("basic", 1, 1, 1), ("basic", 3, 15, 17), ("basic", 4, 16, 15), ("basic", 5, 17, 16), ("basic", 63, 33, 35),
          ("basic", 64, 16, 17), ("basic", 65, 17, 35), ("basic", 256, 33, 35),
          ("repeats", 1, 16, 15), ("repeats", 3, 1, 16), ("repeats", 4, 17, 1), ("repeats", 5, 15, 35),
          ("repeats", 63, 33, 35), ("repeats", 64, 17, 17), ("repeats", 65, 15, 16), ("repeats", 256, 16, 17)]
SHAPE_IDS = ["%s-k%d-B%d-n%d" % s for s in SHAPES]


def _golden_keys(n_keys):
    hist = load_hist("H256")
    keys = list(hist)[:n_keys]
    return keys, [hist[j] for j in keys]


def _points(kind, n_keys, n, rng):
    """n points inside the bounds; from 15 points on the last two lie outside them (basic: coverage below its lower
    bound, error rate below 0; repeats: q1 below its lower bound, error rate below 0 with q above 1), and the 256-key
    shapes carry the dead-key point at index 1."""
    e = rng.uniform(0.005, 0.08, n) if n_keys <= 5 else rng.uniform(0.0005, 0.004, n)
    rate = rng.uniform(1.0, 1.6, n) * max(n_keys, 4)
    c = rate / ((R - K + 1) / R * (1.0 - e) ** K)
    cols = [c, e]
    if kind == "repeats":
        cols += [rng.uniform(0.4, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.6, 0.95, n)]
    pts = np.stack(cols, axis=1)
    if n >= 15:
        if kind == "basic":
            pts[n - 2, 0] = 0.001  # (clamped to 0.01: nearly all mass on key 1, so 1 - sum p_j is tiny there)
            pts[n - 1, 1] = -0.1
        else:
            pts[n - 2, 2] = 0.1
            pts[n - 1, 1], pts[n - 1, 4] = -0.05, 1.5
    if n_keys == 256:
        pts[1] = DEAD_POINT[kind]
    return pts


@functools.lru_cache(maxsize=None)
def _case(kind, n_keys, B, n):
    """The model's histogram, the batch's histograms and tails, and the points of one shape (seeded; nothing here
    needs a device or the oracle)."""
    rng = np.random.default_rng([SEED, 0 if kind == "basic" else 1, n_keys, B, n])
    keys, own = _golden_keys(n_keys)
    model_tail = 1000 if (n_keys + B) % 2 else 0
    counts = rng.integers(0, 10 ** 6 + 1, size=(B, n_keys)).astype(np.float64)
    counts[rng.random((B, n_keys)) < 1.0 / 3.0] = 0.0
    tails = np.where(np.arange(B) % 2 == 1, rng.integers(1, 10 ** 5, size=B), 0).astype(np.float64)
    rows = {"zero": 0}
    counts[0] = 0.0
    if B >= 2:
        rows["own"] = 1
        counts[1] = own
    return {"kind": kind, "keys": keys, "own": own, "model_tail": model_tail, "counts": counts, "tails": tails,
            "rows": rows, "points": _points(kind, n_keys, n, rng), "dead_at": 1 if n_keys == 256 else None}


def _oracle_model(oracle, case, counts, tail):
    hist = {j: (int(v) if float(v).is_integer() else float(v)) for j, v in zip(case["keys"], counts)}
    return oracle.OracleModel(case["kind"], K, R, hist, tail, max_error=MAX_ERROR)


_REFERENCE = {}


def _reference(oracle, shape):
    """Computed once per shape and shared: the case with its dead-key rows set (they need the oracle's probabilities),
    1 - sum p_j per point, and the oracle's log-likelihood at a seeded sample of (b, i) -- at least 64 entries (all
    where the shape has fewer), with every entry of the zero row, the own-counts row, the dead-key point and its two
    rows."""
    if shape in _REFERENCE:
        return _REFERENCE[shape]
    kind, n_keys, B, n = shape
    case = dict(_case(*shape))
    counts, tails, pts = case["counts"].copy(), case["tails"].copy(), case["points"]
    rows = dict(case["rows"])
    probe = _oracle_model(oracle, case, counts[0], 0)
    probs = [probe.compute_probabilities(*p) for p in pts]
    rest = np.array([1.0 - math.fsum(p.values()) for p in probs])
    if case["dead_at"] is not None:
        p_dead = probs[case["dead_at"]]
        dead_keys = [at for at, j in enumerate(case["keys"]) if p_dead[j] == 0.0]
        assert dead_keys, "coverage 0.5 must underflow at the upper keys"
        assert all(probs[i][j] > 0.0 for i in range(n) if i != case["dead_at"] and i < n - 2 for j in case["keys"])
        rows["alive"], rows["dead"] = 2, 3  # a histogram without a count on a dead key, and its twin with one
        counts[2, dead_keys] = 0.0
        counts[3] = counts[2]
        counts[3, dead_keys[len(dead_keys) // 2]] = 12345.0
        tails[2] = tails[3]  # (an odd row: positive)
    rng = np.random.default_rng([SEED, 7, n_keys, B, n])
    sample = {(b, i) for b in rows.values() for i in range(n)}
    if case["dead_at"] is not None:
        sample |= {(b, case["dead_at"]) for b in range(B)}
    cells = [(b, i) for b in range(B) for i in range(n)]
    extra = [cells[at] for at in rng.permutation(len(cells))]
    for cell in extra:
        if len(sample) >= min(64 + len(rows) * n, len(cells)):
            break
        sample.add(cell)
    want = {}
    for b in sorted({b for b, _ in sample}):
        idx = sorted(i for bb, i in sample if bb == b)
        values = _oracle_model(oracle, case, counts[b], tails[b]).compute_loglikelihood_many(pts[idx], n_threads=8)
        want.update({(b, i): float(v) for i, v in zip(idx, values)})
    case.update(counts=counts, tails=tails, rows=rows, rest=rest, want=want)
    _REFERENCE[shape] = case
    return case


_DEVICE = {}


def _device(hip_lib, oracle, shape):
    """The model, the batch and its cross result for one shape, computed once; the models stay open for the module."""
    if shape not in _DEVICE:
        from covest_amd import BasicModel, HistogramBatch, RepeatsModel
        case = _reference(oracle, shape)
        cls = BasicModel if case["kind"] == "basic" else RepeatsModel
        model = cls(K, R, (case["keys"], case["own"]), case["model_tail"], max_error=MAX_ERROR)
        batch = HistogramBatch(model, case["counts"], case["tails"])
        cross = batch.loglikelihood_cross(case["points"])
        _DEVICE[shape] = (model, batch, cross, batch.info())
    return _DEVICE[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for model, batch, _, _ in _DEVICE.values():
        batch.close()
        model.close()
    _DEVICE.clear()


def _twin(model, case, counts, tail):
    from covest_amd.bootstrap import _replicate_model
    return _replicate_model(model, case["keys"], counts, tail)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cross_against_the_oracle(hip_lib, oracle, shape):
    case = _reference(oracle, shape)
    _, batch, cross, _ = _device(hip_lib, oracle, shape)
    B, n = shape[2], shape[3]
    assert cross.shape == (B, n) and len(batch) == B
    assert len(case["want"]) >= min(64, B * n)
    worst, tail_entries, left_out = 0.0, 0, 0
    for (b, i), want in sorted(case["want"].items()):
        if case["tails"][b] != 0:
            tail_entries += 1
            if case["rest"][i] < 1e-3:  # the tail term is ill-conditioned where 1 - sum p_j is tiny
                left_out += 1
                continue
        err = rel_err(float(cross[b, i]), want)
        worst = max(worst, err)
        assert err <= TOL, (shape, b, i, float(cross[b, i]), want)
    print("%s: %d entries, worst relative error %.3g, %d of %d tail entries left out"
          % (SHAPE_IDS[SHAPES.index(shape)], len(case["want"]), worst, left_out, tail_entries))
    assert left_out * 4 <= tail_entries
    assert all(cross[case["rows"]["zero"], i] == 0.0 for i in range(n))  # no counts, no tail: exactly 0
    if case["dead_at"] is not None:
        at = case["dead_at"]
        assert cross[case["rows"]["dead"], at] == -math.inf and case["want"][(case["rows"]["dead"], at)] == -math.inf
        assert math.isfinite(cross[case["rows"]["alive"], at]) and math.isfinite(case["want"][(case["rows"]["alive"], at)])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_cross_against_a_twin_model_through_k_direct(hip_lib, oracle, shape):
    case = _reference(oracle, shape)
    model, _, cross, _ = _device(hip_lib, oracle, shape)
    B = shape[2]
    chosen = sorted({min(1, B - 1), B // 2, B - 1})  # the own-counts row among them
    if "dead" in case["rows"]:
        chosen = [case["rows"]["dead"], case["rows"]["alive"], B - 1]
    for b in chosen:
        twin = _twin(model, case, case["counts"][b], case["tails"][b])
        try:
            want = twin.loglikelihood_points(case["points"], kernel="direct")
        finally:
            twin.close()
        for i, (g, w) in enumerate(zip(cross[b], want)):
            assert rel_err(float(g), float(w)) <= TOL_KERNELS, (shape, b, i, float(g), float(w))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] in (5, 65, 256)],
                         ids=[i for s, i in zip(SHAPES, SHAPE_IDS) if s[1] in (5, 65, 256)])
def test_table_row_against_the_public_probabilities(hip_lib, oracle, shape):
    """counts 0 and tail 1: the cross result IS log(1 - sp), the table's own tail term, and sp the sum of what
    compute_probabilities(clamp=True) returns."""
    from covest_amd import HistogramBatch
    case = _reference(oracle, shape)
    model, _, _, _ = _device(hip_lib, oracle, shape)
    pts = case["points"]
    batch = HistogramBatch(model, np.zeros((1, shape[1])), [1.0])
    got = batch.loglikelihood_cross(pts)
    batch.close()
    assert got.shape == (1, len(pts))
    compared = 0
    for i, p in enumerate(pts):
        sp = math.fsum(model.compute_probabilities(*p, clamp=True).values())
        if 1.0 - sp < 1e-3:
            continue
        compared += 1
        assert rel_err(float(got[0, i]), math.log(1.0 - sp)) <= 1e-12, (shape, i, float(got[0, i]), sp)
    assert compared * 4 >= 3 * len(pts) or len(pts) < 4


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("shape", [("basic", 65, 17, 35), ("repeats", 64, 17, 17), ("basic", 256, 33, 35)],
                         ids=["basic-k65", "repeats-k64", "basic-k256"])
def test_pairs_equal_the_cross_entries(hip_lib, oracle, shape, n):
    """The pairs kernel adds a row's products lane by lane and by wave shuffles, the cross contraction inside the MFMA
    in the order of its key permutation: two orders of one sum of like-signed terms, so 1e-13 relative, not the bits.
    Specials (the dead-key rule) are exact."""
    case = _reference(oracle, shape)
    _, batch, cross, _ = _device(hip_lib, oracle, shape)
    B, n_pts = shape[2], shape[3]
    rng = np.random.default_rng([SEED, 11, n])
    at = rng.integers(0, n_pts, size=n)               # points repeat
    index = rng.permutation(np.arange(n) % B)         # a permuted index with repeated histograms
    if case["dead_at"] is not None and n > 3:
        at[:2] = case["dead_at"]
        index[0], index[1] = case["rows"]["dead"], case["rows"]["alive"]
    got = batch.loglikelihood_pairs(index, case["points"][at])
    info = batch.info()
    assert got.shape == (n,) and info["pairs_requests"] == n and info["points_tabled"] == n and info["cross_tiles"] == 0
    for i in range(n):
        assert rel_err(float(got[i]), float(cross[index[i], at[i]])) <= 1e-13, (shape, n, i)
    if case["dead_at"] is not None and n > 3:
        assert got[0] == -math.inf and math.isfinite(got[1])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_argmin_per_histogram(hip_lib, oracle, shape):
    case = _reference(oracle, shape)
    _, batch, cross, _ = _device(hip_lib, oracle, shape)
    best, arg = batch.argmin_cross(case["points"])
    assert best.shape == arg.shape == (shape[2],) and arg.dtype == np.int64
    for b in range(shape[2]):
        want_arg, want_best = oracle.first_min(-cross[b])
        assert (int(arg[b]), float(best[b])) == (want_arg, want_best), (shape, b)
    # every point twice, bit-equal: the first of two equal minima wins
    twice = np.concatenate([case["points"], case["points"]])
    best2, arg2 = batch.argmin_cross(twice)
    assert np.array_equal(arg2, arg) and np.array_equal(best2, best)


def test_argmin_of_a_row_that_is_nowhere_finite(hip_lib, oracle):
    from covest_amd import HistogramBatch
    shape = ("basic", 256, 33, 35)
    case = _reference(oracle, shape)
    model, _, _, _ = _device(hip_lib, oracle, shape)
    counts = np.zeros((2, 256))
    counts[0, 255] = 7.0  # a count on key 256, where p underflows at both points
    counts[1, 0] = 7.0
    batch = HistogramBatch(model, counts)
    pts = np.array([[0.5, 0.02], [0.4, 0.03]])
    cross = batch.loglikelihood_cross(pts)
    best, arg = batch.argmin_cross(pts)
    batch.close()
    assert np.all(cross[0] == -math.inf) and np.all(np.isfinite(cross[1]))
    assert (int(arg[0]), float(best[0])) == (-1, math.inf) == oracle.first_min(-cross[0])
    assert (int(arg[1]), float(best[1])) == oracle.first_min(-cross[1])
    assert case["dead_at"] == 1


def test_argmin_carries_the_minimum_across_table_chunks(hip_lib, oracle):
    """The table budget is a constant of the build (256 MiB: 131072 points of 256 keys), so the list is long enough for
    two chunks.  Histogram 0's minimum lies in the first chunk and is repeated, bit-equal, in the second (the first
    wins); histogram 1's lies in the second chunk only."""
    from covest_amd import BasicModel, HistogramBatch
    keys, own = _golden_keys(256)
    per_chunk = (256 << 20) // (256 * 8)
    probe = oracle.OracleModel("basic", K, R, dict(zip(keys, own)), 0, max_error=MAX_ERROR)
    p = probe.compute_probabilities(150.0, 0.03)
    other = [float(round(1e6 * p[j])) for j in keys]
    model = BasicModel(K, R, (keys, own), 0, max_error=MAX_ERROR)
    batch = HistogramBatch(model, [own, other, np.zeros(256)], [0.0, 0.0, 5.0])
    pts = np.tile(np.array([[300.0, 0.3]]), (per_chunk + 40, 1))
    pts[5] = pts[per_chunk + 7] = [100.0, 0.02]
    pts[per_chunk + 20] = [150.0, 0.03]
    best, arg = batch.argmin_cross(pts)
    info = batch.info()
    assert info["table_chunks"] == 2 and info["points_tabled"] == per_chunk + 40
    assert arg.tolist()[:2] == [5, per_chunk + 20]
    cross = batch.loglikelihood_cross(pts)
    assert batch.info()["table_chunks"] == 2
    for b in range(3):
        assert (int(arg[b]), float(best[b])) == oracle.first_min(-cross[b]), b
    assert cross[0, 5] == cross[0, per_chunk + 7] == -best[0]
    # the same values whether a point's row lies in the first chunk or in the second
    small = batch.loglikelihood_cross(pts[[5, 0, per_chunk + 20]])
    assert np.array_equal(small, cross[:, [5, 0, per_chunk + 20]])
    batch.close()
    model.close()


@pytest.mark.parametrize("shape", [("basic", 63, 33, 35), ("basic", 256, 33, 35), ("repeats", 63, 33, 35)],
                         ids=["basic-k63", "basic-k256-dead", "repeats-k63"])
def test_the_table_is_shared_by_the_histograms(hip_lib, oracle, shape):
    case = _reference(oracle, shape)
    _, _, _, info = _device(hip_lib, oracle, shape)
    assert info["points_tabled"] == 35 and info["table_chunks"] == 1  # not 33 * 35
    assert info["cross_tiles"] == 3 * 3 and info["pairs_requests"] == 0
    if case["dead_at"] is None:
        assert info["dead_points"] == 0 and info["fixup_waves"] == 0
    else:
        assert info["dead_points"] >= 1 and info["fixup_waves"] == 33 * info["dead_points"]


@pytest.mark.parametrize("kind, tail", [("basic", 0), ("basic", 2500), ("repeats", 0), ("repeats", 2500)])
def test_draw_equals_the_bootstrap_generator(hip_lib, kind, tail):
    from covest_amd import BasicModel, HistogramBatch, RepeatsModel, draw_histograms, model_cells
    keys, own = _golden_keys(65)
    cls = BasicModel if kind == "basic" else RepeatsModel
    model = cls(K, R, (keys, own), tail, max_error=MAX_ERROR)
    theta = [70.0, 0.03] + ([0.7, 0.4, 0.8] if kind == "repeats" else [])
    _, weights, has_tail = model_cells(model, theta)
    n_draws = int(sum(own)) + tail
    want = draw_histograms(weights, n_draws, 5, seed=SEED)
    batch = HistogramBatch.draw(model, theta, replicates=5, seed=SEED)
    counts, tails = batch.counts()
    assert len(batch) == 5 and counts.shape == (5, 65) and has_tail == (tail != 0)
    assert np.array_equal(counts, want[:, :65].astype(np.float64))
    assert np.array_equal(tails, want[:, 65].astype(np.float64) if has_tail else np.zeros(5))
    assert counts.sum() + tails.sum() == 5 * n_draws
    # replicates 2 .. 4 of the same stream, fewer draws, and the histograms usable at once
    later = HistogramBatch.draw(model, theta, replicates=3, seed=SEED, first_replicate=2, n_draws=1000)
    assert np.array_equal(later.counts()[0], draw_histograms(weights, 1000, 3, seed=SEED, first_replicate=2)[:, :65])
    assert np.isfinite(batch.loglikelihood_cross([theta])).all()
    model.close()  # closes both batches
    assert batch._handle is None and later._handle is None


def test_empty_and_edge_calls(hip_lib):
    from covest_amd import BasicModel, HistogramBatch
    keys, own = _golden_keys(5)
    model = BasicModel(K, R, (keys, own), 0, max_error=MAX_ERROR)
    batch = HistogramBatch(model, [own, own])
    none = np.empty((0, 2))
    assert batch.loglikelihood_cross(none).shape == (2, 0)
    assert batch.loglikelihood_pairs([], none).shape == (0,)
    best, arg = batch.argmin_cross(none)
    assert best.tolist() == [math.inf, math.inf] and arg.tolist() == [-1, -1]
    empty = HistogramBatch(model, np.empty((0, 5)))
    assert len(empty) == 0 and empty.loglikelihood_cross([[10.0, 0.05]]).shape == (0, 1)
    assert empty.argmin_cross([[10.0, 0.05]])[0].shape == (0,) and empty.counts()[0].shape == (0, 5)
    drawn = HistogramBatch.draw(model, [10.0, 0.05], replicates=0)
    assert len(drawn) == 0
    one = batch.loglikelihood_cross([[10.0, 0.05]])
    assert one[0, 0] == one[1, 0] and math.isfinite(one[0, 0])
    assert rel_err(float(batch.loglikelihood_pairs([1], [[10.0, 0.05]])[0]), float(one[0, 0])) <= 1e-13
    batch.close()
    batch.close()  # twice
    with pytest.raises(ValueError):
        batch.loglikelihood_cross([[10.0, 0.05]])
    model.close()  # the model first ...
    empty.close()  # ... then its batches
    drawn.close()
    assert empty._handle is None and drawn._handle is None
