"""The strict re-evaluation of the handed-back points, put off until somebody reads the values.

A plain evaluate() launches the recurrence kernel and an arg-min that proves its winner on the provisional values; the
patching pass (ll_fix.hip) runs when the values, the per-axis minima, the launch record or a device pointer are asked
for, and from argmin() only where the winner could not be proven.  Every case here is held against a second handle that
patches inside every evaluation (DenseGrid.fix_eager: the order before the change): the values byte for byte, the
arg-min pair, and the arg-min of the final values under the reference's rule (first_wins_scan).

The histogram is H280 of tests/test_gpu_variants.py: keys 1..40 falling and key 280 with count 2, whose p_j crosses the
clamp of handback.h inside the grids below -- chosen with the oracle on the CPU: per point p_280 is 0 (LL = -inf), below
p_clamp (the point is handed back), or above it.  Whether a pass is still owed is read off the diagnostic
provisional_loglikelihoods(): it succeeds exactly while one is.  The queue itself is not visible from the host (the launch
record is host bookkeeping), so "the queue is not empty" is asserted through its effect: the record shows the pass and
some value moved.
"""
import math

import numpy as np
import pytest


def _falling(keys, top):
    return {int(j): max(1, int(top * math.exp(-0.07 * i))) for i, j in enumerate(keys)}


H280 = {**_falling(range(1, 41), 20000), 280: 2}
E8 = np.linspace(0.01, 0.04, 8)
# basic, 8 x 8: per row of c (13 .. 18) one point handed back between the normal ones and the -inf ones (flat 1, 18, 35, 52, 60)
BASIC_8X8 = [np.linspace(13.0, 18.0, 8), E8]
# repeats, 3 x 2 x 4 x 2 x 5: eleven points handed back (flat 47 .. 77 at c = 2, 124 .. 144 at c = 3), nineteen at -inf
REPEATS_240 = [np.array([2.0, 3.0, 4.0]), np.array([0.02, 0.05]), np.linspace(0.4, 0.9, 4), np.array([0.3, 0.7]),
               np.array([0.3, 0.5, 0.7, 0.8, 0.9])]
# only handed-back points are finite, everything else is -inf (c = 13 twice: an exact tie between two queued points)
BASIC_FALLBACK = [np.array([13.0, 13.0]), E8[1:]]
REPEATS_FALLBACK = [np.array([2.0]), np.array([0.05]), np.array([0.9]), np.array([0.3, 0.7]), np.array([0.7, 0.8, 0.9])]
# every c twice: exact ties among the handed-back points and among the others
BASIC_TIES = [np.repeat(np.linspace(13.0, 18.0, 8)[[0, 2, 4, 6]], 2), E8]
# beyond one workgroup's reach (16 384 points): the two-stage arg-min
BASIC_TWO_STAGE = [np.linspace(13.0, 18.0, 160), np.linspace(0.01, 0.04, 110)]
BASIC_TWO_STAGE_FALLBACK = [np.linspace(12.0, 13.0, 150), np.linspace(E8[1], 0.04, 110)]

FIX = {"recur": "fix_basic_packed<8>", "factored": "fix_list<5,1>"}


@pytest.fixture(scope="module")
def models(hip_lib):
    from covest_amd import BasicModel, RepeatsModel
    ms = {"recur": BasicModel(21, 100, H280, 0, max_error=8), "factored": RepeatsModel(21, 100, H280, 0, max_error=8)}
    yield ms
    for m in ms.values():
        m.close()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _owed(g):
    """Whether the strict pass of the last evaluate() is still owed."""
    from covest_amd import _capi
    try:
        g.provisional_loglikelihoods()
        return True
    except _capi.CovestHipError:
        return False


def _eager(model, axes, kernel, flat_range=None):
    """(values, arg-min pair, launches) of a handle that patches inside the evaluation."""
    from covest_amd import DenseGrid
    g = DenseGrid(model, axes, flat_range)
    g.fix_eager(True)
    g.evaluate(kernel=kernel)
    assert not _owed(g)
    out = g.loglikelihoods(), g.argmin(), g.launch_record()["launches"]
    g.close()
    return out


def _reference_argmin(ll, begin=0):
    from covest_amd.grid import first_wins_scan
    val, arg, _ = first_wins_scan(-ll, math.inf, 1)
    return (val, arg + begin) if arg >= 0 else (math.inf, -1)


def _argmin_name(n):
    return "argmin_small" if n <= 16384 else "argmin_stage1+2"


def _check_lazy(model, axes, kernel, flat_range=None, want_moved=True):
    """One evaluate() on a fresh handle: what is provisional, what is final, against the eager handle.  Returns
    (provisional, final, arg-min, fell_back)."""
    from covest_amd import DenseGrid
    g = DenseGrid(model, axes, flat_range)
    g.evaluate(kernel=kernel)
    prov = g.provisional_loglikelihoods()  # (owed: the call succeeds)
    best = g.argmin()
    fell_back = not _owed(g)
    ll = g.loglikelihoods()
    assert not _owed(g)
    launches = g.launch_record()["launches"]
    g.close()
    ell, ebest, elaunches = _eager(model, axes, kernel, flat_range)
    n, begin = len(ll), (flat_range[0] if flat_range else 0)
    # final values: the eager handle's, byte for byte; the same pass, and the arg-min a second time behind it
    assert ll.tobytes() == ell.tobytes()
    assert launches[FIX[kernel]] == 1 and launches[_argmin_name(n)] == 2, launches
    assert elaunches[FIX[kernel]] == 1 and elaunches[_argmin_name(n)] == 1, elaunches
    # the arg-min: the eager handle's and the reference's rule over the final values
    want = _reference_argmin(ll, begin)
    assert best[1] == ebest[1] == want[1], (best, ebest, want)
    assert best[1] < 0 or best[0] == ebest[0] == want[0], (best, ebest, want)
    # the bound: a value the pass moved was above its final value (-LL provisional is a lower bound); every other bit for bit
    moved = _bits(prov) != _bits(ll)
    assert bool(moved.any()) == want_moved, int(moved.sum())
    assert not np.isnan(prov[moved]).any() and not np.isnan(ll[moved]).any()
    assert np.all(prov[moved] > ll[moved]), (prov[moved], ll[moved])
    return prov, ll, best, fell_back


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,axes,n_handed_back", [("recur", BASIC_8X8, 5), ("factored", REPEATS_240, 11)])
def test_final_values_and_the_bound(models, kernel, axes, n_handed_back):
    prov, ll, best, fell_back = _check_lazy(models[kernel], axes, kernel)
    moved = np.flatnonzero(_bits(prov) != _bits(ll))
    # (the oracle's count of points whose p_280 is below the clamp: the nearest is at 0.62 of it, the nearest above at 2.3)
    assert len(moved) == n_handed_back, moved
    assert np.isneginf(ll).any() and np.isfinite(ll[moved]).all()
    # (the oracle's winner is a normal point, 2e4 in -LL below the runner-up: the margin is 2e-3)
    assert not fell_back and best[1] >= 0 and best[1] not in set(moved.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,axes", [("recur", BASIC_FALLBACK), ("factored", REPEATS_FALLBACK),
                                         ("recur", BASIC_TWO_STAGE_FALLBACK)])
def test_a_queued_winner_takes_the_fallback(models, kernel, axes):
    """Every finite point is a handed-back one: the winner is queued, the flag is set, argmin() runs the pass and the
    arg-min again and returns the final pair."""
    prov, ll, best, fell_back = _check_lazy(models[kernel], axes, kernel)
    assert fell_back
    finite = np.isfinite(ll)
    # every finite point was handed back and moved (a handed-back point may also end at -inf: a p_280 that only the strict
    # evaluation can tell from 0, handback.h kZeroSteps)
    assert finite.any() and np.all((_bits(prov) != _bits(ll))[finite])
    assert np.all(np.isneginf(ll[~finite]))
    assert best[1] >= 0 and best[0] == -ll[best[1]]


@pytest.mark.gpu
def test_two_stage_arg_min_proves_its_winner(models):
    prov, ll, best, fell_back = _check_lazy(models["recur"], BASIC_TWO_STAGE, "recur")
    assert not fell_back  # (the oracle's winner is a normal point, 775 in -LL below the runner-up: the margin is 2e-3)
    assert (_bits(prov) != _bits(ll)).sum() >= 100


@pytest.mark.gpu
def test_edges(models, hip_lib):
    from covest_amd import BasicModel, DenseGrid
    from conftest import load_hist
    m = models["recur"]
    # an empty queue: nothing is handed back, the pass is owed all the same and moves nothing; argmin() leaves it owed
    plain = BasicModel(21, 100, load_hist("sim_c10_e0.05"), 0, max_error=8)
    axes = [np.linspace(8.0, 12.0, 24), np.linspace(0.01, 0.09, 16)]
    _, _, _, fell_back = _check_lazy(plain, axes, "recur", want_moved=False)
    assert not fell_back
    plain.close()
    # nothing wins: -inf and NaN everywhere, no fallback and (inf, -1)
    doomed = [np.array([float("nan"), 1.0, 2.0, float("nan")]), E8]
    _, ll, best, fell_back = _check_lazy(m, doomed, "recur", want_moved=False)
    assert np.isnan(ll).any() and np.isneginf(ll).any() and not np.isfinite(ll).any()
    assert best == (math.inf, -1) and not fell_back
    # one point, a handed-back one
    _, ll, best, fell_back = _check_lazy(m, [np.array([13.0]), E8[1:2]], "recur")
    assert fell_back and best == (-ll[0], 0)
    # one point, a normal one
    _, ll, best, fell_back = _check_lazy(m, [np.array([18.0]), E8[:1]], "recur", want_moved=False)
    assert not fell_back and best == (-ll[0], 0)
    # blocks of the flat range that begin and end on handed-back points, and one between them
    for lo, hi in ((18, 53), (1, 2), (19, 35)):
        _check_lazy(m, BASIC_8X8, "recur", flat_range=(lo, hi), want_moved=(lo, hi) != (19, 35))
    _check_lazy(models["factored"], REPEATS_240, "factored", flat_range=(47, 125))
    # duplicate axis values: exact ties among handed-back points and among the others, the lowest index wins
    _, ll, best, _ = _check_lazy(m, BASIC_TIES, "recur")
    rows = ll.reshape(8, 8)
    for r in range(0, 8, 2):
        assert np.array_equal(_bits(rows[r]), _bits(rows[r + 1])), r
    assert best[1] + 8 < 64 and _bits(ll)[best[1]] == _bits(ll)[best[1] + 8] and (best[1] // 8) % 2 == 0
    g = DenseGrid(m, BASIC_FALLBACK)  # (the tie between the two queued winners)
    g.evaluate(kernel="recur")
    assert g.argmin()[1] == 0 and _bits(g.loglikelihoods())[0] == _bits(g.loglikelihoods())[7]
    g.close()


@pytest.mark.gpu
def test_state(models):
    from covest_amd import DenseGrid, _capi
    m = models["recur"]
    ell, ebest, _ = _eager(m, BASIC_8X8, "recur")
    dll, dbest, _ = _eager(m, BASIC_8X8, "direct")
    g = DenseGrid(m, BASIC_8X8)
    # evaluate() twice without reading: the second evaluation's values, whichever of the two owed a pass
    g.evaluate(kernel="recur")
    g.evaluate(kernel="recur")
    assert _owed(g) and g.loglikelihoods().tobytes() == ell.tobytes() and g.argmin() == ebest
    g.evaluate(kernel="recur")
    g.evaluate(kernel="direct")
    assert not _owed(g) and g.loglikelihoods().tobytes() == dll.tobytes() and g.argmin() == dbest
    assert set(g.launch_record()["launches"]) == {"ll_direct", "argmin_small"}
    g.evaluate(kernel="recur")
    assert _owed(g) and g.argmin() == ebest and _owed(g)
    assert g.loglikelihoods().tobytes() == ell.tobytes()
    # reset with a pass owed: it is dropped, the next evaluation is the new grid's
    g.evaluate(kernel="recur")
    g.reset(BASIC_TIES)
    assert not _owed(g)
    g.evaluate(kernel="recur")
    tll, tbest, _ = _eager(m, BASIC_TIES, "recur")
    assert _owed(g) and g.loglikelihoods().tobytes() == tll.tobytes() and g.argmin() == tbest
    g.reset(BASIC_8X8)
    # each reader completes on its own, and a second call launches nothing more
    done = {"ll_basic<8>": 1, FIX["recur"]: 1, "argmin_small": 2}
    readers = {"axis_minima": lambda: g.axis_minima(()), "loglikelihoods": g.loglikelihoods,
               "launch_record": g.launch_record, "ll_device_ptr": lambda: g.ll_device_ptr, "complete": g.complete}
    for name, read in readers.items():
        g.evaluate(kernel="recur")
        assert _owed(g), name
        first = read()
        assert not _owed(g), name
        assert g.launch_record()["launches"] == done, (name, g.launch_record())
        read()
        assert g.launch_record()["launches"] == done, (name, g.launch_record())
        if name == "axis_minima":
            assert (float(first[0]), int(first[1])) == ebest
        if name == "ll_device_ptr":
            assert first
        assert g.loglikelihoods().tobytes() == ell.tobytes() and g.argmin() == ebest, name
    # the scan path keeps the pass inside, before the scan
    g.evaluate(kernel="recur", scan_start=math.inf)
    assert not _owed(g)
    rec = g.launch_record()["launches"]
    assert rec == {"ll_basic<8>": 1, FIX["recur"]: 1, "argmin_scan_small": 1}
    assert list(rec).index(FIX["recur"]) < list(rec).index("argmin_scan_small")
    idx, val = g.scan_records()
    assert idx[-1] == ebest[1] and val[-1] == ebest[0]
    # the arg-min pair taken on the device: completed, and the handle patches inside its evaluations from then on
    g.evaluate(kernel="recur")
    assert _owed(g)
    assert _capi.lib().covest_grid_argmin_pair_device(g._handle)
    assert not _owed(g)
    assert g.launch_record()["launches"] == done
    g.evaluate(kernel="recur")
    assert not _owed(g)
    assert g.launch_record()["launches"] == {"ll_basic<8>": 1, FIX["recur"]: 1, "argmin_small": 1}
    assert g.loglikelihoods().tobytes() == ell.tobytes() and g.argmin() == ebest
    g.fix_eager(False)
    g.evaluate(kernel="recur")
    assert _owed(g)
    g.close()
