"""K-factored with builder waves that skip the key tiles whose copy numbers no unit reads (DESIGN.md section 6ac;
covest_amd/csrc/band.h, factored_build.h build_item) against K-direct: 1e-10 relative with the IEEE specials in the
same places, the same arg-min under the near-tie rule of tests/test_gpu_variants.py.  That every situation a skip can
go wrong in really occurs in these grids -- a wave that never skips, one that skips for good, one that re-enters, a
re-entry on a run start, skips in both buffers, a skip at an item from the 64th on -- is checked without a device,
tests/test_colhi_host.py.

The histogram is tests/test_gpu_factored_band.py's: keys 1 .. 200 and 260 .. 330, ten key tiles, a run start behind the
gap, a short tile either side of it, the last tile taken first.  The grids: c in {12, 21, 30} x e in {0.005, 0.048, 0.08}
x q in {0.11, 0.17, 0.6} over 4 q1 x 4 q2 -- sixteen weight vectors a q, which is what gives a q-tile ONE q and with it
shared steps and a band (four would be laid out by cut-off alone, plan_factored.cpp wants_shared_order, and nothing could
be skipped): cut-offs up to 134, a row stride of 162, three builder waves of four, the smallest shape with a wave that
can skip."""
import os

import numpy as np
import pytest

from test_gpu_factored_band import HIST, LONG_HIST, Q1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q4 = [np.linspace(0.3, 0.95, 4), np.linspace(0.1, 0.9, 4)]
GRIDS = {
    "skip": [np.array([12.0, 21.0, 30.0]), np.array([0.005, 0.048, 0.08]), Q4[0], Q4[1], np.array([0.11, 0.17, 0.6])],
    # low c: units that die in the first interval (the last tile is taken first), bands that reach the unit's top
    "dying": [np.array([0.6, 1.1, 2.0]), np.array([0.02, 0.1]), Q4[0], Q4[1], np.array([0.11, 0.3])],
}
# more than 64 key tiles (keys 1 .. 2200 in 69): the items from the 64th on share the last entry of the limit's table
LONG_GRID = [np.array([12.0, 30.0]), np.array([0.02]), Q1, np.array([0.5]), np.array([0.05, 0.17])]


def _evaluate(m, axes, kernel, flat_range=None):
    from covest_amd import DenseGrid
    g = DenseGrid(m, axes, flat_range)
    g.evaluate(kernel=kernel)
    out = g.loglikelihoods(), g.argmin(), g.launch_record()
    g.close()
    return out


@pytest.fixture(scope="module")
def direct():
    """K-direct's values and arg-min per (histogram, tail, grid): computed once, shared, never changed."""
    cache = {}

    def get(key, m, axes):
        if key not in cache:
            ll, best, _ = _evaluate(m, axes, "direct")
            ll.setflags(write=False)
            cache[key] = (ll, best)
        return cache[key]
    return get


def _check(m, om, axes, tail, name, direct, key):
    from test_gpu_variants import _against_direct, _points, _same_winner
    ll, best, rec = _evaluate(m, axes, "factored")
    rll, rbest = direct(key, m, axes)
    _against_direct(om, ll, rll, tail, name, lambda idx: _points(axes, idx))
    assert _same_winner(best[1], rbest[1], rll), (name, best, rbest)
    return ll, rec


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 7])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_skipping_grid_against_direct(hip_lib, oracle, direct, grid, tail):
    import band_shapes as bs
    import colhi_shapes as cs
    from covest_amd import RepeatsModel
    m = RepeatsModel(21, 100, HIST, tail, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, HIST, tail, max_error=8)
    name = "colskip: %s%s" % (grid, " tail" if tail else "")
    axes = GRIDS[grid]
    ll, rec = _check(m, om, axes, tail, name, direct, (grid, tail))
    want = "ll_factored<256,tail,plain>" if tail else "ll_factored<256,plain>"
    assert want in rec["launches"], (name, rec["launches"])
    plan = next(p for p in rec["plans"] if p["list_mode"] == 0)
    qts = bs.q_tiles(axes[2], axes[3], axes[4], max(HIST))
    assert plan["shared_tiles"] == sum(qt["nsh"] > 0 for qt in qts) and plan["ld"] <= 162, (name, plan, qts)
    # the planner's part of the limit as tests/colhi_shapes.py restates it (what tests/test_colhi_host.py proves it on):
    # below the second builder wave's first copy number, or nothing could be skipped
    if not tail:
        ktiles = bs.key_tiles(HIST)
        floor, _ = cs.col_floor(qts, cs.place_units(qts, cs.build_cost(ktiles)))
        assert plan["col_floor"] == floor, (name, plan, floor)
    assert plan["col_floor"] < cs.WAVE, (name, plan)
    n_inf, n_fin = int(np.isneginf(ll).sum()), int(np.isfinite(ll).sum())
    print("\n%s: %d points, %d finite, %d -inf, col_floor %d" % (name, ll.size, n_fin, n_inf, plan["col_floor"]))
    assert n_fin > 0 and (grid != "dying" or n_inf > 0), name
    # a block cut through the grid -- through a (c, e) pair's weight vectors at either end: the whole grid's bits
    total = ll.size
    lo, hi = total // 3 + 5, total - total // 4 - 3
    part, _, _ = _evaluate(m, axes, "factored", (lo, hi))
    assert np.array_equal(part, ll[lo:hi], equal_nan=True), name
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 7])
def test_skips_beyond_the_64th_item(hip_lib, oracle, direct, tail):
    from covest_amd import RepeatsModel
    m = RepeatsModel(21, 100, LONG_HIST, tail, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, LONG_HIST, tail, max_error=8)
    ll, rec = _check(m, om, LONG_GRID, tail, "colskip: 69 tiles%s" % (" tail" if tail else ""), direct, ("long", tail))
    plan = next(p for p in rec["plans"] if p["list_mode"] == 0)
    assert plan["shared_tiles"] == 2 and plan["col_floor"] < 64 and plan["n_threads"] == 512, plan
    assert np.isfinite(ll).any()
    m.close()


@pytest.mark.gpu
def test_paths_without_a_skip_keep_their_bits(hip_lib):
    """A grid whose weight vectors are longer than a workgroup's 512 lanes (chunks: list mode 3) and a point list (list
    modes 1 and 2) build every column as before: bit for bit the values of the commit before this one
    (tests/golden/colskip_unskipped.npz, written by that commit's library on an MI355X)."""
    from covest_amd import RepeatsModel
    from test_gpu_variants import H1600, LONG, _list_points
    want = np.load(os.path.join(GOLDEN, "colskip_unskipped.npz"))
    m = RepeatsModel(21, 100, H1600, 0, max_error=8)
    ll, _, rec = _evaluate(m, LONG, "factored")
    assert any(p["list_mode"] == 3 for p in rec["plans"]), rec["plans"]
    assert np.array_equal(ll, want["chunked"], equal_nan=True)
    m.close()
    m = RepeatsModel(21, 100, {**HIST, 700: 3}, 0, max_error=8)
    pts = _list_points(23, 24, 40.0)
    fast = m.loglikelihood_points(pts, kernel="factored")
    plans = m.launch_record()["plans"]
    assert any(p["list_mode"] == 1 for p in plans) and any(p["list_mode"] == 2 for p in plans), plans
    assert np.array_equal(fast, want["points"], equal_nan=True)
    m.close()
