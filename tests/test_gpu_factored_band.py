"""K-factored with the contraction cut to each unit's band (covest_amd/csrc/band.h) against
K-direct: 1e-10 relative with the IEEE specials in the same places, the same arg-min under the near-tie rule of
tests/test_gpu_variants.py.  Small grids of the repeats model, chosen for where a band can go wrong; that each named
situation really occurs in them is checked without a device, tests/test_band_host.py (SITUATIONS below).

The histogram: keys 1 .. 200 and 260 .. 330 with falling counts -- ten key tiles, one gap too wide to bridge (a run
start in the middle of the walk), a short tile on either side of it, and a last tile that the tail-less walk takes
first.  Its largest key caps threshold_o at 330, so q = 0.05 gives cut-offs of 232 .. 284 (the 290-column row stride)."""
import math

import numpy as np
import pytest


def _falling(keys, top):
    return {int(j): max(1, int(top * math.exp(-0.02 * i))) for i, j in enumerate(keys)}


HIST = _falling(list(range(1, 201)) + list(range(260, 331)), 50000)
Q1 = np.linspace(0.3, 0.95, 16)  # 16 values and one q2: every q-tile has one q, and shared steps where it is long enough
GRIDS = {
    # q = 0.05: units of 71 steps, 56 of them shared; q = 0.2: 19 steps, 14 shared; q = 0.8: units too short for shared
    # steps (q = 0.6 still has three)
    "band": [np.array([4.0, 12.0, 30.0]), np.array([0.005, 0.08]), Q1, np.array([0.5]), np.array([0.05, 0.2, 0.8])],
    # low c: the copy numbers' means stop below the late keys -- units that die in the first interval (the last tile is
    # taken first), bands that reach the unit's top (refused) and rows near e^-300 at the mid points
    "dying": [np.array([0.6, 1.1, 2.0]), np.array([0.02, 0.1]), Q1, np.array([0.5]), np.array([0.05, 0.3])],
}
# what tests/test_band_host.py must find in each grid: a band refused in some tile (the full range), a band that cuts,
# q-tiles without shared steps (no band at all) and with them
SITUATIONS = {"band": ["refused", "cut", "unbanded", "banded"], "dying": ["refused", "cut", "banded"]}


def _compare(m, om, axes, tail, name):
    from covest_amd import DenseGrid
    from test_gpu_variants import _against_direct, _points, _same_winner
    fac = DenseGrid(m, axes)
    fac.evaluate(kernel="factored")
    rec = fac.launch_record()
    ll, best = fac.loglikelihoods(), fac.argmin()
    ref = DenseGrid(m, axes)
    ref.evaluate(kernel="direct")
    rll, rbest = ref.loglikelihoods(), ref.argmin()
    _against_direct(om, ll, rll, tail, name, lambda idx: _points(axes, idx))
    assert _same_winner(best[1], rbest[1], rll), (name, best, rbest)
    fac.close()
    ref.close()
    return rec, ll


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 7])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_banded_grid_against_direct(hip_lib, oracle, grid, tail):
    from covest_amd import RepeatsModel
    m = RepeatsModel(21, 100, HIST, tail, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, HIST, tail, max_error=8)
    name = "band: %s%s" % (grid, " tail" if tail else "")
    rec, ll = _compare(m, om, GRIDS[grid], tail, name)
    want = "ll_factored<512,tail,plain,ld290>" if tail else "ll_factored<512,plain,ld290>"
    assert want in rec["launches"], (name, rec["launches"])
    assert any(p["shared_tiles"] > 0 and p["list_mode"] == 0 for p in rec["plans"]), (name, rec["plans"])
    n_inf, n_fin = int(np.isneginf(ll).sum()), int(np.isfinite(ll).sum())
    print("\n%s: %d points, %d finite, %d -inf, lowest finite %.6g" % (name, ll.size, n_fin, n_inf, ll[np.isfinite(ll)].min()))
    assert n_fin > 0
    # the planner's shapes as tests/band_shapes.py restates them (what tests/test_band_host.py proves the band on)
    import band_shapes as bs
    axes = GRIDS[grid]
    qts = bs.q_tiles(axes[2], axes[3], axes[4], max(HIST))
    plan = next(p for p in rec["plans"] if p["list_mode"] == 0)
    assert plan["shared_tiles"] == sum(qt["nsh"] > 0 for qt in qts), (name, plan, qts)
    assert plan["ld"] == (max(qt["t_hi"] for qt in qts) - 1 + 31) // 32 * 32 + 2, (name, plan)
    assert m.bins_evaluated == sum(nb for _, nb in bs.key_tiles(HIST)), name  # (no filler keys: the gap is a run start)
    if grid == "dying":
        assert n_inf > 0, name  # (units that die: a weight vector whose p_j is 0 at a counted key)
        # ... and finite sums that hold a p_j near e^-300: the three lowest finite points, by the oracle
        from test_gpu_variants import _points
        low = np.argsort(np.where(np.isfinite(ll), ll, np.inf))[:3]
        smallest = min(min(v for v in om.compute_probabilities(*p).values()) for p in _points(axes, low))
        print("%s: smallest p_j among the three lowest finite points %.3g" % (name, smallest))
        assert 0.0 < smallest < 1e-100, (name, smallest)
    m.close()


# More than 64 key tiles: the bands of the items from the 64th on share one entry (the last lane's: one key range from
# the 64th item's first key to the histogram's last), keys 1 .. 2200 in 69 tiles
LONG_HIST = _falling(range(1, 2201), 50000)
LONG_GRID = [np.array([12.0, 30.0]), np.array([0.02]), Q1, np.array([0.5]), np.array([0.05])]


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 7])
def test_more_items_than_lanes(hip_lib, oracle, tail):
    from covest_amd import RepeatsModel
    m = RepeatsModel(21, 100, LONG_HIST, tail, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, LONG_HIST, tail, max_error=8)
    rec, ll = _compare(m, om, LONG_GRID, tail, "band: 69 tiles%s" % (" tail" if tail else ""))
    assert any(p["shared_tiles"] > 0 and p["list_mode"] == 0 for p in rec["plans"]), rec["plans"]
    assert np.isfinite(ll).any()
    m.close()


@pytest.mark.gpu
def test_unbanded_paths_are_as_before(hip_lib, oracle):
    """A grid whose weight vectors are longer than a workgroup's 512 lanes (chunks: list mode 3) and a point list (list
    modes 1 and 2): kernels without a band, against K-direct as before."""
    from covest_amd import RepeatsModel
    from test_gpu_variants import H1600, LONG, _against_direct, _list_points, _same_winner
    m = RepeatsModel(21, 100, H1600, 0, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, H1600, 0, max_error=8)
    rec, _ = _compare(m, om, LONG, 0, "band: long parts")
    assert any(p["list_mode"] == 3 for p in rec["plans"]), rec["plans"]
    m.close()
    hist = {**HIST, 700: 3}
    m = RepeatsModel(21, 100, hist, 0, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, hist, 0, max_error=8)
    pts = _list_points(23, 24, 40.0)
    fast = m.loglikelihood_points(pts, kernel="factored")
    plans = m.launch_record()["plans"]
    assert any(p["list_mode"] == 1 for p in plans) and any(p["list_mode"] == 2 for p in plans), plans
    ref = m.loglikelihood_points(pts, kernel="direct")
    _against_direct(om, fast, ref, 0, "band: point list", lambda idx: pts[idx])
    assert _same_winner(oracle.first_min(-fast)[0], oracle.first_min(-ref)[0], ref)
    m.close()
