"""K-factored where the planner charges every builder wave its own share of the build charge (DESIGN.md section 6ah;
covest_amd/csrc/unit_deal.h kBuildShare, plan_factored.cpp place_units): a dense plain grid with one workgroup a (c, e) pair
-- 192 pairs or more -- deals its units by falling charges, because its upper builder waves skip items (section 6ac);
every other grid keeps the one charge and the tables it had.

The shapes are tests/test_gpu_factored_colskip.py's, widened to 192 pairs: keys 1 .. 200 and 260 .. 330, 16 values of c
in 12 .. 30 x 12 values of e in 0.005 .. 0.08 (lambda0 = c (1 - e)^21 spans a decade), q in {0.11, 0.17, 0.6} over
4 q1 x 4 q2, with nineteen more key tiles at keys 400 .. 1000 (the falling charges are for histograms that reach beyond
the low keys), with and without a tail; the low keys alone, which keep the one charge; and the 2 200-key histogram (69
items) once.  On each: K-factored against K-direct at 1e-10 with the specials in the same places and the same arg-min;
the real plan's col_floor equal to the deal restated here WITH the shares; a block cut through the grid bit-equal to the
whole grid; the e axis reversed giving the same bits point for point.  A deal moves no value by more than the order of
a point's sums: nothing here leans on the bits of the commit before, only tests/test_gpu_factored_colskip.py's paths
without a skip do, and they keep theirs."""
import numpy as np
import pytest

from test_gpu_factored_band import HIST, LONG_HIST, Q1, _falling
from test_gpu_factored_colskip import Q4, _evaluate

SHARES = (100, 75, 40, 40, 40, 40, 40, 40)  # unit_deal.h kBuildShare
C16, E12 = np.linspace(12.0, 30.0, 16), np.linspace(0.005, 0.08, 12)
GRID = [C16, E12, Q4[0], Q4[1], np.array([0.11, 0.17, 0.6])]
LONG_GRID = [C16, E12, Q1, np.array([0.5]), np.array([0.05, 0.17])]
# HIST's ten key tiles and nineteen more at keys 400 .. 1000: a histogram at low keys alone (HIST: every tile starts at
# or below tiles.h kLowKeyTile) keeps the one charge, as the trimmed histograms of a real run do
HIGH_HIST = _falling(list(range(1, 201)) + list(range(260, 331)) + list(range(400, 1001)), 50000)
EVEN = (100,) * 8


def place_units(qts, charge, shares):
    """tests/colhi_shapes.py place_units with plan_factored.cpp's charge per builder wave: charge x share, rounded."""
    import colhi_shapes as cs
    n_columns, nw = cs.geometry(qts)
    units = []
    for i, qt in enumerate(qts):
        nsh = qt["nsh"]
        cost = max(1, qt["n_steps"] - nsh) + cs.UNIT_OVERHEAD + ((1 + (nsh + cs.SHARED_DIV - 1) // cs.SHARED_DIV) if nsh else 0)
        units += [(i, 0, cost), (i, 1, cost)]
    units.sort(key=lambda u: -u[2])
    n_bins = min(4, nw)
    bin_load, wave_load = [0] * n_bins, [0] * nw
    for w in range(nw):
        if w * cs.WAVE < n_columns:
            c = (charge * shares[w] + 50) // 100 + (cs.LAST_BUILDER_EXTRA if ((w + 1) * cs.WAVE >= n_columns and w >= n_bins) else 0)
            bin_load[w % n_bins] += c
            wave_load[w] += c
    held = [[] for _ in range(nw)]
    for i, h, cost in units:
        best = -1
        for w in range(nw):
            if len(held[w]) >= cs.MAX_UNITS:
                continue
            if best < 0 or bin_load[w % n_bins] < bin_load[best % n_bins] or (
                    bin_load[w % n_bins] == bin_load[best % n_bins] and wave_load[w] < wave_load[best]):
                best = w
        held[best].append((i, h))
        bin_load[best % n_bins] += cost
        wave_load[best] += cost
    return held


def test_restatement_with_even_shares_is_the_shared_one():
    """(no device) the deal restated here with every share at 100 is tests/colhi_shapes.py's, and the shipped shares
    deal this file's grid differently: the GPU cases below do run another deal than the commit before."""
    import band_shapes as bs
    import colhi_shapes as cs
    qts = bs.q_tiles(GRID[2], GRID[3], GRID[4], max(HIGH_HIST))
    charge = cs.build_cost(bs.key_tiles(HIGH_HIST))
    assert charge == cs.BUILD_COST and cs.build_cost(bs.key_tiles(HIST)) == cs.BUILD_COST_LOW
    assert place_units(qts, charge, EVEN) == cs.place_units(qts, charge)
    assert place_units(qts, charge, SHARES) != cs.place_units(qts, charge)


@pytest.fixture(scope="module")
def direct():
    """K-direct's values and arg-min per case: computed once, shared, never changed."""
    cache = {}

    def get(key, m, axes):
        if key not in cache:
            ll, best, _ = _evaluate(m, axes, "direct")
            ll.setflags(write=False)
            cache[key] = (ll, best)
        return cache[key]
    return get


def _case(oracle, direct, hist, axes, tail, name, threads, shares=SHARES):
    import band_shapes as bs
    import colhi_shapes as cs
    from covest_amd import RepeatsModel
    from test_gpu_variants import _against_direct, _points, _same_winner
    m = RepeatsModel(21, 100, hist, tail, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, hist, tail, max_error=8)
    ll, best, rec = _evaluate(m, axes, "factored")
    rll, rbest = direct((name, tail), m, axes)
    _against_direct(om, ll, rll, tail, name, lambda idx: _points(axes, idx))
    assert _same_winner(best[1], rbest[1], rll), (name, best, rbest)
    assert np.isfinite(ll).any(), name
    plan = next(p for p in rec["plans"] if p["list_mode"] == 0)
    assert plan["n_threads"] == threads and plan["n_qblocks"] == 1, (name, plan)
    # (with a tail too: every key of these histograms has a count, so no item of the walk stands for several tiles and
    # the charge is the tail-less one)
    qts = bs.q_tiles(axes[2], axes[3], axes[4], max(hist))
    floor, _ = cs.col_floor(qts, place_units(qts, cs.build_cost(bs.key_tiles(hist)), shares))
    assert plan["col_floor"] == floor, (name, plan, floor)
    # a block cut through the grid, through a (c, e) pair's weight vectors at either end: the whole grid's bits
    total = ll.size
    lo, hi = total // 3 + 5, total - total // 4 - 3
    part, _, _ = _evaluate(m, axes, "factored", (lo, hi))
    assert np.array_equal(part, ll[lo:hi], equal_nan=True), name
    # the e axis reversed: the same bits point for point (a pair's deal and sums do not depend on where it stands)
    rev = [axes[0], axes[1][::-1].copy()] + list(axes[2:])
    rl, _, _ = _evaluate(m, rev, "factored")
    shape = tuple(len(a) for a in axes)
    assert np.array_equal(rl.reshape(shape)[:, ::-1], ll.reshape(shape), equal_nan=True), name
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 7])
def test_falling_charges_against_direct(hip_lib, oracle, direct, tail):
    _case(oracle, direct, HIGH_HIST, GRID, tail, "wave charges: 192 pairs%s" % (" tail" if tail else ""), 256)


@pytest.mark.gpu
def test_low_keys_keep_the_one_charge(hip_lib, oracle, direct):
    _case(oracle, direct, HIST, GRID, 0, "wave charges: 192 pairs at low keys", 256, EVEN)


# The shapes the shares are gated off for, beside the chunked grid and the point list of
# tests/test_gpu_factored_colskip.py (tests/golden/colskip_unskipped.npz): name -> (histogram, axes, max_error)
SMALL = [np.array([12.0, 21.0, 30.0]), np.array([0.005, 0.048, 0.08])] + GRID[2:]
GATED = {"below192": (HIGH_HIST, SMALL, 8), "s22": (HIGH_HIST, GRID, 22), "lowkeys": (HIST, GRID, 8)}


@pytest.mark.gpu
def test_gated_off_shapes_keep_their_bits(hip_lib):
    """A grid below 192 pairs, a model with more than 8 error classes and a histogram at low keys alone keep the one
    charge: bit for bit the values of the commit before this one (tests/golden/wave_charges_parent.npz, written by that
    commit's library on an MI355X)."""
    import os
    from covest_amd import RepeatsModel
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_charges_parent.npz"))
    for name, (hist, axes, max_error) in GATED.items():
        m = RepeatsModel(21, 100, hist, 0, max_error=max_error)
        ll, _, rec = _evaluate(m, axes, "factored")
        assert any(p["list_mode"] == 0 for p in rec["plans"]), (name, rec["plans"])
        assert np.array_equal(ll, want[name], equal_nan=True), name
        m.close()


@pytest.mark.gpu
def test_falling_charges_beyond_the_64th_item(hip_lib, oracle, direct):
    _case(oracle, direct, LONG_HIST, LONG_GRID, 0, "wave charges: 69 tiles", 512)
