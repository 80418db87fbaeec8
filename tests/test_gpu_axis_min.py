"""Per-axis minima of a dense grid on the device (covest_grid_axis_min, DenseGrid.axis_minima; `-m gpu`).

1-2. exact against the handle's own values: a numpy restatement of the per-cell selection scan over
     grid.loglikelihoods(), every mask, values bit-equal and indices identical; mask 0 is argmin(), all axes kept is
     -loglikelihoods() itself;
3.   blocks that split cells merge to the whole grid's result (merge_axis_minima, DeviceBlocks);
4.   calling order, and nothing else of the handle changes;
5.   against the reference (tests/golden/axis_min.json, tests/golden/make_golden_axis_min.py);
6.   the coverage interval end to end against the oracle's profile.
"""
import itertools

import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err

pytestmark = pytest.mark.gpu

C3_AXES = [np.linspace(15.0, 30.0, 128), np.linspace(0.005, 0.08, 128), np.linspace(0.3, 0.95, 16), np.array([0.5]),
           np.linspace(0.05, 0.95, 16)]


def _thin_c3():
    """The C3 axes of bench.py thinned to 8 x 8 x 16 x 1 x 16 = 16 384 points (about half of them LL = -inf)."""
    return [C3_AXES[0][::16], C3_AXES[1][::16], C3_AXES[2], C3_AXES[3], C3_AXES[4]]


def numpy_axis_minima(ll, shape, keep, flat_begin=0):
    """The per-cell selection scan restated: `ll` the block's values from flat index `flat_begin` on.  Reshape, kept
    axes forward, first index of the strict minimum per cell; a NaN never wins and +inf never wins (as
    covest_amd.grid.first_wins_scan: `val < min_val` from +inf), such cells are (+inf, -1)."""
    total = int(np.prod(shape, dtype=np.int64))
    neg = np.full(total, np.inf)
    with np.errstate(invalid="ignore"):
        block = -np.asarray(ll, dtype=np.float64)
    block[np.isnan(block)] = np.inf
    neg[flat_begin:flat_begin + len(block)] = block
    keep = sorted(keep)
    order = keep + [d for d in range(len(shape)) if d not in keep]
    kept_shape = tuple(shape[d] for d in keep)
    n_cells = int(np.prod(kept_shape, dtype=np.int64))
    vals = np.transpose(neg.reshape(shape), order).reshape(n_cells, -1)
    flat = np.transpose(np.arange(total, dtype=np.int64).reshape(shape), order).reshape(n_cells, -1)
    first = np.argmin(vals, axis=1)  # the first occurrence of the minimum = the lowest flat index
    rows = np.arange(n_cells)
    best, arg = vals[rows, first].copy(), flat[rows, first].copy()
    arg[best == np.inf] = -1
    return best.reshape(kept_shape), arg.reshape(kept_shape)


def _bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _all_masks(n_axes):
    return [tuple(d for d in range(n_axes) if (mask >> d) & 1) for mask in range(1 << n_axes)]


def _check_every_mask(grid, name):
    ll = grid.loglikelihoods()
    stats = {"cells": 0, "empty": 0, "tied": 0}
    for keep in _all_masks(len(grid.shape)):
        want_v, want_i = numpy_axis_minima(ll, grid.shape, keep, grid.flat_range[0])
        got_v, got_i = grid.axis_minima(keep)
        assert got_v.dtype == np.float64 and got_i.dtype == np.int64
        assert got_v.shape == want_v.shape == tuple(grid.shape[d] for d in keep), (name, keep)
        assert _bit_equal(got_v, want_v), (name, keep, "values")
        assert np.array_equal(got_i, want_i), (name, keep, "indices")
        stats["cells"] += want_v.size
        stats["empty"] += int((want_i < 0).sum())
    print("%s: %d masks, %d cells, %d of them (+inf, -1)" % (name, 1 << len(grid.shape), stats["cells"], stats["empty"]))
    return ll, stats


def _sim_models(tail=0):
    from covest_amd import BasicModel, RepeatsModel
    hist = load_hist("sim_c10_e0.05")
    return BasicModel(21, 100, hist, tail, max_error=8, device=0), RepeatsModel(21, 100, hist, tail, max_error=8, device=0)


# ----------------------------------------------------------------------------- 1, 2
def test_every_mask_exact_on_the_smoke_grids(hip_lib):
    from covest_amd import DenseGrid
    basic, rep = _sim_models()
    g = DenseGrid(basic, [np.linspace(8.0, 12.0, 24), np.linspace(0.01, 0.09, 16)])
    g.evaluate()
    _check_every_mask(g, "smoke basic 24x16")
    axes = [np.array([9.0, 10.0, 11.0]), np.array([0.03, 0.05]), np.linspace(0.4, 1.0, 4), np.array([0.2, 0.6]),
            np.linspace(0.05, 0.9, 5)]
    rg = DenseGrid(rep, axes)
    rg.evaluate(kernel="factored")
    _check_every_mask(rg, "smoke repeats 3x2x4x2x5")
    rg.evaluate(kernel="direct")  # another evaluation on the same handle: the reduction follows it
    _check_every_mask(rg, "smoke repeats 3x2x4x2x5, K-direct")


def test_every_mask_exact_with_minus_inf_cells_on_h10k_rep(hip_lib):
    from covest_amd import DenseGrid, RepeatsModel
    m = RepeatsModel(21, 100, load_hist("H10k_rep"), 0, max_error=8, device=0)
    g = DenseGrid(m, _thin_c3())
    assert g.total == 16384 <= 20000
    g.evaluate()
    ll, stats = _check_every_mask(g, "H10k_rep, thinned C3")
    assert np.isneginf(ll).sum() > g.total // 4 and np.isfinite(ll).sum() > g.total // 4  # the grid is what the case wants
    assert stats["empty"] > 0  # whole cells without a point below +inf
    # 2. keep nothing = the arg-min pair; keep everything = -LL itself with its own index
    v, i = g.axis_minima(())
    assert v.shape == () and (float(v), int(i)) == g.argmin()
    v, i = g.axis_minima(range(5))
    with np.errstate(invalid="ignore"):
        neg = -ll
    below = neg < np.inf
    assert _bit_equal(v.reshape(-1), np.where(below, neg, np.inf))
    assert np.array_equal(i.reshape(-1), np.where(below, np.arange(g.total), -1))
    assert g.axis_minima(("coverage", "q"))[0].shape == (8, 16)  # names and numbers alike
    assert np.array_equal(g.axis_minima(("q", "coverage"))[1], g.axis_minima((0, 4))[1])


def test_every_mask_exact_with_a_fixed_parameter_and_exact_ties(hip_lib):
    from covest_amd import DenseGrid
    basic, rep = _sim_models()
    g = DenseGrid(basic, [np.linspace(9.0, 11.0, 37), np.array([0.05])])  # a length-1 axis: a fixed parameter
    g.evaluate()
    _check_every_mask(g, "basic 37x1")
    g2 = DenseGrid(basic, [np.array([10.0]), np.linspace(0.01, 0.09, 300)])
    g2.evaluate()
    _check_every_mask(g2, "basic 1x300")
    # q1 = 1.0: q2 and q do not enter the value, so whole runs of points are EXACTLY equal -- the lowest index wins
    axes = [np.linspace(9.0, 11.0, 5), np.array([0.04, 0.05]), np.array([0.6, 1.0]), np.array([0.2, 0.5, 0.9]),
            np.linspace(0.1, 0.9, 7)]
    rg = DenseGrid(rep, axes)
    rg.evaluate()
    ll, _ = _check_every_mask(rg, "repeats with q1 = 1.0")
    cells = ll.reshape(5, 2, 2, 21)  # (c, e, q1) cells of 21 (q2, q) nodes
    ties = int(((cells == cells.max(axis=3, keepdims=True)).sum(axis=3) > 1).sum())
    print("repeats with q1 = 1.0: %d of 20 (c, e, q1) cells hold an exact tie for the minimum" % ties)
    assert ties > 0
    # ... and ties that hold whatever the kernel: an axis that names a value twice, every point a wave of its own
    dg = DenseGrid(basic, [np.array([10.0, 11.0, 10.0, 10.0, 11.0]), np.array([0.05, 0.04, 0.05])])
    dg.evaluate(kernel="direct")
    dll, _ = _check_every_mask(dg, "basic with repeated axis values")
    assert dll[0] == dll[2] == dll[6] == dll[8] == dll[9] and dg.axis_minima(())[1] == dg.argmin()[1]


# ----------------------------------------------------------------------------- 3
BLOCK_MASKS = [(0, 1), (0,), (4,), (1, 3)]  # (c,e), (c), (q), (e,q2)


def test_blocks_that_split_cells_merge_to_the_whole(hip_lib):
    from covest_amd import DenseGrid, RepeatsModel
    from covest_amd.grid import DeviceBlocks, merge_axis_minima
    m = RepeatsModel(21, 100, load_hist("H10k_rep"), 0, max_error=8, device=0)
    axes = _thin_c3()
    whole = DenseGrid(m, axes)
    whole.evaluate()
    bounds = [0, 4097, 11111, 16384]  # uneven, inside (c, e) rows of 256 points
    blocks = [DenseGrid(m, axes, (a, b)) for a, b in zip(bounds[:-1], bounds[1:])]
    for b in blocks:
        b.evaluate()
    devs = DeviceBlocks(m, axes, [0, 0])
    devs.evaluate()
    for keep in BLOCK_MASKS:
        want_v, want_i = whole.axis_minima(keep)
        parts = [b.axis_minima(keep) for b in blocks]
        for b, (pv, pi) in zip(blocks, parts):  # a block alone is exact too: only its own points, global indices
            bv, bi = numpy_axis_minima(b.loglikelihoods(), b.shape, keep, b.flat_range[0])
            assert _bit_equal(pv, bv) and np.array_equal(pi, bi), (keep, b.flat_range)
        got_v, got_i = merge_axis_minima(parts)
        assert _bit_equal(got_v, want_v) and np.array_equal(got_i, want_i), keep
        dv, di = devs.axis_minima(keep)
        assert _bit_equal(dv, want_v) and np.array_equal(di, want_i), keep
    empty = DenseGrid(m, axes, (777, 777))  # a block without a point
    empty.evaluate()
    v, i = empty.axis_minima((0, 1))
    assert np.all(v == np.inf) and np.all(i == -1)
    devs.close()


# ----------------------------------------------------------------------------- 4
def test_calling_order_and_nothing_else_changes(hip_lib):
    from covest_amd import DenseGrid, _capi
    basic, rep = _sim_models()
    axes = [np.array([9.0, 10.0, 11.0]), np.array([0.03, 0.05]), np.linspace(0.4, 0.95, 4), np.array([0.2, 0.6]),
            np.linspace(0.05, 0.9, 5)]
    g = DenseGrid(rep, axes)
    with pytest.raises(_capi.CovestHipError):
        g.axis_minima((0,))  # no evaluation yet
    g.evaluate(scan_start=1e300)
    before = (g.argmin(), g.scan_records(), g.launch_record(), g.loglikelihoods().tobytes())
    for keep in [(0, 1), (), (4,), (0, 1, 2, 3, 4), (0, 1)]:  # repeated calls with different masks are independent
        first = g.axis_minima(keep)
        again = g.axis_minima(keep)
        assert _bit_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    after = (g.argmin(), g.scan_records(), g.launch_record(), g.loglikelihoods().tobytes())
    assert before == after
    assert not any("axis_min" in n for n in before[2]["launches"]) and not any("axis_min" in n for n in _capi.compiled_variants())
    g.reset(axes)
    with pytest.raises(_capi.CovestHipError):
        g.axis_minima((0,))  # a reset without an evaluation
    g.evaluate()
    assert g.axis_minima((0,))[0].shape == (3,)
    # the C ABI's own checks: a mask bit at or above n_axes, n_cells not the product of the kept lengths
    import ctypes
    L = _capi.lib()
    v, i = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)()
    assert L.covest_grid_axis_min(g._handle, 1 << 5, 1, v, i) == _capi.COVEST_E_INVALID
    assert L.covest_grid_axis_min(g._handle, 3, 5, v, i) == _capi.COVEST_E_INVALID
    assert L.covest_grid_axis_min(g._handle, 3, 6, v, i) == 0
    bg = DenseGrid(basic, [np.linspace(8.0, 12.0, 5), np.linspace(0.01, 0.09, 4)])
    bg.evaluate()
    assert L.covest_grid_axis_min(bg._handle, 4, 1, v, i) == _capi.COVEST_E_INVALID  # axis 2 of a two-axis grid
    assert L.covest_abi_version() == 1


# ----------------------------------------------------------------------------- 5
def _golden_model(case):
    from covest_amd import BasicModel, RepeatsModel
    fix = load_golden("axis_min.json")
    cls = RepeatsModel if case["model"] == "repeats" else BasicModel
    return cls(fix["k"], fix["r"], load_hist(fix["hist"]), case["tail"], max_error=fix["max_error"], device=0)


# The cases the check was set for -- the repeat model at tail 0 and tail 1000 and the basic model (tail 0) -- are held
# to the suite's plain 1e-9.  The basic model WITH a tail is a case added here, and for it the plain 1e-9 is not a
# bound the reference itself supports: its term tail * log(1 - sp_j) (covest/models.py:103-104) hangs on the last bits
# of sp_j = fsum(p_j) where 1 - sp_j is tiny, and on this histogram 1 - sp_j is 5e-14 .. 6e-8 at 32 of the 63 nodes
# (the fixture holds the sp_j the reference saw).  Two correct double-precision evaluations of p_j differ by rounding,
# so the bound there is the one the parity suite uses for every tail case (tests/parity_helpers.py _tail_slack: K eps
# n_keys of error in sp_j carried through the log, computed from the REFERENCE's sp_j alone), on top of the 1e-9; how
# many points may fall under it is the count the fixture's generator took from the reference's numbers.  Indices get
# no slack in any case.
GRADED_TAIL = {"repeats_tail0": False, "repeats_tail1000": False, "basic_tail0": False, "basic_tail1000": True}


@pytest.mark.parametrize("name", sorted(GRADED_TAIL))
def test_against_the_reference(hip_lib, name):
    """Minima at the suite's 1e-9 relative; an index identical unless the reference's runner-up of the cell lies within
    2e-9 relative of its winner (then either is accepted); such cells at most 1 % of a mask's cells, re-asserted here
    from the fixture.  basic_tail1000 alone: a minimum beyond 1e-9 passes if it is within the graded tail slack of the
    reference's winning point (see GRADED_TAIL above).

    Measured on an MI355X: repeats_tail0, repeats_tail1000, basic_tail0 -- worst minimum 1.4e-12, 1.4e-12, 1.8e-15
    relative; every index identical in all four cases, no near-tie cell.  basic_tail1000: mask (c,e) worst 1.76e-6 with
    10 of 63 cells beyond 1e-9, mask (e) 7.4e-8 with 1 of 7, mask (c) 2.9e-10 -- the likelihood kernel's value against
    the reference's where the tail term is ill-conditioned; the selection itself is bit-exact (tests above)."""
    from covest_amd import DenseGrid
    from parity_helpers import _slack_of
    fix = load_golden("axis_min.json")
    case = fix["cases"][name]
    axes = [np.array(a) for a in fix["axes"]][:len(case["shape"])]
    assert [len(a) for a in axes] == case["shape"]
    slack = None
    if GRADED_TAIL[name]:
        slack = _slack_of(case["tail"], case["ll"], case["sp"], len(load_hist(fix["hist"])))
        budget = case["tail_slack"]
        assert budget["points"] == len(case["ll"])
        assert sum(c == "graded" for c in slack.classes) <= budget["graded"] and sum(c == "flip" for c in slack.classes) <= budget["flip"]
    m = _golden_model(case)
    g = DenseGrid(m, axes)
    g.evaluate()
    ll = g.loglikelihoods()
    print("%s: worst relative error of a point's LL against the reference: %.3g" % (
        name, max(rel_err(float(a), float(b)) for a, b in zip(ll, case["ll"]))))
    failures = []
    for label, mask in case["masks"].items():
        keep = tuple(mask["keep"])
        want_v, want_i = np.array(mask["negll"]), np.array(mask["index"])
        ru_v = np.array([np.inf if v is None else v for v in mask["runner_up_negll"]])
        ru_i = np.array(mask["runner_up_index"])
        near = (ru_i >= 0) & (np.abs(ru_v - want_v) <= fix["near_tie"] * np.abs(want_v))
        assert mask["cells"] == want_v.size and fix["near_tie"] == 2e-9 and fix["near_tie_cap"] == 0.01
        assert int(near.sum()) == mask["near_ties"] and near.sum() <= 0.01 * want_v.size
        got_v, got_i = g.axis_minima(keep)
        got_v, got_i = got_v.reshape(-1), got_i.reshape(-1)
        errs = [rel_err(float(a), float(b)) for a, b in zip(got_v, want_v)]
        beyond = [c for c, e in enumerate(errs) if e > 1e-9]
        # (graded case: the slack of the reference's winning point, an absolute difference)
        missed = [c for c in beyond if slack is None or not (slack[want_i[c]] > 0 and abs(got_v[c] - want_v[c]) <= slack[want_i[c]])]
        ok = (got_i == want_i) | (near & (got_i == ru_i))
        print("%s mask (%s): %d cells, worst relative error of a minimum %.3g (%d cells beyond 1e-9, %d of them outside the "
              "tail slack), %d indices differ, %d near-tie cells" % (
                  name, label, want_v.size, max(errs), len(beyond), len(missed), int((got_i != want_i).sum()), int(near.sum())))
        if slack is not None and beyond:
            print("   largest share of the tail slack used: %.2g" % max(
                abs(got_v[c] - want_v[c]) / slack[want_i[c]] for c in beyond if slack[want_i[c]] > 0))
        if missed:
            failures.append((label, "minimum", max(errs[c] for c in missed)))
        if not ok.all():
            failures.append((label, "index", np.flatnonzero(~ok)[:8].tolist()))
    assert not failures, (name, failures)


# ----------------------------------------------------------------------------- 6
def _bracket(prof, threshold, best, step):
    """(last node inside, first node outside) going `step` from the minimum, as likelihood_interval walks."""
    i = best
    while prof[i + step] <= threshold:
        i += step
    return i, i + step


def test_coverage_interval_end_to_end(hip_lib, oracle):
    from scipy.stats import chi2
    from covest_amd import BasicModel, coverage_interval, likelihood_interval, print_output
    hist = load_hist("sim_c10_e0.05")
    c0, e0 = 10.0190776, 0.0499923  # the golden optimum
    cs, es = np.linspace(0.98 * c0, 1.02 * c0, 201), np.linspace(0.96 * e0, 1.04 * e0, 41)
    m = BasicModel(21, 100, hist, 0, max_error=8, device=0)
    got = coverage_interval(m, (c0, e0), [cs, es], hist_orig=hist)
    lo, hi = got["coverage_interval"]
    assert lo is not None and hi is not None and lo < c0 < hi
    om = oracle.OracleModel("basic", 21, 100, hist, 0, max_error=8)
    pts = np.array(list(itertools.product(cs, es)))
    prof = (-om.compute_loglikelihood_many(pts, n_threads=16)).reshape(len(cs), len(es)).min(axis=1)
    want_lo, want_hi, want_at = likelihood_interval(cs, prof)
    best = int(np.argmin(prof))
    threshold = prof[best] + 0.5 * chi2.ppf(0.95, 1)
    for label, g, w, step in (("lower", lo, want_lo, -1), ("upper", hi, want_hi, +1)):
        i, j = _bracket(prof, threshold, best, step)
        slope = abs((prof[j] - prof[i]) / (cs[j] - cs[i]))
        tol = 2e-9 * abs(prof[best]) / slope  # 1e-9 on each of the two interpolated values, through the interpolation
        print("%s endpoint: got %.9f want %.9f, |diff| %.3g, tolerance %.3g (slope %.4g per unit of c, nodes %d/%d)" % (
            label, g, w, abs(g - w), tol, slope, i, j))
        assert abs(g - w) <= tol, (label, g, w, tol)
    assert got["coverage_argmin"] == want_at and got["level"] == 0.95
    # the genome size follows endpoint by endpoint, the order reversed
    occurrences = sum(i * n for i, n in hist.items())
    assert got["genome_size_interval"] == (round(occurrences / m.correct_c(hi)), round(occurrences / m.correct_c(lo)))
    rec = print_output(hist, m, True, 1, estimated=(c0, e0), silent=True, intervals=got)
    assert rec["genome_size_interval"][0] <= rec["genome_size"] <= rec["genome_size_interval"][1]
    assert rec["coverage_interval"][0] < rec["coverage"] < rec["coverage_interval"][1] and rec["interval_level"] == 0.95
