"""Every compiled instantiation of the likelihood kernels, reached on purpose and proven to have run.

Each case names the instantiations and K-factored plan features it must reach; the launch record of the evaluation
(covest_grid_launch_record / covest_model_launch_record, include/covest_amd.h) must show them.  Then the values: the
whole grid or list against K-direct at 1e-10 relative (IEEE specials in the same places), a seeded sample against the
oracle at 1e-9 with the graded tail slack (tests/parity_helpers.py), the arg-min against K-direct's, and -- for grids
-- ragged flat-range blocks bit-identical to the whole grid.  Each family's test ends by asserting that what its cases
observed covers the family's share of covest_compiled_variants(): an instantiation added later fails here until a
case reaches it.
"""
import math
import zlib

import numpy as np
import pytest

from conftest import load_hist, rel_err
from parity_helpers import TOL, _check, _slack_budget, _tail_noise

SUBNORMAL = 2.2250738585072014e-308

# which family answers for which compiled instantiation (K-factored's variants are the grid family's: a point list
# reaches only the 512-thread, non-plain ones)
FAMILIES = {
    "factored grids": lambda n: n.startswith("ll_factored<") or n == "ll_finish_dense",
    "factored point lists": lambda n: n == "ll_finish_partials",
    "basic and hand-back": lambda n: n.startswith(("ll_basic<", "fix_")),
    "arg-min": lambda n: n.startswith("argmin_"),
    "derivatives": lambda n: n.startswith("ll_deriv"),
}


def _falling(keys, top):
    return {int(j): max(1, int(top * math.exp(-0.07 * i))) for i, j in enumerate(keys)}


def _share(family):
    from covest_amd import _capi
    return {n for n in _capi.compiled_variants() if FAMILIES[family](n)}


def _observe(observed, case, rec):
    for name, count in rec["launches"].items():
        observed.setdefault(name, []).append((case, count))


def _report(family, observed):
    share = _share(family)
    print("\n%s: instantiations observed (launches, cases)" % family)
    for name in sorted(share | {n for n in observed if FAMILIES[family](n)}):
        seen = observed.get(name, [])
        print("  %-36s %6d launches in %2d cases%s" % (name, sum(c for _, c in seen), len(seen), "" if seen else "  NEVER"))
    got = {n for n in observed if FAMILIES[family](n)}
    assert got == share, "%s: never reached %s" % (family, sorted(share - got))


def _sample(name, total, k=16):
    """A seeded sample of flat indices (the seed is the case's name: the same points on every box)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(rng.choice(total, size=min(k, total), replace=False))


def _points(axes, flat):
    shape = tuple(len(a) for a in axes)
    return np.array([[float(a[i]) for a, i in zip(axes, np.unravel_index(int(f), shape))] for f in flat])


def _against_oracle(om, pts, got, tail, name):
    want = om.compute_loglikelihood_many(pts, n_threads=16)
    slack = _tail_noise(om, pts, want, tail)
    _slack_budget(name, slack)
    _check(got, want, name + " vs oracle", slack=slack)


def _against_direct(om, fast, ref, tail, name, pts_of):
    """The whole of `fast` against K-direct's `ref`: specials in the same places, finite values at 1e-10 -- or, where
    the tail term is ill-conditioned, within the graded slack from the oracle's sp_j (pts_of(indices) -> points)."""
    assert np.array_equal(np.isneginf(fast), np.isneginf(ref)) and np.array_equal(np.isnan(fast), np.isnan(ref)), name
    assert np.array_equal(np.isposinf(fast), np.isposinf(ref)), name
    off = [int(i) for i in np.flatnonzero(np.isfinite(ref)) if rel_err(float(fast[i]), float(ref[i])) > 1e-10]
    slack = [0.0] * len(ref)
    if off and tail:
        for i, s in zip(off, _tail_noise(om, pts_of(off), ref[off], tail)):
            slack[i] = s
    _check(fast, ref, name + " vs direct", tol=1e-10, slack=slack)


def _same_winner(a, b, ref):
    """Arg-min a (fast kernel) against b (K-direct): the same index, or -- only where the two candidates' K-direct
    values are within the 1e-10 the values may differ by -- a near tie either may win."""
    return a == b or (a >= 0 and b >= 0 and rel_err(float(ref[a]), float(ref[b])) <= 1e-10)


def _grid_case(m, om, axes, kernel, tail, name, launches, plan_ok, observed, n_blocks=3, block_ulps=0):
    from covest_amd import DenseGrid
    fac = DenseGrid(m, axes)
    fac.evaluate(kernel=kernel)
    rec = fac.launch_record()
    missing = set(launches) - set(rec["launches"])
    assert not missing, (name, sorted(missing), rec)
    assert plan_ok(rec["plans"]), (name, rec["plans"])
    _observe(observed, name, rec)
    ll, best = fac.loglikelihoods(), fac.argmin()
    ref = DenseGrid(m, axes)
    ref.evaluate(kernel="direct")
    rll, rbest = ref.loglikelihoods(), ref.argmin()
    _against_direct(om, ll, rll, tail, name, lambda idx: _points(axes, idx))
    assert _same_winner(best[1], rbest[1], rll), (name, best, rbest)
    sel = _sample(name, fac.total)
    _against_oracle(om, _points(axes, sel), ll[sel], tail, name)
    # ragged blocks of the flat range: the same plan, the same bits
    cuts = [0] + sorted(int(c) for c in _sample(name + " cuts", fac.total - 2, n_blocks - 1) + 1) + [fac.total]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        blk = DenseGrid(m, axes, flat_range=(lo, hi))
        blk.evaluate(kernel=kernel)
        parts.append(blk.loglikelihoods())
        blk.close()
    blocks = np.concatenate(parts)
    if block_ulps == 0:
        assert np.array_equal(blocks, ll, equal_nan=True), name
    else:
        assert np.array_equal(np.isfinite(blocks), np.isfinite(ll)) and np.array_equal(blocks[~np.isfinite(ll)],
                                                                                     ll[~np.isfinite(ll)], equal_nan=True), name
        fin = np.isfinite(ll)
        assert np.all(np.abs(blocks[fin] - ll[fin]) <= block_ulps * np.spacing(np.abs(ll[fin]))), name
    fac.close()
    ref.close()
    return rec, ll


# ---- K-factored, dense grids ------------------------------------------------------------------------------------------
# (name, histogram, tail, max_error, k, axes, instantiations, plan predicate).  threshold_o is capped by the largest key,
# which sets the row stride ld = roundup32(columns) + 2: keys to 32 -> 34, to 64 -> 66, to 280 -> 290 (kLdWide, the band
# of largest threshold_o - 1 in 257..288), to 450 -> one LDS buffer (ld > 320).
H60 = _falling(range(1, 61), 20000)
H280 = {**_falling(range(1, 41), 20000), 280: 2}
H450 = {**_falling(range(1, 41), 20000), 450: 2}
H1600 = {**_falling(range(1, 61), 20000), 1600: 3}
SPO_AXES = [np.exp(np.linspace(np.log(0.01), np.log(30.0), 16)), np.linspace(0.01, 0.12, 12)]
Q216 = [np.linspace(0.0, 1.0, 6), np.linspace(0.0, 1.0, 6), np.linspace(0.5, 0.95, 6)]
FEW = [np.array([5.0, 9.0]), np.array([0.03, 0.06]), np.linspace(0.4, 0.9, 4), np.array([0.5]), np.linspace(0.3, 0.9, 8)]
FEW10 = [np.array([6.0]), np.array([0.1, 0.4]), np.array([0.5, 0.8]), np.array([0.5]), np.linspace(0.1, 0.9, 5)]
MANY = [np.array([20.0, 31.0]), np.array([0.01, 0.04]), np.linspace(0.3, 0.9, 7), np.linspace(0.0, 1.0, 6),
        np.linspace(0.08, 0.9, 16)]
WIDE = [np.array([9.0, 16.0]), np.array([0.02, 0.1]), np.linspace(0.3, 0.9, 4), np.array([0.2, 0.7]),
        np.array([0.03, 0.2, 0.5, 0.9])]
LONG = [np.array([0.8, 1.5]), np.array([0.02]), np.linspace(0.5, 0.9, 4), np.array([0.3, 0.7]),
        np.array([0.0105, 0.012, 0.2, 0.6])]
SHARED = [np.array([14.0, 27.0]), np.array([0.01, 0.06]), np.linspace(0.3, 0.95, 4), np.linspace(0.05, 0.9, 4),
          np.array([0.04, 0.07, 0.15, 0.33, 0.6, 0.97])]
UNSHARED = [SHARED[0], SHARED[1], np.linspace(0.3, 0.95, 3), np.linspace(0.05, 0.9, 3), SHARED[4]]


def _plan(**want):
    """The record holds a plan with every field as given (callables: a predicate of the field)."""
    def ok(plans):
        return any(all(v(p[k]) if callable(v) else p[k] == v for k, v in want.items()) for p in plans)
    return ok


def _all(*preds):
    return lambda plans: all(p(plans) for p in preds)


MULTI_Q = lambda v: v > 1
FACTORED_CASES = [
    ("256 threads plain", H60, 0, 8, 21, FEW, ["ll_factored<256,plain>"], _plan(n_threads=256, list_mode=0, n_pass=1)),
    ("256 threads plain tail", H60, 5, 8, 21, FEW, ["ll_factored<256,tail,plain>"], _plan(n_threads=256, n_pass=1)),
    ("256 threads 12 classes", H60, 0, 12, 21, FEW10, ["ll_factored<256>"], _plan(n_threads=256, n_pass=2)),
    ("256 threads 16 classes tail", H60, 3, 16, 21, FEW10, ["ll_factored<256,tail>"], _plan(n_threads=256, n_pass=2)),
    ("22 classes", H60, 0, 22, 21, MANY, ["ll_factored<512>"], _plan(n_threads=512, n_pass=3, n_qblocks=MULTI_Q)),
    ("22 classes tail", H60, 7, 22, 21, MANY, ["ll_factored<512,tail>"], _plan(n_threads=512, n_pass=3)),
    ("32 classes k31", H60, 0, 32, 31, MANY, ["ll_factored<512>"], _plan(n_pass=4, n_qblocks=MULTI_Q)),
    ("32 classes k31 tail", H60, 4, 32, 31, MANY, ["ll_factored<512,tail>"], _plan(n_pass=4)),
    ("kLdWide band", H280, 0, 8, 21, WIDE, ["ll_factored<512,plain,ld290>"], _plan(ld=290, n_buf=2, n_pass=1)),
    ("kLdWide band tail", H280, 6, 8, 21, WIDE, ["ll_factored<512,tail,plain,ld290>"], _plan(ld=290, n_buf=2)),
    ("single buffer", H450, 0, 8, 21, WIDE, ["ll_factored<512,plain>"], _plan(n_buf=1, n_threads=512)),
    ("single buffer tail", H450, 5, 8, 21, WIDE, ["ll_factored<512,tail,plain>"], _plan(n_buf=1, n_threads=512)),
    ("q-blocks", H60, 0, 8, 21, MANY, ["ll_factored<512,plain>"], _plan(n_threads=512, n_qblocks=MULTI_Q, ld=66)),
    ("shared steps", H60, 0, 8, 21, SHARED, [], _plan(shared_tiles=MULTI_Q, list_mode=0)),
    ("shared steps tail", H60, 7, 8, 21, SHARED, [], _plan(shared_tiles=MULTI_Q, list_mode=0)),
    ("no shared steps", H60, 0, 8, 21, UNSHARED, [], _plan(shared_tiles=0, list_mode=0)),
    ("long parts S8", H1600, 0, 8, 21, LONG, ["ll_factored<512>", "ll_finish_dense"],
     _all(_plan(long=1, list_mode=3, n_pass=1), _plan(long=0, list_mode=0))),
    ("long parts S8 tail", H1600, 3, 8, 21, LONG, ["ll_factored<512,tail>", "ll_finish_dense"],
     _all(_plan(long=1, list_mode=3, n_pass=1), _plan(long=0, list_mode=0))),
    ("long parts S22", H1600, 0, 22, 21, LONG, ["ll_factored<512>", "ll_finish_dense"], _plan(long=1, n_pass=3)),
    ("long parts S22 tail", H1600, 3, 22, 21, LONG, ["ll_factored<512,tail>", "ll_finish_dense"], _plan(long=1, n_pass=3)),
]
# the small row strides of the SPO parts (a plain grid with a tail, 512 threads): ld 34 and 66, each with key tiles of
# both parities (the walk ends in either buffer), and the same shapes without a tail
# (the q axis sets the largest threshold_o: ld 34 from q = 0.5 on, 66 from q = 0.3 on)
for _keys, _ld, _q0 in ((32, 34, 0.5), (64, 34, 0.5), (96, 66, 0.3), (128, 66, 0.3)):
    for _tail in (5, 0):
        FACTORED_CASES.append(("SPO ld %d, %d keys%s" % (_ld, _keys, " tail" if _tail else ""),
                               _falling(range(1, _keys + 1), 20000), _tail, 8, 21,
                               SPO_AXES + Q216[:2] + [np.linspace(_q0, 0.95, 6)],
                               ["ll_factored<512,tail,plain>" if _tail else "ll_factored<512,plain>"],
                               _plan(n_threads=512, ld=_ld, n_buf=2, n_pass=1)))


@pytest.mark.gpu
def test_factored_grid_variants(hip_lib, oracle):
    from covest_amd import RepeatsModel
    observed = {}
    for name, hist, tail, S, k, axes, launches, plan_ok in FACTORED_CASES:
        m = RepeatsModel(k, 100, hist, tail, max_error=S)
        om = oracle.OracleModel("repeats", k, 100, hist, tail, max_error=S)
        _grid_case(m, om, axes, "factored", tail, "variants: " + name, launches + ["fix_list<5,1>"], plan_ok, observed)
        m.close()
    # past the launch split (2^22 / n_qblocks (c, e) rows a launch): 2 049 x 2 049 rows, two weight vectors
    hist = _falling(range(1, 21), 5000)
    m = RepeatsModel(21, 100, hist, 0, max_error=8)
    om = oracle.OracleModel("repeats", 21, 100, hist, 0, max_error=8)
    axes = [np.linspace(0.5, 30.0, 2049), np.linspace(0.001, 0.2, 2049), [0.7], [0.5], [0.3, 0.8]]
    rec, _ = _grid_case(m, om, axes, "factored", 0, "variants: launch split", [], _plan(n_qblocks=1), observed,
                        n_blocks=2)
    assert sum(c for n, c in rec["launches"].items() if n.startswith("ll_factored<")) > 1, rec
    m.close()
    _report("factored grids", observed)


# ---- K-factored, point lists ------------------------------------------------------------------------------------------
def _list_points(seed, n, c_hi):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0.5, c_hi, n), rng.uniform(0.005, 0.15, n), rng.uniform(0.3, 1.0, n),
                            rng.uniform(0.0, 1.0, n), np.concatenate([rng.uniform(0.006, 0.02, n // 2),
                                                                      rng.uniform(0.1, 0.95, n - n // 2)])])


@pytest.mark.gpu
def test_factored_point_list_variants(hip_lib, oracle):
    """List mode 1 (a point's threshold_o - 1 within a workgroup's 512 lanes) and list mode 2 (beyond: chunks of 512
    copy numbers, ll_finish_partials), each with and without a tail, in one call."""
    from covest_amd import RepeatsModel
    observed = {}
    hist = {**_falling(range(1, 61), 20000), 700: 3}
    for tail in (0, 4):
        name = "variants: point list%s" % (" tail" if tail else "")
        m = RepeatsModel(21, 100, hist, tail, max_error=8)
        om = oracle.OracleModel("repeats", 21, 100, hist, tail, max_error=8)
        pts = _list_points(17 + tail, 40, 40.0)
        fast = m.loglikelihood_points(pts, kernel="factored")
        rec = m.launch_record()
        want = ["ll_factored<512,tail>" if tail else "ll_factored<512>", "ll_finish_partials"]
        assert set(want) <= set(rec["launches"]), (name, rec)
        assert _plan(list_mode=1)(rec["plans"]) and _plan(list_mode=2)(rec["plans"]), (name, rec["plans"])
        _observe(observed, name, rec)
        ref = m.loglikelihood_points(pts, kernel="direct")
        assert set(m.launch_record()["launches"]) == {"ll_direct"}
        _against_direct(om, fast, ref, tail, name, lambda idx: pts[idx])
        assert _same_winner(oracle.first_min(-fast)[0], oracle.first_min(-ref)[0], ref), name
        sel = _sample(name, len(pts))
        _against_oracle(om, pts[sel], fast[sel], tail, name)
        m.close()
    _report("factored point lists", observed)


# ---- K-basic and the hand-back passes ---------------------------------------------------------------------------------
# (k, max_error) -> streams: 8, 16, 24 (22 classes: fix_list<2,1>; 24 classes, which needs k >= 23 -- a model has at
# most k + 1: the packed kernel), 32 (k = 31).  A key with a
# SUBNORMAL p_j (tests/test_gpu_parity.py test_subnormal_pj_goes_to_the_strict_kernel) on every grid, so that the
# hand-back pass really patches values.
SUB_HIST = {1: 1000, 2: 500, 150: 6000, 151: 40, 153: 7}
BASIC_CASES = [(21, 8, "ll_basic<8%s>", "fix_basic_packed<8>"), (21, 16, "ll_basic<16%s>", "fix_basic_packed<16>"),
               (21, 22, "ll_basic<24%s>", "fix_list<2,1>"), (23, 24, "ll_basic<24%s>", "fix_basic_packed<24>"),
               (31, 32, "ll_basic<32%s>", "fix_basic_packed<32>")]


def _basic_axes(k):
    # (k = 23, 31: about the error-free rates c (r - k + 1) / r (1 - e)^k that k = 21 has on the c axis)
    return [np.linspace(0.50, 0.85, 141) * {21: 1.0, 23: 1.047, 31: 1.265}[k], np.array([0.01, 0.02])]


def _subnormal_points(om, pts, key=150):
    return [i for i, p in enumerate(pts) if 0.0 < om.compute_probabilities(*p)[key] < SUBNORMAL]


@pytest.mark.gpu
def test_basic_and_hand_back_variants(hip_lib, oracle):
    from covest_amd import BasicModel, DenseGrid, RepeatsModel
    observed = {}
    for k, S, basic, fix in BASIC_CASES:
        for tail in (0, 9):
            name = "variants: basic k%d S%d%s" % (k, S, " tail" if tail else "")
            m = BasicModel(k, 100, SUB_HIST, tail, max_error=S)
            om = oracle.OracleModel("basic", k, 100, SUB_HIST, tail, max_error=S)
            axes = _basic_axes(k)
            launches = [basic % (",tail" if tail else ""), fix]
            # (blocks to 2 ulps, not bit for bit: K-basic decides per WAVE whether the rest of the keys go by the closed
            # form or key by key (ll_basic.hip), so a point near that border rounds with the wave it shares, and the
            # blocks' ragged starts regroup the waves -- seen at k = 23 and 31; the same grid evaluated twice is
            # bit-identical, as the list of its points is)
            _, ll = _grid_case(m, om, axes, "recur", tail, name, launches, lambda plans: plans == [], observed,
                               block_ulps=2)
            pts = _points(axes, range(len(ll)))
            sub = _subnormal_points(om, pts)
            assert len(sub) >= 10, (name, len(sub))
            _against_oracle(om, pts[sub], ll[sub], tail, name + " subnormal")
            # the same points as a list
            lst = m.loglikelihood_points(pts, kernel="recur")
            rec = m.launch_record()
            m_again = DenseGrid(m, axes)
            m_again.evaluate(kernel="recur")
            assert np.array_equal(m_again.loglikelihoods(), ll, equal_nan=True), name
            m_again.close()
            assert set(launches) <= set(rec["launches"]), (name, rec)
            _observe(observed, name + " list", rec)
            _check(lst, ll, name + " list vs grid", tol=1e-10)
            _against_oracle(om, pts[sub], lst[sub], tail, name + " list subnormal")
            m.close()
    # the repeats model with more than 8 classes: K-factored hands its points to fix_list<5,1>
    for tail in (0, 9):
        name = "variants: repeats S16%s" % (" tail" if tail else "")
        rm = RepeatsModel(21, 100, SUB_HIST, tail, max_error=16)
        orm = oracle.OracleModel("repeats", 21, 100, SUB_HIST, tail, max_error=16)
        axes = [np.exp(np.linspace(np.log(0.03), np.log(0.8), 60)), [0.01], [0.7, 0.9], [0.5], [0.6, 0.95, 1.0]]
        _, ll = _grid_case(rm, orm, axes, "factored", tail, name, ["fix_list<5,1>"], _plan(n_pass=2), observed)
        pts = _points(axes, range(len(ll)))
        sub = _subnormal_points(orm, pts)
        assert len(sub) >= 10, (name, len(sub))
        _against_oracle(orm, pts[sub], ll[sub], tail, name + " subnormal")
        rm.close()
    _report("basic and hand-back", observed)


# ---- the arg-min paths ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argmin_variants(hip_lib):
    """One workgroup (n <= 16384), two stages (16385, and more than 256 x kArgminBlocks), the scan kernel, each also on
    a block with flat_begin != 0.  Every window holds NaN (a NaN c value), LL = -inf (p_j = 0 at small c), exact ties
    (every c value twice in a row: bit-identical values) and, through K-direct-ref in the reference's overflow band,
    LL = +inf.  The device's (min, index) against first_wins_scan over the values read back; windows where nothing
    wins give -1."""
    from covest_amd import BasicModel, DenseGrid
    from covest_amd.grid import first_wins_scan
    observed = {}
    hist = {1: 5, 2: 3, 10000: 2}
    m = BasicModel(21, 100, hist, 0, max_error=8)
    base = [float("nan"), 0.05, 14600.0, 9000.0, 11000.0, 14900.0, 12500.0, 0.2, 14300.0, 14700.0]
    cs = np.repeat(np.array(base * 1000), 2)  # (each value twice: ties)
    es = np.array([0.001, 0.0015, 0.002, 0.003, 0.004, 0.006, 0.008, 0.01, 0.02, 0.03, 0.05, 0.08, 0.1, 0.2, 0.3, 0.4,
                   0.5, 0.001, 0.0025, 0.0035, 0.0045, 0.007, 0.009, 0.015])  # (0.001 twice)
    doomed = np.repeat(np.array([float("nan"), 0.05, 0.1, 0.2] * 3000), 2)  # LL = -inf or NaN everywhere
    total = len(cs) * len(es)
    for n in (16384, 16385, 256 * 1024 + 7919):
        for begin in (0, 4099):
            assert begin + n <= total
            for kernel, scan in (("direct_ref", None), ("direct", None), ("direct_ref", math.inf)):
                if scan is not None and n > 16384:
                    continue
                name = "arg-min n=%d begin=%d %s%s" % (n, begin, kernel, " scan" if scan is not None else "")
                g = DenseGrid(m, [cs, es], flat_range=(begin, begin + n))
                g.evaluate(kernel=kernel, scan_start=scan)
                rec = g.launch_record()
                want = "argmin_scan_small" if scan is not None else "argmin_small" if n <= 16384 else "argmin_stage1+2"
                assert want in rec["launches"], (name, rec)
                _observe(observed, name, rec)
                ll = g.loglikelihoods()
                vals = -ll
                assert np.isnan(ll).any() and np.isneginf(ll).any(), name
                assert np.isposinf(ll).any() == (kernel == "direct_ref"), name
                # ties: the rows of a c value's two copies are bit-identical (and e = 0.001 twice within a row)
                row = len(es)
                r0 = -(-begin // row)
                r0 += r0 % 2  # (the first copy of a pair whose rows lie inside the window)
                pairs = [(r, r + 1) for r in range(r0, (begin + n) // row - 1, 2)]
                assert pairs, name
                for r, s in pairs:
                    a, b = ll[r * row - begin:(r + 1) * row - begin], ll[s * row - begin:(s + 1) * row - begin]
                    assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, r)
                    assert a[0].view(np.int64) == a[17].view(np.int64), (name, r)
                wmin, warg, _ = first_wins_scan(vals, math.inf, 1)
                got = g.argmin()
                assert got[1] == (warg + begin if warg >= 0 else -1), (name, got, warg)
                assert warg < 0 or got[0] == wmin or (math.isnan(got[0]) and math.isnan(wmin)), (name, got, wmin)
                g.close()
            # nothing wins: -1
            g = DenseGrid(m, [doomed, es], flat_range=(begin, begin + n))
            g.evaluate(kernel="direct")
            ll = g.loglikelihoods()
            assert not (ll > -math.inf).any(), n
            assert first_wins_scan(-ll, math.inf, 1)[1] == -1 and g.argmin()[1] == -1, n
            _observe(observed, "arg-min nothing wins n=%d" % n, g.launch_record())
            g.close()
    m.close()
    _report("arg-min", observed)


# ---- the derivative kernel ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_derivative_variants(hip_lib):
    """ll_deriv<P,mode> for both models and the three modes (value + gradient, + Hessian, + outer product of the scores)
    on the 15-key histogram: each call's record shows its instantiation and ll_deriv_finish, once each and nothing else;
    a call of 16384 + 16384 + 3 points shows three launches of each.  The value beside the derivatives is K-direct's at
    1e-11 (the values themselves: tests/test_gpu_deriv_shapes.py and the three fixtures' tests)."""
    from covest_amd import BasicModel, RepeatsModel
    observed = {}
    hist = load_hist("sim_c10_e0.05")
    modes = (("grad", "loglikelihood_gradient_points"), ("hess", "loglikelihood_hessian_points"),
             ("opg", "loglikelihood_score_outer_points"))
    for cls, P, pts in ((BasicModel, 2, [[10.0, 0.05], [8.0, 0.02]]),
                        (RepeatsModel, 5, [[10.0, 0.05, 0.6, 0.5, 0.3], [8.0, 0.02, 0.8, 0.3, 0.6]])):
        m = cls(21, 100, hist, 0, max_error=8)
        direct = m.loglikelihood_points(pts, kernel="direct")
        for mode, fn in modes:
            name = "ll_deriv<%d,%s>" % (P, mode)
            out = getattr(m, fn)(pts)
            rec = m.launch_record()
            assert rec["launches"] == {name: 1, "ll_deriv_finish": 1} and rec["plans"] == [], (name, rec)
            _observe(observed, "derivatives: " + name, rec)
            _check(out[0], direct, name + " vs direct", tol=1e-11)
            assert all(np.all(np.isfinite(a)) for a in out), name
        big = np.tile(np.array(pts), (16386, 1))[:2 * 16384 + 3]
        ll, _ = m.loglikelihood_gradient_points(big)
        rec = m.launch_record()
        assert rec["launches"] == {"ll_deriv<%d,grad>" % P: 3, "ll_deriv_finish": 3}, rec
        _observe(observed, "derivatives: %d points, P = %d" % (len(big), P), rec)
        assert ll.shape == (len(big),) and np.array_equal(ll[:2], ll[-3:-1]) and ll[-1] == ll[0]
        m.close()
    _report("derivatives", observed)


def test_every_compiled_variant_has_a_family(hip_lib):
    """The families above answer for every compiled instantiation, each for its own."""
    from covest_amd import _capi
    names = _capi.compiled_variants()
    assert len(names) == len(set(names)) >= 29
    for n in names:
        assert sum(1 for f in FAMILIES.values() if f(n)) == 1, n
