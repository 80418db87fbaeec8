"""Repeat-bearing genomes without a device: covest_repeat_plan -- host arithmetic of the library
-- against its numpy restatement (tests/repeat_reference.py) bit for bit, the plan's structure and its family shares,
every refusal of the three entry points and of covest_amd.simulate's wrappers, spectrum_to_q on hand-made spectra, and
that nothing is computed where there is no device."""
import ctypes
import math

import numpy as np
import pytest

import repeat_reference as rr

SEEDS = (0, (1 << 63) + 5)
# (q1, q2, q, max_copies): q1 = 1 (q2 and q without a say), no family of two, the defaults' neighbourhood, a cap that is
# hit (0.5 * 0.5 * 0.95^5 = 19 % of the families beyond 7 copies), everything on max_copies, and max_copies = 1
SETTINGS = ((1.0, 0.5, 0.5, 64), (1.0, 0.0, 1.0, 64), (0.3, 0.0, 1.0, 64), (0.6, 0.5, 0.5, 64), (0.5, 0.5, 0.05, 8),
            (0.0, 0.0, 0.0, 8), (0.6, 0.5, 0.5, 1))


def lib_plan(hip_lib, n_units, q1, q2, q, max_copies, seed, both):
    plan = np.full(n_units, -7, dtype=np.int64)
    n_families = ctypes.c_int64(-7)
    rc = hip_lib.covest_repeat_plan(n_units, q1, q2, q, max_copies, seed, 1 if both else 0, plan.ctypes.data,
                                    ctypes.byref(n_families))
    assert rc == 0, hip_lib.covest_last_error()
    return plan, n_families.value


def copies_of(plan):
    ids, counts = np.unique(plan >> 1, return_counts=True)
    return ids, counts


@pytest.mark.parametrize("n_units", [0, 1, 2, 1000])
def test_plan_equals_the_restatement(hip_lib, n_units):
    from covest_amd import simulate as sim
    for q1, q2, q, max_copies in SETTINGS:
        for both in (True, False):
            for seed in SEEDS:
                want, want_families = rr.plan(n_units, q1, q2, q, seed, max_copies, both)
                got, got_families = lib_plan(hip_lib, n_units, q1, q2, q, max_copies, seed, both)
                where = (n_units, q1, q2, q, max_copies, both, seed)
                assert np.array_equal(got, want) and got_families == want_families, where
                py, py_families = sim.repeat_plan(n_units, q1, q2, q, seed, max_copies, both)
                assert py.dtype == np.int64 and np.array_equal(py, want) and py_families == want_families, where
                if not both:
                    assert (got & 1).all(), where
                elif n_units == 1000:
                    assert 0 < int((got & 1).sum()) < 1000, where


def test_thresholds_by_hand(hip_lib):
    """The thresholds spelled out with plain floats, and the library's copy numbers against them: family f of a plan has
    1 + #{o: t_o <= u_f} units, u_f from one Philox block in plain integers.  The restatement gives the same."""
    cdf = [0.6, 0.6 + 0.4 * 0.5, 0.6 + 0.4 * 0.5 + 0.4 * 0.5 * 0.5]
    cdf.append(cdf[-1] + 0.4 * 0.5 * 0.5 * 0.5)
    cdf.append(cdf[-1] + 0.4 * 0.5 * 0.5 * 0.5 * 0.5)
    t = [int(math.floor(c * 2.0 ** 32)) for c in cdf]
    seed = (9 << 32) | 77
    plan, n_families = lib_plan(hip_lib, 300, 0.6, 0.5, 0.5, 6, seed, True)
    _, counts = copies_of(plan)
    by_hand = []
    for f in range(n_families - 1):                                             # (the last family may be cut)
        u = rr.sr.philox_scalar((f, 0, 0, 4), (77, 9))[0]
        by_hand.append(1 + sum(1 for x in t if x <= u))
    assert counts[:-1].tolist() == by_hand and set(by_hand) == {1, 2, 3, 4, 5, 6}
    assert rr.thresholds(0.6, 0.5, 0.5, 6) == t
    assert rr.thresholds(1.0, 0.5, 0.5, 4) == [1 << 32] * 3 and rr.thresholds(0.0, 0.0, 0.0, 4) == [0] * 3
    assert rr.thresholds(0.3, 0.9, 0.9, 1) == []
    for f in (0, 1, 5, (1 << 32) + 3):
        u = rr.sr.philox_scalar((f & rr.sr.MASK, f >> 32, 0, 4), (77, 9))[0]
        assert int(rr.copy_numbers(f, 1, 0.6, 0.5, 0.5, 6, seed)[0]) == 1 + sum(1 for x in t if x <= u)


def test_plan_structure(hip_lib):
    for q1, q2, q, max_copies in SETTINGS:
        for seed in SEEDS:
            for n_units in (1, 2, 1000):
                plan, n_families = lib_plan(hip_lib, n_units, q1, q2, q, max_copies, seed, True)
                ids, counts = copies_of(plan)
                where = (q1, q2, q, max_copies, seed, n_units)
                assert np.array_equal(ids, np.arange(n_families)), where            # exactly 0 .. n_families - 1
                o = rr.copy_numbers(0, n_families, q1, q2, q, max_copies, seed)
                assert np.array_equal(counts[:-1], o[:-1]) and 1 <= counts[-1] <= o[-1], where
                assert counts.max() <= max_copies, where
                if q1 == 1.0 or max_copies == 1:
                    assert np.array_equal(np.sort(plan >> 1), np.arange(n_units)), where  # a permutation
                if (q1, q2, q) == (0.3, 0.0, 1.0):
                    assert set(counts[:-1].tolist()) <= {1, 3}, where
                    if n_units == 1000:
                        assert set(counts[:-1].tolist()) == {1, 3}, where
                if (q1, q2, q) == (0.0, 0.0, 0.0):
                    assert (counts[:-1] == max_copies).all(), where
                if (q1, q2, q, max_copies) == (0.5, 0.5, 0.05, 8) and n_units == 1000:
                    assert counts.max() == 8, where                                   # the cap is hit
    # the shuffle moves the units: the families are not in order
    plan, _ = lib_plan(hip_lib, 1000, 0.6, 0.5, 0.5, 64, 0, True)
    assert not np.array_equal(plan >> 1, np.sort(plan >> 1))


@pytest.mark.parametrize("seed", [0, 20241018])
def test_family_shares(hip_lib, seed):
    """200 000 units at (0.6, 0.5, 0.5): the share of families with 1, 2 and 3 copies within five binomial standard
    deviations, sqrt(p (1 - p) / F), of the probability the thresholds give (the last family, which may be cut, left
    out).  The library's plan and the restatement are the same families."""
    q1, q2, q, n_units = 0.6, 0.5, 0.5, 200_000
    plan, n_families = lib_plan(hip_lib, n_units, q1, q2, q, 64, seed, True)
    _, counts = copies_of(plan)
    counts = counts[:-1]
    assert np.array_equal(counts, rr.copy_numbers(0, n_families - 1, q1, q2, q, 64, seed))
    t = [0] + rr.thresholds(q1, q2, q, 64)
    F = counts.size
    for o in (1, 2, 3):
        p = (t[o] - t[o - 1]) / 2.0 ** 32
        share = int((counts == o).sum()) / F
        sigma = math.sqrt(p * (1 - p) / F)
        print("seed %d o %d: p %.6f share %.6f = %.2f sigma" % (seed, o, p, share, (share - p) / sigma))
        assert abs(share - p) <= 5 * sigma, (o, p, share, sigma)


def test_c_entry_points_refuse_bad_arguments(hip_lib):
    """COVEST_E_INVALID before any device is looked for; n_units == 0 and n == 0 are COVEST_OK with nothing launched."""
    plan = np.zeros(16, dtype=np.int64)
    nf = ctypes.c_int64(-1)

    def make(n_units=4, q1=0.5, q2=0.5, q=0.5, max_copies=8, out=plan.ctypes.data, fam=ctypes.byref(nf)):
        return hip_lib.covest_repeat_plan(n_units, q1, q2, q, max_copies, 1, 1, out, fam)

    assert make() == 0 and nf.value >= 1
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert make(q1=bad) == -1 and make(q2=bad) == -1 and make(q=bad) == -1
    assert make(max_copies=0) == -1 and make(max_copies=-1) == -1 and make(max_copies=(1 << 20) + 1) == -1
    assert make(n_units=1, max_copies=1 << 20) == 0
    assert make(n_units=-1) == -1
    assert make(n_units=(1 << 40) + 1) == -4 and make(n_units=1 << 62) == -4      # refused, not thrown
    assert make(out=None) == -1 and make(fam=None) == -1
    nf.value = -1
    assert make(n_units=0) == 0 and nf.value == 0
    assert make(n_units=0, out=None) == 0 and make(n_units=0, out=None, fam=None) == 0

    out = np.zeros(64, dtype=np.uint8)
    p, o = plan.ctypes.data, out.ctypes.data

    def host(n_units=4, unit_len=10, n=40, d=0.1, pp=p, op=o):
        return hip_lib.covest_repeat_genome(-1, pp, n_units, unit_len, n, d, 1, op)

    def device(n_units=4, unit_len=10, n=40, d=0.1, pp=p, op=o):
        return hip_lib.covest_repeat_genome_device(-1, pp, n_units, unit_len, n, d, 1, op, None)

    for fn in (host, device):
        assert fn(unit_len=0) == -1 and fn(unit_len=-5) == -1
        assert fn(n=-1) == -1
        assert fn(n=41) == -1 and fn(n_units=3, n=31) == -1 and fn(n_units=0, n=1) == -1   # n > n_units * unit_len
        assert fn(n_units=-1, n=0) == -1
        assert fn(d=-0.1) == -1 and fn(d=1.1) == -1 and fn(d=float("nan")) == -1
        assert fn(pp=None) == -1 and fn(op=None) == -1
        assert fn(n=0) == 0 and fn(n=0, pp=None, op=None) == 0 and fn(n=0, d=1.0) == 0
    neg = plan.copy()
    neg[2] = -2
    assert host(pp=neg.ctypes.data) == -1 and b"negative" in hip_lib.covest_last_error()
    assert host(pp=neg.ctypes.data, n=0) == -1            # the host form looks at the plan whatever n is
    far = plan.copy()
    far[1] = ((1 << 63) // 10) << 1                        # (f + 1) * unit_len beyond 63 bits
    assert host(pp=far.ctypes.data) == -1 and b"63 bits" in hip_lib.covest_last_error()
    assert not out.any()


def test_argument_validation():
    from covest_amd import simulate as sim
    for bad in (-0.01, 1.01, float("nan")):
        for kw in ({"q1": bad}, {"q2": bad}, {"q": bad}):
            args = dict(q1=0.5, q2=0.5, q=0.5)
            args.update(kw)
            with pytest.raises(ValueError):
                sim.repeat_plan(10, seed=1, **args)
            with pytest.raises(ValueError):
                sim.repeat_genome(100, 10, seed=1, **args)
        with pytest.raises(ValueError):
            sim.repeat_genome(100, 10, 0.5, 0.5, 0.5, 1, divergence=bad)
    for bad in (0, -1, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError):
            sim.repeat_plan(10, 0.5, 0.5, 0.5, 1, max_copies=bad)
    with pytest.raises(ValueError):
        sim.repeat_plan(-1, 0.5, 0.5, 0.5, 1)
    with pytest.raises(ValueError):
        sim.repeat_plan(10, 0.5, 0.5, 0.5, 1 << 64)
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 0, 0.5, 0.5, 0.5, 1)
    with pytest.raises(ValueError):
        sim.repeat_genome(-1, 10, 0.5, 0.5, 0.5, 1)
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 10, seed=1)                                     # neither (q1, q2, q) nor a plan
    plan = np.zeros(10, dtype=np.int64)
    with pytest.raises(ValueError):
        sim.repeat_genome(101, 10, plan=plan)                                  # n > n_units * unit_len
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 10, plan=np.array([0, -2] * 5))
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 10, plan=np.array([(1 << 60) << 1] * 10))       # f * unit_len beyond 63 bits
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 10, plan=plan.reshape(2, 5))
    with pytest.raises(ValueError):
        sim.repeat_genome_device(0, 10, 10, 101, 0)
    with pytest.raises(ValueError):
        sim.repeat_genome_device(0, 10, 0, 5, 0)
    with pytest.raises(ValueError):
        sim.repeat_genome_device(0, 10, 10, 100, 0, divergence=2.0)
    with pytest.raises(ValueError):
        sim.genome_spectrum("ACGTN" * 10, 5)
    assert sim.genome_spectrum("ACGT", 5) == {}                                # shorter than k: no k-mer, no device asked


def test_no_cpu_path(hip_lib):
    """Without a device the argument checks come first (ValueError), then CovestHipError: nothing is computed here."""
    from covest_amd import _capi, simulate as sim
    if hip_lib.covest_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(ValueError):
        sim.repeat_genome(100, 10, 0.5, 0.5, 0.5, 1, divergence=1.5)
    with pytest.raises(_capi.CovestHipError):
        sim.repeat_genome(100, 10, 0.5, 0.5, 0.5, 1)
    with pytest.raises(_capi.CovestHipError):
        sim.repeat_genome(100, 10, plan=np.zeros(10, dtype=np.int64))
    with pytest.raises(_capi.CovestHipError):
        sim.genome_spectrum("ACGT" * 10, 5)
    plan, n_families = sim.repeat_plan(10, 0.5, 0.5, 0.5, 1)                   # the plan needs no device
    assert plan.size == 10 and 1 <= n_families <= 10


def test_spectrum_to_q():
    from covest_amd.simulate import spectrum_to_q
    assert spectrum_to_q({1: 70, 2: 15, 3: 10, 4: 5}) == (0.7, 0.5, 15 / 20)
    assert spectrum_to_q({1: 10}) == (1.0, None, None)
    assert spectrum_to_q({}) == (None, None, None)
    assert spectrum_to_q({2: 4}) == (0.0, 1.0, None)
    assert spectrum_to_q({3: 4}) == (0.0, 0.0, 1.0)                            # every tail k-mer at 3 copies: q = 1
    assert spectrum_to_q({1: 1, 5: 2, 10: 1}) == (0.25, 0.0, 3 / (3 * 2 + 8))
    assert spectrum_to_q({1: 5, 2: 0, 7: 0}) == (1.0, None, None)
    # a geometric tail at rate 1/2, cut at 11 copies: N_o = 1024 >> (o - 2)
    assert spectrum_to_q({o: 1024 >> (o - 2) for o in range(3, 12)})[2] == 1022 / 2026
    with pytest.raises(ValueError):
        spectrum_to_q({0: 3})


def test_repeat_genome_record():
    """RepeatGenome over the restatement's arrays (host arithmetic)."""
    from covest_amd.simulate import RepeatGenome
    plan, _ = rr.plan(40, 0.5, 0.5, 0.5, 3)
    bases = rr.genome(plan, 25, 990, 0.0, 3)
    g = RepeatGenome(bases, plan, 25, 0.0, 3)
    assert len(g) == 990 and g.n_units == 40 and g.unit_len == 25
    assert np.array_equal(g.family_of_unit, plan >> 1) and np.array_equal(g.forward, (plan & 1) == 1)
    ids, counts = copies_of(plan)
    assert g.copies() == dict(zip(ids.tolist(), counts.tolist())) and sum(g.copies().values()) == 40
