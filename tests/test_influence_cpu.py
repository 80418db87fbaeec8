"""The delete-one-read influence without a GPU: the identity behind the rows, checked on the plain restatement
(tests/influence_reference.py) against a recount; summarize_influence against the per-read formula; the record; and
the argument errors that are raised before the library is asked."""
import functools
import math

import numpy as np
import pytest

import influence_reference as ir
import kmer_reference as kr
import sim_reference as sr
from covest_amd import influence as infl
from covest_amd.report import print_output

CASE = dict(genome_len=500, seed=20261021, n_reads=200, read_len=40, error_rate=0.01, k=9)


@functools.lru_cache(maxsize=None)
def small_case():
    """(reads as strings, counts) of CASE under sim_reference and kmer_reference alone; canonical keys."""
    c = CASE
    genome = sr.random_genome(c["genome_len"], c["seed"])
    bases, _, _, _ = sr.simulate(genome, c["read_len"], 0, c["n_reads"], c["error_rate"], c["seed"], True)
    reads = tuple(row.tobytes().decode() for row in bases)
    return reads, kr.count(reads, c["k"], True)


def test_identity_for_an_arbitrary_table():
    """Delta_r of the restatement equals sum_x table[a'_x] - sum_x table[a_x] over ALL distinct keys, a' the counts of
    a recount without read r, for a random table (fewer rows than the largest abundance: the clamp takes part)."""
    k = CASE["k"]
    reads, counts = small_case()
    rng = np.random.default_rng(5)
    table = rng.normal(size=(18, 3)) * np.array([1.0, 1e3, 1e-4])
    assert max(counts.values()) > table.shape[0]
    top = table.shape[0] - 1
    repeats = [r for r in range(len(reads)) if any(m > 1 for _, m, _, _ in ir.first_terms(reads[r], counts, k, True, table))]
    assert repeats, "no read repeats a key: the case does not test the multiplicity"
    chosen = (repeats[:6] + [r for r in range(0, len(reads), 10) if r not in repeats[:6]])[:20]
    assert len(chosen) == 20 and len(set(chosen)) == 20
    for r in chosen:
        without = kr.count(reads[:r] + reads[r + 1:], k, True)
        row = ir.influence_row(reads[r], counts, k, True, table)
        bound = ir.row_bound(reads[r], counts, k, True, table)
        assert row[3] == CASE["read_len"] - k + 1
        for col in range(3):
            exact = math.fsum([float(table[min(without.get(x, 0), top)][col]) for x in counts] +
                              [-float(table[min(a, top)][col]) for a in counts.values()])
            assert abs(row[col] - exact) <= bound[col], (r, col, row[col], exact, bound[col])
            assert abs(exact) > 1e6 * bound[col]  # (not vacuous: the row is not rounding noise)


def test_restatement_conventions():
    k = 5
    counts = kr.count(["ACGTACGTAC", "AAAAAAAAA"], k, False)
    table = np.array([[0.0], [1.0], [4.0], [9.0], [16.0], [25.0]])
    rows = ir.influence_rows(["ACGT", "", "AAAAAAAAA", "ACGTACGTAC"], counts, k, False, table)
    assert rows[0].tolist() == [0.0, 0.0] and rows[1].tolist() == [0.0, 0.0]  # shorter than k: zeros, no window
    assert rows[2].tolist() == [table[0, 0] - table[5, 0], 5.0]               # a homopolymer: one key, m = W = 5
    # ACGTA, CGTAC twice each, GTACG, TACGT once: every key vanishes
    assert rows[3].tolist() == [2 * (0.0 - 4.0) + 2 * (0.0 - 1.0), 6.0]
    long_read = "ACGT" * 1025 + "A"
    assert len(long_read) - k + 1 == 4097
    assert np.isnan(ir.influence_row(long_read, counts, k, False, table)[0])
    assert ir.influence_row(long_read, counts, k, False, table)[1] == 4097.0


def hand_info(names, estimate, free, rng):
    """A stand-in for observed_information's dict: a random positive definite covariance of the free block."""
    a = rng.normal(size=(len(free), len(free)))
    cov = a @ a.T + len(free) * np.eye(len(free))
    return {'params': list(names), 'estimate': list(estimate), 'free': list(free), 'covariance': cov.tolist(),
            'reason': None, 'bounds': [(None, None)] * len(names)}


def packed_centred(rows):
    n, q = rows.shape
    mean = rows.sum(axis=0) / n
    d = rows - mean
    full = d.T @ d
    return rows.sum(axis=0), np.array([full[a, b] for a in range(q) for b in range(a, q)])


def correct_c(c):
    return c * 0.8


@pytest.mark.parametrize("names,free,fix", [
    (("coverage", "error_rate"), [0, 1], None),
    (("coverage", "error_rate", "q1", "q2", "q"), [0, 1, 2, 3, 4], None),
    (("coverage", "error_rate", "q1"), [0, 2], [None, 0.05, None]),   # a fixed parameter
    (("coverage", "error_rate", "q1"), [1, 2], [11.0, None, None]),   # the coverage fixed: the genome size goes with it
])
def test_summarize_influence_against_the_per_read_formula(names, free, fix):
    rng = np.random.default_rng(len(names) * 10 + len(free))
    P, n, N = len(names), 57, 123456.0
    estimate = [11.0, 0.05, 0.7, 0.6, 0.5][:P]
    info = hand_info(names, estimate, free, rng)
    rows = np.concatenate([rng.normal(size=(n, P)) * 50.0, rng.integers(0, 80, size=(n, 1)).astype(float)], axis=1)
    total, cross = packed_centred(rows)
    got = infl.summarize_influence(total, cross, n, info, N, names, fix, 0.9, correct_c)

    inverse = np.zeros((P, P))
    inverse[np.ix_(free, free)] = np.asarray(info['covariance'])
    c, S = estimate[0], N / correct_c(estimate[0])
    shifts = np.zeros((n, P + 1))
    for r in range(n):  # the explicit pseudo-shift of every read
        delta = inverse @ rows[r, :P]
        kappa = delta[0] + c * rows[r, P] / N
        shifts[r, :P] = delta
        shifts[r, 0] = kappa
        shifts[r, P] = -S * kappa / c
    mean = shifts.mean(axis=0)
    V = (n - 1) / n * (shifts - mean).T @ (shifts - mean)
    from scipy.stats import norm
    z = norm.ppf(0.95)
    centres = estimate + [S]
    assert got['reads'] == n and got['level'] == 0.9 and got['reason'] is None
    assert got['quantities'] == list(names) + ['genome_size']
    for d, name in enumerate(got['quantities']):
        of = 0 if d == P else d
        if of not in free:
            assert got['standard_errors'][name] is None and got['intervals'][name] is None and got['mean_shift'][name] is None
            continue
        se = math.sqrt(V[d, d])
        assert got['standard_errors'][name] == pytest.approx(se, rel=1e-12)
        assert got['mean_shift'][name] == pytest.approx(mean[d], rel=1e-12, abs=1e-12 * se)
        assert got['intervals'][name] == pytest.approx([centres[d] - z * se, centres[d] + z * se], rel=1e-12)
    if 0 in free:
        assert np.allclose(np.asarray(got['covariance']), V, rtol=1e-12, atol=1e-12 * np.abs(V).max())


def test_summarize_influence_without_a_covariance_and_with_one_read():
    names = ("coverage", "error_rate")
    info = {'params': list(names), 'estimate': [10.0, 0.02], 'free': [0, 1], 'covariance': None,
            'reason': "the information of the free parameters (coverage, error_rate) is not positive definite"}
    got = infl.summarize_influence(np.zeros(3), np.zeros(6), 40, info, 1000.0, names, None, 0.95, correct_c)
    assert got['reason'] == info['reason'] and got['covariance'] is None and got['reads'] == 40
    for key in ('standard_errors', 'intervals', 'mean_shift'):
        assert set(got[key]) == {"coverage", "error_rate", "genome_size"} and all(v is None for v in got[key].values())
    info = hand_info(names, [10.0, 0.02], [0, 1], np.random.default_rng(1))
    one = infl.summarize_influence(np.array([1.0, 2.0, 30.0]), np.zeros(6), 1, info, 1000.0, names, None, 0.95, correct_c)
    assert one['reason'] == "a jackknife needs at least two reads" and one['reads'] == 1
    assert all(v is None for v in one['standard_errors'].values())
    with pytest.raises(ValueError):
        infl.summarize_influence(np.zeros(2), np.zeros(6), 4, info, 1000.0, names, None, 0.95, correct_c)  # P + 1 sums
    with pytest.raises(ValueError):
        infl.summarize_influence(np.zeros(3), np.zeros(5), 4, info, 1000.0, names, None, 0.95, correct_c)
    with pytest.raises(ValueError):
        infl.summarize_influence(np.zeros(3), np.zeros(6), 4, info, 1000.0, names, [None], 0.95, correct_c)
    with pytest.raises(ValueError):
        infl.summarize_influence(np.zeros(3), np.zeros(6), 4, info, 1000.0, names, None, 1.0, correct_c)


class StandInModel:
    params = ("coverage", "error_rate")
    hist = {1: 5, 2: 7, 3: 2}

    @staticmethod
    def short_name():
        return "stand-in"

    @staticmethod
    def correct_c(c):
        return 0.5 * c

    @staticmethod
    def compute_loglikelihood(*args):
        return -1.0


def test_print_output_records_the_summary():
    model = StandInModel()
    hist = dict(model.hist)
    plain = print_output(hist, model, True, 1, estimated=[10.0, 0.02], silent=True)
    assert print_output(hist, model, True, 1, estimated=[10.0, 0.02], silent=True, read_influence=None) == plain
    assert not [key for key in plain if key.startswith("read_influence")]
    summary = {'standard_errors': {'coverage': 0.25, 'error_rate': None, 'genome_size': 3.5},
               'intervals': {'coverage': [9.5, 10.5], 'error_rate': None, 'genome_size': (1.0, 2.0)},
               'reads': 77, 'level': 0.9, 'reason': None}
    record = print_output(hist, model, True, 1, estimated=[10.0, 0.02], silent=True, read_influence=summary)
    added = {"read_influence_reads": 77, "read_influence_level": 0.9, "read_influence_se_coverage": 0.25,
             "read_influence_se_genome_size": 3.5, "read_influence_interval_coverage": [9.5, 10.5],
             "read_influence_interval_genome_size": [1.0, 2.0]}
    assert {key: record[key] for key in plain} == plain
    assert {key: record[key] for key in record if key not in plain} == added

    class Carrier:  # a ReadInfluence is asked for its summary
        @staticmethod
        def summary():
            return dict(summary, reason="no covariance", standard_errors={}, intervals={})
    record = print_output(hist, model, True, 1, estimated=[10.0, 0.02], silent=True, read_influence=Carrier())
    assert {key: record[key] for key in record if key not in plain} == {
        "read_influence_reads": 77, "read_influence_level": 0.9, "read_influence_reason": "no covariance"}


def test_argument_errors_come_before_the_library(monkeypatch):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "lib", no_library)
    counts = KmerCounts.__new__(KmerCounts)
    counts.k, counts.canonical, counts._handle = 5, False, None
    reads = ["ACGTACGT"]
    for table in (np.zeros(3), np.zeros((0, 2)), np.zeros((3, 0)), np.zeros((3, 9)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            counts.read_influence(reads, table)
    with pytest.raises(KeyError):
        counts.read_influence(["ACGN"], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        counts.read_influence((np.zeros(4, dtype=np.uint8), np.array([0, 9])), np.zeros((2, 2)))  # offsets beyond the bases
    for rows in (np.zeros(4), np.zeros((4, 0)), np.zeros((4, 10))):
        with pytest.raises(ValueError):
            infl.rows_moments(rows)
    with pytest.raises(ValueError):
        infl.rows_moments(np.zeros((4, 3)), centre=np.zeros(2))
    for q in (0, 10):
        with pytest.raises(ValueError):
            infl.rows_moments_device(256, 4, q, 256, 256, 256)
    with pytest.raises(ValueError):
        infl.rows_moments_device(256, -1, 3, 256, 256, 256)
    with pytest.raises(ValueError):
        infl.unpack_cross(np.zeros(5), 3)

    class Sampled(StandInModel):
        sample_factor = 2
        k = 5
    with pytest.raises(ValueError, match="sample factor 1"):
        infl.read_influence(Sampled(), [10.0, 0.02], counts, reads)
    model = StandInModel()
    model.k = 5
    with pytest.raises(ValueError, match="2 parameters expected"):
        infl.read_influence(model, [10.0], counts, reads)
    with pytest.raises(ValueError, match="level"):
        infl.read_influence(model, [10.0, 0.02], counts, reads, level=1.5)
    with pytest.raises(ValueError, match="fix"):
        infl.read_influence(model, [10.0, 0.02], counts, reads, fix=[None])
    model.k = 7
    with pytest.raises(ValueError, match="counter's k"):
        infl.read_influence(model, [10.0, 0.02], counts, reads)
    with pytest.raises(ValueError, match="2 parameters expected"):
        infl.score_rows(model, [1.0, 2.0, 3.0])
