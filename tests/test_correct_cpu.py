"""The correction's restatement (tests/correct_reference.py) on hand-made inputs, the argument errors of the Python layer
that are raised before the library is asked, print_output's record with and without corrections=, and the simulated
case of DESIGN.md section 6af under the references alone.  No GPU."""
import numpy as np
import pytest

import correct_reference as cr
import kmer_reference as kr
import lookup_reference as lr


def test_runs_of():
    assert cr.runs_of([]) == []
    assert cr.runs_of([False, False]) == []
    assert cr.runs_of([True]) == [(0, 0)]
    assert cr.runs_of([True, True, False, True, False, False, True, True]) == [(0, 1), (3, 3), (6, 7)]


def covering(p, k, length):
    return max(0, p - k + 1), min(p, length - k)


@pytest.mark.parametrize("k,length", [(1, 1), (1, 5), (3, 3), (3, 4), (3, 5), (5, 9), (5, 20), (7, 12), (7, 13), (7, 14)])
def test_candidate_positions_are_the_bases_with_exactly_these_covering_windows(k, length):
    """Rule 3 against its own definition, for every run [f, l] of every shape: read shorter than 2k - 1, of 2k - 1
    bases, longer."""
    last = length - k
    for f in range(last + 1):
        for l in range(f, last + 1):
            want = [p for p in range(length) if covering(p, k, length) == (f, l)]
            assert cr.candidate_positions(f, l, k, length) == want, (f, l)
    # every base is the candidate of exactly one run
    assert sorted(p for f in range(last + 1) for l in range(f, last + 1)
                  for p in cr.candidate_positions(f, l, k, length)) == list(range(length))


K = 7
G = kr.genome()[:62]  # no 7-mer twice on either strand (the next test)


def test_hand_made_genome_has_no_repeated_window():
    for canonical in (False, True):
        assert set(kr.count([G], K, canonical).values()) == {1}


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("p", [0, 1, K - 2, K - 1, K, 30, 62 - K - 1, 62 - K, 62 - K + 1, 60, 61])
def test_one_substitution_comes_back(p, canonical):
    k = K
    counts = kr.count([G] * 3, k, canonical)
    read = G[:p] + ("A" if G[p] != "A" else "C") + G[p + 1:]
    fixed, row = cr.correct_read(read, counts, k, canonical, 2)
    assert (fixed, row) == (G, (1, 1, 0, 0))
    fixed, row = cr.correct_read(read.lower(), counts, k, canonical, 2)
    assert (fixed, row) == (G.lower(), (1, 1, 0, 0))
    assert cr.correct_read(read, counts, k, canonical, 0) == (read, (0, 0, 0, 0))


def test_two_substitutions_by_distance():
    """k - 1 and k apart: one merged run longer than k, unfixable; k + 1 apart: a strong window between, both corrected."""
    k = K
    counts = kr.count([G] * 3, k)

    def planted(*ps):
        return "".join(("A" if c != "A" else "C") if i in ps else c for i, c in enumerate(G))
    for d in (k - 1, k):
        read = planted(20, 20 + d)
        assert cr.correct_read(read, counts, k, False, 2) == (read, (1, 0, 0, 1))
    assert cr.correct_read(planted(20, 20 + k + 1), counts, k, False, 2) == (G, (2, 2, 0, 0))


def test_ambiguity_and_no_window():
    k = K
    x, y = G[:20], G[21:42]
    both = kr.count([x + "A" + y, x + "C" + y] * 3, k)
    read = x + "G" + y
    assert cr.correct_read(read, both, k, False, 2) == (read, (1, 0, 1, 0))
    only = kr.count([x + "A" + y] * 3, k)
    assert cr.correct_read(read, only, k, False, 2) == (x + "A" + y, (1, 1, 0, 0))
    assert cr.correct_read(read.lower(), only, k, False, 2) == ((x + "A" + y).lower(), (1, 1, 0, 0))
    for short in ("", "ACG", "acgt"):
        assert cr.correct_read(short, only, k, False, 2) == (short, (0, 0, 0, 0))
    # a read of fewer than 2k - 1 bases, wrong in the middle: the whole read is one run, several positions are tried
    counts = kr.count([G] * 3, k)
    clean = G[10:10 + 2 * k - 3]
    read = clean[:k - 2] + ("A" if clean[k - 2] != "A" else "C") + clean[k - 1:]
    assert cr.candidate_positions(0, k - 3, k, len(read)) == [k - 3, k - 2, k - 1]
    assert cr.correct_read(read, counts, k, False, 2) == (clean, (1, 1, 0, 0))
    out, offsets, fix, strings = cr.correct(["", read, "ACG"], counts, k, False, 2)
    assert offsets.tolist() == [0, 0, len(read), len(read) + 3] and out.tobytes().decode() == clean + "ACG"
    assert fix.tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]] and strings == ["", clean, "ACG"]


def test_simulated_case_under_the_reference():
    """the case of lookup_reference.CASE corrected at cutoff 3, every figure pinned."""
    c, want = lr.CASE, cr.CASE_EXPECTED
    _, bases, hit, reads, counts = lr.simulated_case()
    truth = cr.simulated_case_truth()
    assert np.array_equal(bases != truth, hit)
    out, fix, strings = cr.simulated_case_corrected()
    assert fix.sum(axis=0).tolist() == [1624, 1402, 0, 222]
    assert fix.sum(axis=0).tolist() == [want[n] for n in ("runs", "corrected", "ambiguous", "unfixable")]
    assert np.array_equal(fix[:, 0], fix[:, 1:].sum(axis=1))
    assert cr.recovery_figures(bases, out, truth) == (1851, 449, 1396, 218, 0, 0)
    assert cr.recovery_figures(bases, out, truth) == tuple(want[n] for n in (
        "wrong_before", "wrong_after", "reads_wrong_before", "reads_wrong_after", "miscorrected", "reads_worse"))
    assert int((out != bases).sum()) == want["corrected"]
    assert cr.table_figures(counts) == (26989, 20329) == (want["distinct_before"], want["singletons_before"])
    assert cr.table_figures(kr.count(strings, c["k"], True)) == (10260, 4235) == (want["distinct_after"],
                                                                                  want["singletons_after"])


@pytest.mark.parametrize("cutoff", [3, 4, 5, 6, 7])
def test_simulated_case_conditions_at_every_cutoff(cutoff):
    """What must hold for the reference alone: no correction to a base other than the true one, no read with more
    wrong bases after than before, at least 85 % of the runs corrected."""
    _, bases, _, _, _ = lr.simulated_case()
    out, fix, _ = cr.simulated_case_corrected(cutoff)
    runs, corrected = int(fix[:, 0].sum()), int(fix[:, 1].sum())
    *_, miscorrected, worse = cr.recovery_figures(bases, out, cr.simulated_case_truth())
    print("cutoff %d: %d of %d runs corrected (%.4f)" % (cutoff, corrected, runs, corrected / runs))
    assert miscorrected == 0 and worse == 0
    assert corrected >= 0.85 * runs


class _NeverAsked:
    """A KmerCounts without a handle: any call into the library would fail on it."""
    k, _handle = 5, None


def _correct(*args, **kwargs):
    from covest_amd.kmer_hist import KmerCounts
    return KmerCounts.correct(_NeverAsked(), *args, **kwargs)


def test_argument_errors_before_the_library_is_asked(monkeypatch):
    from covest_amd import _capi

    def refuse():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "lib", refuse)
    with pytest.raises(KeyError):
        _correct(["ACGTN"], 2)
    with pytest.raises(ValueError):
        _correct(["ACGT"], -1)
    with pytest.raises(ValueError):
        _correct(["ACGT"], 1 << 32)
    with pytest.raises(ValueError):
        _correct((np.zeros(4, dtype=np.int32), np.array([0, 4])), 2)
    with pytest.raises(ValueError):
        _correct((np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 5])), 2)
    with pytest.raises(TypeError):
        _correct(["ACGT"])  # the cutoff is not optional: there is no correction without one
    got = _correct([], 3)  # no reads: nothing to ask the library for
    assert got.n_reads == 0 and got.bases.size == 0 and got.runs.size == 0 and got.changed.size == 0
    assert got.strings() == [] and got.k == 5 and got.cutoff == 3


def _corrected_reads(level=None):
    from covest_amd.kmer_hist import CorrectedReads
    from covest_amd.read_errors import ReadCorrections
    bases = np.frombuffer(b"ACGTAacgtTT", dtype=np.uint8)
    fix = np.array([[2, 2, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0], [3, 1, 0, 2]], dtype=np.uint32)
    found = CorrectedReads(5, bases, np.array([0, 5, 9, 9, 11]), fix, np.array([1, 3]), 4)
    return found if level is None else ReadCorrections(found, level)


def test_corrected_reads_and_shares():
    found = _corrected_reads()
    assert found.strings() == ["ACGTA", "acgt", "", "TT"] and found.n_reads == 4
    assert found.runs.dtype == np.int64 and found.runs.tolist() == [2, 1, 0, 3]
    assert (found.corrected.tolist(), found.ambiguous.tolist(), found.unfixable.tolist()) == ([2, 0, 0, 1], [0, 1, 0, 0],
                                                                                             [0, 0, 0, 2])
    got = _corrected_reads(0.5)
    assert got.strings() == found.strings() and got.level == 0.5 and got.cutoff == 4 and got.k == 5
    assert got.corrected_share == 0.25 and got.unresolved_share == 0.5


class _StandIn:
    """What print_output touches of a model, without a device."""
    params = ("coverage", "error_rate")
    hist = {1: 8, 2: 4, 3: 2}

    def short_name(self):
        return "basic"

    def correct_c(self, c):
        return c * 0.8

    def compute_loglikelihood(self, *args):
        return -123.5


def test_print_output_record():
    """Without corrections= the record is what it was; with it, six more entries and nothing else changed."""
    from covest_amd import print_output
    hist = dict(_StandIn.hist)
    args = dict(estimated=(10.0, 0.05), silent=True)
    plain = print_output(hist, _StandIn(), True, 1, **args)
    same = print_output(hist, _StandIn(), True, 1, corrections=None, **args)
    assert same == plain and list(same) == list(plain)
    assert not any(key.startswith("corrections") for key in plain)
    names = ("cutoff", "reads", "runs", "corrected", "ambiguous", "unfixable")
    for corrections in (_corrected_reads(), _corrected_reads(0.5)):
        record = print_output(hist, _StandIn(), True, 1, corrections=corrections, **args)
        assert set(record) - set(plain) == {"corrections_" + name for name in names}
        assert {key: record[key] for key in plain} == plain
        assert [record["corrections_" + name] for name in names] == [4, 4, 6, 3, 1, 2]
        assert all(type(record["corrections_" + name]) is int for name in names)
