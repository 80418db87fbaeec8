"""The per-read lookup's restatement (tests/lookup_reference.py) against tests/kmer_reference.py, the numpy helpers of
covest_amd.read_errors on hand-made inputs, the simulated case of DESIGN.md section 6ae under the references alone, and
the argument errors that are raised before the library is asked.  No GPU."""
import math
import random

import numpy as np
import pytest

import kmer_reference as kr
import lookup_reference as lr

NONE = lr.NONE


@pytest.mark.parametrize("k", [1, 12, 13, 31])
@pytest.mark.parametrize("canonical", [False, True])
def test_restatement_against_the_counts(k, canonical):
    """Looking the counted reads up gives every key's count back: per key, the windows that hold it are as many as its
    count (minus what the reads shorter than k added to it), and the layout holds the sentinel where no window starts."""
    reads = kr.sweep_reads(k)
    counts = kr.count(reads, k, canonical)
    abundance, offsets, summary, _ = lr.lookup(reads, counts, k, canonical)
    assert abundance.size == sum(len(r) for r in reads) and offsets[-1] == abundance.size
    seen = {}
    for i, read in enumerate(reads):
        row = abundance[offsets[i]:offsets[i + 1]]
        n_windows = max(len(read) - k + 1, 0)
        assert (row[n_windows:] == NONE).all() and (row[:n_windows] != NONE).all()
        d = kr._digits(read)
        for s in range(n_windows):
            key = kr._key(d[s:s + k], k, canonical)
            assert row[s] == counts[key] and row[s] >= 1
            seen[key] = seen.get(key, 0) + 1
        assert summary[i, 0] == (row[:n_windows].min() if n_windows else NONE)
    short = kr.count([r for r in reads if len(r) < k], k, canonical)
    assert {key: n + short.get(key, 0) for key, n in seen.items()} == {key: counts[key] for key in seen}
    assert set(counts) - set(seen) <= set(short)


def test_sentinel_layout_and_absent_keys():
    k = 4
    counts = kr.count(["ACGTAC"], k)
    reads = ["ACGTAC", "", "ACG", "TTTTT", "ACGT"]
    abundance, offsets, summary, _ = lr.lookup(reads, counts, k, False, cutoff=1)
    assert offsets.tolist() == [0, 6, 6, 9, 14, 18]
    assert abundance.tolist() == [1, 1, 1, NONE, NONE, NONE] + [NONE] * 3 + [0, 0, NONE, NONE, NONE] + [1, NONE, NONE, NONE]
    assert summary.tolist() == [[1, 0, NONE, NONE], [NONE, 0, NONE, NONE], [NONE, 0, NONE, NONE], [0, 2, 0, 1],
                                [1, 0, NONE, NONE]]
    # a count beyond 32 bits is clipped in the abundance, not in the weight's index
    big = {kr._key(kr._digits("ACGT"), k, False): 1 << 33}
    abundance, _, summary, score = lr.lookup(["ACGT"], big, k, False, cutoff=5, weights=[1.0, 2.0, 4.0])
    assert abundance[0] == NONE - 1 and summary[0].tolist() == [NONE - 1, 0, NONE, NONE] and score[0] == 4.0


@pytest.mark.parametrize("found,cutoff,want", [
    ([], 3, (NONE, 0, NONE, NONE)),                    # no window
    ([2], 3, (2, 1, 0, 0)),                            # one window, weak
    ([5], 3, (5, 0, NONE, NONE)),                      # one window, not weak
    ([1, 2, 0, 1], 3, (0, 4, 0, 3)),                   # all weak
    ([7, 3, 9], 3, (3, 0, NONE, NONE)),                # none weak: the cutoff itself is not below it
    ([1, 2, 9, 9, 9], 3, (1, 2, 0, 1)),                # a weak run at the front
    ([9, 9, 9, 2, 1], 3, (1, 2, 3, 4)),                # ... at the back
    ([0, 0, 0], 0, (0, 0, NONE, NONE)),                # cutoff 0: no window is weak
])
def test_summary_fields(found, cutoff, want):
    assert lr.summary_of(found, cutoff) == want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 1000])
def test_butterfly_sum_against_fsum(n):
    rng = random.Random(n)
    w = [rng.uniform(-1, 1) * 10.0 ** rng.randrange(-8, 8) for _ in range(n)]
    got = lr.butterfly_sum(w)
    assert abs(got - math.fsum(w)) <= n * 2.0 ** -52 * sum(abs(v) for v in w)
    if n == 0:
        assert got == 0.0 and math.copysign(1.0, got) == 1.0
    if n:  # the order matters: the same numbers backwards need not give the same bits, the same order always does
        assert lr.butterfly_sum(w) == got


def _posterior(keys, error_share):
    from covest_amd.posterior import PosteriorClasses
    n = len(keys)
    return PosteriorClasses(keys, np.ones(n), np.zeros(n), error_share, np.ones((n, 1)), np.ones(n))


def test_abundance_weights():
    from covest_amd.read_errors import abundance_weights
    # keys with gaps, the smallest above 1, not in order; columns: 0, 1, 2 wrong bases
    keys = [7, 3, 4, 10]
    share = np.array([[0.9, 0.07, 0.03], [0.1, 0.6, 0.3], [0.5, 0.3, 0.2], [1.0, 0.0, 0.0]])
    post = _posterior(keys, share)
    err = abundance_weights(post)
    assert err.dtype == np.float64 and err.shape == (11,)
    e3, e4, e7, e10 = 0.6 + 0.3, 0.3 + 0.2, 0.07 + 0.03, 0.0
    assert err.tolist() == [e3, e3, e3, e3, e4, e4, e4, e7, e7, e7, e10]
    log_free = abundance_weights(post, "log_error_free")
    want = [math.log(v) for v in (0.1, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.9, 0.9, 0.9, 1.0)]
    assert np.allclose(log_free, want, rtol=1e-15, atol=0) and log_free[10] == 0.0
    assert abundance_weights(_posterior([2], np.array([[0.0, 1.0]])), "log_error_free").tolist() == [-math.inf] * 3
    with pytest.raises(ValueError):
        abundance_weights(post, "error_free")
    with pytest.raises(ValueError):
        abundance_weights(_posterior([], np.zeros((0, 2))))


def test_locate_single_errors():
    from covest_amd.read_errors import ReadErrorScores
    k, L = 5, 20                                   # 16 windows, the last is 15
    rows = [                                       # (weak, first, last) -> position
        ((0, -1, -1), -1),                         # no weak window
        ((5, 7, 11), 11),                          # an inner error at base 11: windows 7 .. 11
        ((3, 0, 2), 2),                            # at base 2: windows 0 .. 2
        ((1, 0, 0), 0),                            # the first base
        ((1, 15, 15), 19),                         # the last base: only the last window
        ((4, 12, 15), 16),                         # base 16: windows 12 .. 15
        ((6, 3, 8), -1),                           # a run longer than k: more than one error
        ((3, 2, 9), -1),                           # not contiguous
    ]
    cols = list(zip(*[r[0] for r in rows]))
    scores = ReadErrorScores(k, [L] * len(rows), [0] * len(rows), cols[0], cols[1], cols[2], np.zeros(len(rows)), 3, 0.5, 0.01)
    want = [r[1] for r in rows]
    assert scores.locate_single_errors().tolist() == want
    assert lr.locate_single_errors(k, [L] * len(rows), *cols).tolist() == want
    assert scores.flagged.tolist() == [w > 0 for w in cols[0]]
    assert scores.flagged_share == 7 / 8 and scores.predicted_share == pytest.approx(1 - 0.99 ** 20, rel=1e-14)
    # a read of exactly k bases, weak: its one window is first and last -- undecided
    short = ReadErrorScores(k, [k], [0], [1], [0], [0], np.zeros(1), 3, 0.5, 0.01)
    assert short.locate_single_errors().tolist() == [-1]


def test_simulated_case_under_the_reference():
    """2 812 reads of 64 bases of a 6 000-base genome at e = 0.01, k = 17 canonical, cutoff 3."""
    from covest_amd.read_errors import ReadErrorScores
    c, want = lr.CASE, lr.CASE_EXPECTED
    _, bases, hit, reads, _ = lr.simulated_case()
    assert bases.shape == (c["n_reads"], c["read_len"])
    summary = lr.simulated_case_summary()
    n_wrong, n_flagged, missed, false, sens, spec = lr.detection_figures(summary[:, 1] > 0, hit)
    assert (n_wrong, n_flagged, missed, false) == (want["with_error"], want["flagged"], want["missed"], want["false"])
    assert (n_wrong, n_flagged, missed, false) == (1396, 1398, 1, 3)
    assert round(sens, 4) == 0.9993 and round(spec, 4) == 0.9979
    cols = [lr.signed(summary[:, j]) for j in range(4)]
    scores = ReadErrorScores(c["k"], [c["read_len"]] * c["n_reads"], *cols, np.zeros(c["n_reads"]), c["cutoff"], None, None)
    located = scores.locate_single_errors()
    assert np.array_equal(located, lr.locate_single_errors(c["k"], scores.lengths, *cols[1:]))
    assert lr.location_figures(located, hit) == (1018, 1015, 2, 1)
    assert lr.location_figures(located, hit) == (want["single"], want["located_right"], want["located_wrong"],
                                                 want["located_undecided"])
    for cutoff in range(3, 8):  # the bound the device test asserts holds under the reference at every cutoff 3 .. 7
        _, _, _, _, sens, spec = lr.detection_figures(lr.simulated_case_summary(cutoff)[:, 1] > 0, hit)
        assert sens >= 0.999 and spec >= 0.995, cutoff


class _NeverAsked:
    """A KmerCounts without a handle: any call into the library would fail on it."""
    k, _handle = 5, None


def _lookup(*args, **kwargs):
    from covest_amd.kmer_hist import KmerCounts
    return KmerCounts.lookup(_NeverAsked(), *args, **kwargs)


def test_argument_errors_before_the_library_is_asked(monkeypatch):
    from covest_amd import _capi

    def refuse():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "lib", refuse)
    with pytest.raises(KeyError):
        _lookup(["ACGTN"])
    with pytest.raises(KeyError):
        _lookup((np.frombuffer(b"ACGTXACGT", dtype=np.uint8), np.array([0, 9])))
    with pytest.raises(ValueError):
        _lookup(["ACGT"], cutoff=-1)
    with pytest.raises(ValueError):
        _lookup(["ACGT"], cutoff=1 << 32)
    with pytest.raises(ValueError):
        _lookup(["ACGT"], weights=[])
    with pytest.raises(ValueError):
        _lookup(["ACGT"], weights=[[1.0, 2.0]])
    with pytest.raises(ValueError):
        _lookup((np.zeros(4, dtype=np.int32), np.array([0, 4])))
    with pytest.raises(ValueError):
        _lookup((np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 5])))
    with pytest.raises(ValueError):
        _lookup((np.frombuffer(b"ACGT", dtype=np.uint8), np.array([3, 1])))
    # a base outside acgt beyond the offsets' reach is not looked at; no reads: nothing to ask the library for
    got = _lookup((np.frombuffer(b"NN", dtype=np.uint8), np.array([1])))
    assert got.n_reads == 0 and got.abundance.size == 0 and got.weak.size == 0 and got.score is None
    assert _lookup([]).n_reads == 0
