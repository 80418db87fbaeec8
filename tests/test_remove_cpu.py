"""The restatement of removal (tests/remove_reference.py) against a loop over every possible key at k = 2 and 3, and the
Python layer's argument rules, which hold before the library is asked.  No GPU."""
import itertools
import random

import numpy as np
import pytest

import kmer_reference as kr
import remove_reference as rr


def occurrences(kmer, reads, canonical):
    """How often the k-mer `kmer` (a string) starts somewhere in `reads`, on either strand where canonical: by
    comparing strings, one position at a time."""
    k, n = len(kmer), 0
    for read in reads:
        read = read.upper()
        for s in range(len(read) - k + 1):
            window = read[s:s + k]
            n += window == kmer or (canonical and kmer != kr.revcomp(kmer) and window == kr.revcomp(kmer))
    return n


def every_key(k, canonical):
    """(key, k-mer) for every k-mer that is its own key: all 4^k strings, the smaller strand alone where canonical."""
    for letters in itertools.product("ACGT", repeat=k):
        kmer = "".join(letters)
        key = int(kmer.translate(str.maketrans("ACGT", "0123")), 4)
        if not canonical or key <= int(kr.revcomp(kmer).translate(str.maketrans("ACGT", "0123")), 4):
            yield key, kmer


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [2, 3])
def test_against_every_possible_key(k, canonical):
    rng = random.Random(100 * k + canonical)
    reads = ["".join(rng.choice("ACGTacgt") for _ in range(rng.randrange(k, 12))) for _ in range(9)]
    gone, stay = reads[:4], reads[4:]
    t = rr.Table(k, canonical).add(reads)
    before = dict(t.counts)
    t.remove(gone)
    seen = set()
    for key, kmer in every_key(k, canonical):
        all_n, stay_n = occurrences(kmer, reads, canonical), occurrences(kmer, stay, canonical)
        assert before.get(key, 0) == all_n and t.counts.get(key, 0) == stay_n, (kmer, all_n, stay_n)
        assert (key in t.counts) == (all_n > 0), kmer          # a key stays where it was, also at count 0
        assert (key in t.held()) == (stay_n > 0), kmer         # held means count > 0
        seen.add(key)
    assert set(t.counts) <= seen
    held = {key for key, kmer in every_key(k, canonical) if occurrences(kmer, stay, canonical) > 0}
    assert t.occupancy() == (len(held), len(before))
    hist, distinct = t.histogram()
    assert distinct == len(held) and hist[0] == 0 and sum(hist) == len(held)
    assert hist == kr.histogram(stay, k, canonical)[0]
    assert t.lookup(stay[:2]) == [[occurrences(r[s:s + k].upper(), stay, canonical) for s in range(len(r) - k + 1)]
                                  for r in stay[:2]]
    # putting them back gives the table as it was; compaction drops what nothing holds
    assert t.add(gone).counts == before
    t.remove(reads)
    assert t.occupancy() == (0, len(before)) and t.histogram() == ([0], 0)
    assert t.compact().occupancy() == (0, 0)


def test_underflow_raises_and_weights_subtract():
    t = rr.Table(3).add(["ACGTAC", "ACG"], weights=[13, 2])
    assert t.counts[int("012", 4)] == 15
    with pytest.raises(rr.Underflow):
        t.remove(["TTT"])                       # a key the table does not carry
    with pytest.raises(rr.Underflow):
        t.remove(["ACG"], weights=[16])         # more than the key has
    assert t.counts[int("012", 4)] == 15        # (a refused removal changes nothing here)
    t.remove(["TTT", "ACG"], weights=[0, 15])   # weight 0 on a read that was never added: no underflow
    assert t.counts[int("012", 4)] == 0 and int("012", 4) not in t.held() and t.occupancy() == (3, 4)
    short = rr.Table(5, True).add(["AC", ""])
    assert short.occupancy() == (2, 2)
    assert short.remove(["", "AC"]).occupancy() == (0, 2)
    with pytest.raises(rr.Underflow):
        short.remove([""])


# ---- the Python layer, before the library is asked
@pytest.fixture
def no_library(monkeypatch):
    from covest_amd import _capi

    def refuse():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_capi, "lib", refuse)


class _Model:
    k, device, params = 40, -1, ("coverage", "error_rate")


def test_routes_are_checked_first(no_library):
    from covest_amd import jackknife
    reads = np.full((10, 60), ord("A"), dtype=np.uint8)
    assert jackknife.ROUTES == ("recount", "remove")
    for route in ("Remove", "", None, "subtract"):
        with pytest.raises(ValueError, match="route"):
            jackknife.leave_group_out_histograms(reads, 21, 4, route=route)
        with pytest.raises(ValueError, match="route"):
            jackknife.read_jackknife(_Model(), [10.0, 0.01], reads, groups=4, route=route)
    with pytest.raises(ValueError, match="31"):
        jackknife.leave_group_out_histograms(reads, 32, 4, route="remove")
    with pytest.raises(ValueError, match="31"):
        jackknife.read_jackknife(_Model(), [10.0, 0.01], reads, groups=4, route="remove")


def _counter_without_a_device(k=21):
    from covest_amd.kmer_hist import KmerCounts
    c = KmerCounts.__new__(KmerCounts)
    c.k, c.canonical, c._handle = k, False, None
    return c


def test_weights_and_shapes_are_checked_first(no_library):
    c = _counter_without_a_device()
    reads = ["ACGT" * 10, "TTGA" * 9, "C" * 50]
    for bad in ([1, 2], [1, 2, 3, 4], [[1, 2, 3]], [1.0, 2.0, 3.0], [1, -1, 0], [0, 1, 1 << 32]):
        with pytest.raises(ValueError, match="weights"):
            c.remove_weighted(reads, bad)
    with pytest.raises(KeyError):
        c.remove(["ACGN"])
    with pytest.raises(ValueError, match="equal shape"):
        c.replace_reads(reads, reads[:2], [1, 0, 1])
    with pytest.raises(ValueError, match="equal shape"):
        c.replace_reads(reads, ["ACGT" * 10, "TTGA" * 9, "C" * 51], [1, 0, 1])
    with pytest.raises(ValueError, match="equal shape"):   # as many bases, cut elsewhere
        c.replace_reads(["ACGT", "AC"], ["ACG", "TAC"], [1, 1])
    for bad in ([1, 0], [1, 0, 2], [0.0, 1.0, 1.0], [1, 0, -1]):
        with pytest.raises(ValueError):
            c.replace_reads(reads, reads, bad)


def test_print_output_records_the_route():
    from covest_amd.jackknife import summarize_jackknife
    from covest_amd.report import print_output
    from test_split_cpu import NAMES, _Stub
    est = [[9.0, 0.04], [9.1, 0.05], [8.9, 0.06]]
    jack = summarize_jackknife(est, [True] * 3, [10.0, 0.05], [1800.0] * 3, 2000.0, NAMES, [None, 0.05], 0.95, _Stub().correct_c)
    jack.update(groups=3, level=0.95)
    args = dict(estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True)
    without = print_output({1: 1000, 2: 400, 10: 20}, _Stub(), True, 1, jackknife=dict(jack), **args)
    assert "jackknife_route" not in without
    for route in ("recount", "remove"):
        rec = print_output({1: 1000, 2: 400, 10: 20}, _Stub(), True, 1, jackknife=dict(jack, route=route), **args)
        assert rec["jackknife_route"] == route and {k: v for k, v in rec.items() if k != "jackknife_route"} == without
