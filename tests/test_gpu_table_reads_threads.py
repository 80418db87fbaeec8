"""Two threads on ONE counter: the host forms that walk reads against the k-mer table (KmerCounts.lookup, correct,
read_influence) stage their reads in the counter's own buffers, the correction even reads its result out of them, so a
host form holds the counter's lock from its staging to its copies back (host.h KmerHostCall).

Two read sets of equal shape and different content; each set's results are computed single-threaded first -- that pass
also sizes the staging buffers, so nothing reallocates afterwards and a form that ran on the other thread's reads shows
as wrong numbers.  Then a thread a set makes eight rounds of the three calls (ctypes releases the GIL for a call), and
every result must be its single-threaded one.  A pass is necessary, not sufficient: a missing lock shows only when two
calls happen to interleave within the eight rounds.
"""
import random
import threading

import numpy as np
import pytest

import kmer_reference as kr

pytestmark = pytest.mark.gpu

K, N_READS, READ_LEN, ROUNDS, CUTOFF = 21, 64, 100, 8, 1


def read_set(seed):
    """64 reads of 100 bases of the genome, every other one with a substitution: weak windows, runs, corrections."""
    rng = random.Random(seed)
    reads = kr.genome_reads(rng, N_READS, READ_LEN)
    for i in range(0, N_READS, 2):
        at = rng.randrange(READ_LEN)
        other = "ACGT"[("ACGT".index(reads[i][at]) + 1 + rng.randrange(3)) % 4]
        reads[i] = reads[i][:at] + other + reads[i][at + 1:]
    return reads


def results(counts, reads, weights, table):
    looked, fixed = counts.lookup(reads, cutoff=CUTOFF, weights=weights), counts.correct(reads, CUTOFF)
    return looked.abundance, looked.summary, looked.score, fixed.bases, fixed.fix, counts.read_influence(reads, table)


def same(got, want):
    exact = all(np.array_equal(g, w) for g, w in zip(got[:2] + got[3:5], want[:2] + want[3:5]))
    bits = all(g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g.view(np.uint64), w.view(np.uint64))
               for g, w in ((got[2], want[2]), (got[5], want[5])))
    return exact and bits


def test_two_threads_share_a_counter(hip_lib):
    from covest_amd.kmer_hist import KmerCounts
    rng = np.random.default_rng(5)
    weights, table = rng.normal(size=4), rng.normal(size=(4, 3))
    sets = [read_set(101), read_set(202)]
    assert sets[0] != sets[1] and all(len(r) == READ_LEN for s in sets for r in s)
    counts = KmerCounts(K, canonical=True)
    try:
        counts.add_reads([kr.genome()])
        want = [results(counts, reads, weights, table) for reads in sets]
        assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[0][3], want[1][3])
        assert want[0][4][:, 1].sum() > 0 and want[1][4][:, 1].sum() > 0  # (both sets have corrected runs)
        wrong, start = [], threading.Barrier(2)

        def work(which):
            try:
                start.wait()
                for rnd in range(ROUNDS):
                    if not same(results(counts, sets[which], weights, table), want[which]):
                        wrong.append((which, rnd))
            except Exception as e:  # (a failed call must fail the test, not end a thread quietly)
                wrong.append((which, repr(e)))

        threads = [threading.Thread(target=work, args=(which,)) for which in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not wrong, wrong
    finally:
        counts.close()
