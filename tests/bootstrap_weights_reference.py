"""The read bootstrap's multiplicities restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the definition in include/covest_amd.h / DESIGN.md section 6ak, not from the kernel:
  read r (64-bit: index within the call + first_read) of replicate b (uint32) under `seed` takes
  w = word 0 of Philox4x32-10 (tests/sim_reference.philox) on the counter (lo32(r), hi32(r), b, 9), key = (lo32(seed),
  hi32(seed)); its multiplicity is m = #{ i in 0 .. 12 : w >= T_i }, T_i = floor(2^32 P(Poisson(1) <= i)).
The thirteen thresholds are written out here as the header writes them; tests/test_read_bootstrap_cpu.py derives them
again, exactly, from the series of 1 / e.

expand(reads, weights) is the weighted counter's truth: read r repeated weights[r] times, to be counted by the unweighted
restatement (tests/kmer_reference.py).
"""
import numpy as np

import sim_reference as sr

STREAM = 9
THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
              4294966817, 4294967252, 4294967292, 4294967295)


def multiplicity(words):
    """m = #{i : w >= T_i} per 32-bit word (any integer array): uint32."""
    w = np.asarray(words, dtype=np.uint64)
    m = np.zeros(w.shape, dtype=np.uint32)
    for t in THRESHOLDS:
        m += (w >= np.uint64(t)).astype(np.uint32)
    return m


def words(n_reads, replicate, seed=0, first_read=0):
    """Word 0 of the block of reads first_read .. first_read + n_reads - 1 in `replicate`: a uint64 array of 32-bit words."""
    r = [int(first_read) + i for i in range(int(n_reads))]  # (Python integers: the index may pass 2^32, and 2^63)
    lo, hi = sr.split64(r)
    w0, _, _, _ = sr.philox(lo, hi, int(replicate), STREAM, *sr._key(seed))
    return w0


def weights(n_reads, replicate, seed=0, first_read=0):
    """(n_reads,) uint32: what covest_bootstrap_weights writes."""
    if int(n_reads) == 0:
        return np.zeros(0, dtype=np.uint32)
    return multiplicity(words(n_reads, replicate, seed, first_read))


def expand(reads, weights):
    """The list of reads with read r repeated weights[r] times, in order."""
    reads = list(reads)
    if len(reads) != len(weights):
        raise ValueError("one weight a read")
    return [read for read, w in zip(reads, weights) for _ in range(int(w))]
