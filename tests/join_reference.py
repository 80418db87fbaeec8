"""The join of two k-mer tables restated from its definition, and the reads the join's tests
count.  TEST INFRASTRUCTURE ONLY.

    out[i][j] = #{ x in U : min(a(x), rows - 1) == i and min(b(x), cols - 1) == j }

a(x), b(x): what two tests/kmer_reference.py `count` dicts hold for key x, 0 for a key they do not hold; U: the keys held
(with a count above 0) by at least one of them.  It knows nothing of slots, sweeps or bins: a set union and two
look-ups a key.  tests/test_join_cpu.py holds it against a loop over every possible key of hand-made dicts;
tests/test_gpu_join.py holds the device against it.

The reads: a 2 000-base genome, a few hundred reads of 60 .. 100 bases with 2 % substitutions, so that keys share
minimizers and first slots are taken.  Every builder is a pure function of its arguments (seeded generators).
"""
import functools
import random

import numpy as np

import kmer_reference as kr

GENOME_LEN = 2000


def join(counts_a, counts_b, rows, cols):
    """numpy.int64 (rows, cols), rows >= 1 and cols >= 1."""
    if rows < 1 or cols < 1:
        raise ValueError("a matrix has at least one row and one column")
    out = np.zeros((rows, cols), dtype=np.int64)
    held_a = {x for x, n in counts_a.items() if n > 0}
    held_b = {x for x, n in counts_b.items() if n > 0}
    for x in held_a | held_b:
        a = counts_a[x] if x in held_a else 0
        b = counts_b[x] if x in held_b else 0
        out[min(a, rows - 1)][min(b, cols - 1)] += 1
    return out


def unclipped_shape(counts_a, counts_b):
    """(largest count of a + 1, largest count of b + 1): the shape at which no clip bites."""
    return max(counts_a.values(), default=0) + 1, max(counts_b.values(), default=0) + 1


@functools.lru_cache(maxsize=None)
def genome(which=0):
    """Genome 0 is the head of kmer_reference's; the others are drawn on their own (disjoint from it at k >= 12 but for
    chance)."""
    if which == 0:
        return kr.genome()[:GENOME_LEN]
    return kr._random_bases(random.Random(31000 + which), GENOME_LEN)


@functools.lru_cache(maxsize=None)
def noisy_reads(seed, n=300, which=0, rate=0.02, shortest=60, longest=100):
    """n reads of shortest .. longest bases from genome `which`, each base replaced by another with probability
    `rate`; every fourth read reverse-complemented, every other one lower-cased."""
    rng = random.Random(33000 + seed)
    g = genome(which)
    reads = []
    for i in range(n):
        length = rng.randrange(shortest, longest + 1)
        at = rng.randrange(len(g) - length + 1)
        read = list(g[at:at + length])
        for p in range(length):
            if rng.random() < rate:
                read[p] = "ACGT"[("ACGT".index(read[p]) + 1 + rng.randrange(3)) % 4]
        read = "".join(read)
        if i % 4 == 3:
            read = kr.revcomp(read)
        reads.append(read.lower() if i % 2 else read)
    return tuple(reads)
