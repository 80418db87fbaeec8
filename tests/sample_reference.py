"""The read sampler's selection rule and compaction restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the rule in include/covest_amd.h / DESIGN.md section 6m, not from the kernels:
  read r = index within the call + first_read (64-bit);
  w = word 0 of Philox4x32-10 (sim_reference.philox) on the counter (lo32(r), hi32(r), 0, 2), key = (seed & 0xffffffff,
  seed >> 32);
  kept iff w < thr, thr = floor((1.0 / factor) * 2^32) formed in double;
  the output is the kept reads in input order, in the packed layout (bases back to back, offsets[n_kept + 1]).
"""
import math

import numpy as np

import sim_reference as sr


def threshold(factor):
    return int(math.floor((1.0 / float(factor)) * 4294967296.0))


def counter(r):
    """The Philox counter of read r."""
    return (r & sr.MASK, r >> 32, 0, 2)


def words(first_read, n, seed):
    """Word 0 of reads first_read .. first_read + n (uint64 array holding 32-bit words)."""
    r = [int(first_read) + i for i in range(int(n))]
    lo, hi = sr.split64(r)
    return sr.philox(lo, hi, 0, 2, int(seed) & sr.MASK, int(seed) >> 32)[0]


def keep_mask(first_read, n, factor, seed):
    return words(first_read, n, seed) < np.uint64(threshold(factor))


def sample(bases, offsets_or_read_len, first_read, factor, seed):
    """(out_bases, out_offsets, kept): `bases` the reads back to back (any shape, flattened), `offsets_or_read_len` the
    int64 offsets[n + 1] or the one read length (then the number of reads is bases.size // read_len; for read_len 0 pass
    offsets)."""
    blob = np.ascontiguousarray(bases).reshape(-1)
    if np.ndim(offsets_or_read_len) == 0:
        L = int(offsets_or_read_len)
        rows = np.flatnonzero(keep_mask(first_read, blob.size // L, factor, seed))
        return (blob.reshape(-1, L)[rows].reshape(-1), np.arange(rows.size + 1, dtype=np.int64) * L,
                rows.astype(np.int64) + int(first_read))
    else:
        offsets = np.asarray(offsets_or_read_len, dtype=np.int64)
    n = offsets.size - 1
    rows = np.flatnonzero(keep_mask(first_read, n, factor, seed))
    lens = offsets[rows + 1] - offsets[rows]
    out_offsets = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lens, out=out_offsets[1:])
    pieces = [blob[offsets[i]:offsets[i + 1]] for i in rows]
    out = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    return out.astype(np.uint8), out_offsets, rows.astype(np.int64) + int(first_read)
