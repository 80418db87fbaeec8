"""The read split's group rule and stable partition restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the rule in include/covest_amd.h / DESIGN.md section 6aa, not from the kernels:
  read r = index within the call + first_read (64-bit);
  w = word 0 of Philox4x32-10 (sim_reference.philox) on the counter (lo32(r), hi32(r), 0, 8), key = (seed & 0xffffffff,
  seed >> 32);
  group(r) = (w * G) >> 32 in 64-bit integer arithmetic, 1 <= G <= 256;
  the output is the reads in the order of their groups, input order within a group (a stable partition), in the packed
  layout (bases back to back, offsets[n + 1]); read_index[rank] = r; group_first[g] = the rank at which group g starts,
  group_first[G] = n.
"""
import numpy as np

import sim_reference as sr

STREAM = 8


def groups_of(first_read, n, groups, seed):
    """The group of reads first_read .. first_read + n: int64 array."""
    r = [int(first_read) + i for i in range(int(n))]
    lo, hi = sr.split64(r)
    w = sr.philox(lo, hi, 0, STREAM, int(seed) & sr.MASK, int(seed) >> 32)[0]
    return ((w * np.uint64(groups)) >> np.uint64(32)).astype(np.int64).reshape(-1)  # (w < 2^32, G <= 2^8: fits 64 bits)


def _starts(group, groups):
    """group_first: the exclusive running count of the groups' sizes, and the number of reads behind it."""
    group_first = np.zeros(groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(group, minlength=groups), out=group_first[1:])
    return group_first


def split(bases, offsets_or_read_len, first_read, groups, seed):
    """(out_bases, out_offsets, read_index, group_first): `bases` the reads back to back (any shape, flattened),
    `offsets_or_read_len` the int64 offsets[n + 1] or the one read length (then the number of reads is bases.size //
    read_len; for read_len 0 pass offsets).  The packed output is built as sample_reference.sample builds its own."""
    blob = np.ascontiguousarray(bases).reshape(-1)
    if np.ndim(offsets_or_read_len) == 0:
        L = int(offsets_or_read_len)
        n = blob.size // L
        group = groups_of(first_read, n, groups, seed)
        rows = np.argsort(group, kind="stable")
        return (blob.reshape(-1, L)[rows].reshape(-1), np.arange(n + 1, dtype=np.int64) * L,
                rows.astype(np.int64) + int(first_read), _starts(group, groups))
    offsets = np.asarray(offsets_or_read_len, dtype=np.int64)
    n = offsets.size - 1
    group = groups_of(first_read, n, groups, seed)
    rows = np.argsort(group, kind="stable")
    lens = offsets[rows + 1] - offsets[rows]
    out_offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=out_offsets[1:])
    pieces = [blob[offsets[i]:offsets[i + 1]] for i in rows]
    out = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    return out.astype(np.uint8), out_offsets, rows.astype(np.int64) + int(first_read), _starts(group, groups)
