"""The delete-one-read influence rows and the moments of rows restated in plain Python over tests/kmer_reference.py and
tests/lookup_reference.py (TEST INFRASTRUCTURE ONLY; not collected).  Written from the definitions in
include/covest_amd.h and csrc/kmer_influence.h, not from the kernels:

  * a window's key is kmer_reference._key of its digits, its abundance a the count kmer_reference.count holds (0: none);
  * m = the windows of the read with that key; only the FIRST window of a key contributes, and its term per column is
    the single subtraction table[min(max(a - m, 0), n_rows - 1)][c] - table[min(a, n_rows - 1)][c];
  * the sum per column is the lookup's: lane l of 64 adds the terms of its first-occurrence windows l, l + 64, ... in
    ascending order onto +0.0, the 64 partials are folded by the xor butterfly 32, ..., 1; lane 0's value;
  * the last column is the number of windows; a read shorter than k is all +0.0; a read of more than MAX_WINDOWS windows
    has NaN in its value columns;
  * moments: exact sums (math.fsum) -- the device's reduction is held to the bound of an n-term sum, not to the bit.
"""
import math

import numpy as np

import kmer_reference as kr
import lookup_reference as lr

MAX_WINDOWS = 4096
LANES = lr.LANES


def read_keys(read, k, canonical):
    """The key of every window of one read: [] for a read shorter than k."""
    d = kr._digits(read)
    return [kr._key(d[s:s + k], k, canonical) for s in range(len(d) - k + 1)]


def first_terms(read, counts, k, canonical, table):
    """[(window, m, a, term (n_cols,) float64)] of the first-occurrence windows of one read, ascending."""
    table = np.asarray(table, dtype=np.float64)
    top = table.shape[0] - 1
    keys = read_keys(read, k, canonical)
    multiplicity = {}
    for key in keys:
        multiplicity[key] = multiplicity.get(key, 0) + 1
    seen, out = set(), []
    for s, key in enumerate(keys):
        if key in seen:
            continue
        seen.add(key)
        a, m = counts.get(key, 0), multiplicity[key]
        out.append((s, m, a, table[min(max(a - m, 0), top)] - table[min(a, top)]))
    return out


def influence_row(read, counts, k, canonical, table):
    """One row (n_cols + 1,) in the kernel's order of addition."""
    n_cols = np.asarray(table).shape[1]
    n_windows = max(len(read) - k + 1, 0)
    row = np.zeros(n_cols + 1, dtype=np.float64)
    row[n_cols] = float(n_windows)
    if n_windows > MAX_WINDOWS:
        row[:n_cols] = np.nan
        return row
    terms = first_terms(read, counts, k, canonical, table)
    for col in range(n_cols):
        p = [0.0] * LANES
        for s, _, _, term in terms:
            p[s % LANES] = p[s % LANES] + float(term[col])
        off = LANES // 2
        while off >= 1:
            p = [p[lane] + p[lane ^ off] for lane in range(LANES)]
            off //= 2
        row[col] = p[0]
    return row


def influence_rows(reads, counts, k, canonical, table):
    """(n, n_cols + 1) float64 of `reads` (strings) against `counts` (kmer_reference.count of whatever was counted)."""
    n_cols = np.asarray(table).shape[1]
    return np.array([influence_row(r, counts, k, canonical, table) for r in reads], dtype=np.float64).reshape(len(reads), n_cols + 1)


def row_bound(read, counts, k, canonical, table):
    """Per column, W * 2^-52 * sum |terms|: the bound of a W-term floating-point sum in any order."""
    terms = first_terms(read, counts, k, canonical, table)
    n_windows = max(len(read) - k + 1, 0)
    n_cols = np.asarray(table).shape[1]
    return np.array([n_windows * 2.0 ** -52 * math.fsum(abs(float(t[3][c])) for t in terms) for c in range(n_cols)])


def pair_index(q, a, b):
    return a * q - a * (a - 1) // 2 + (b - a)


def moments(rows, centre):
    """(sum, cross, bound_sum, bound_cross) of an (n, q) array about `centre`, by math.fsum over the deviations as IEEE
    doubles form them (the subtraction and the product are rounded once, as on the device); the bounds are those of an
    n-term floating-point sum in any order, n * 2^-52 * sum |terms|."""
    rows = np.asarray(rows, dtype=np.float64)
    n, q = rows.shape
    d = rows - np.asarray(centre, dtype=np.float64)[None, :]
    total = np.array([math.fsum(d[:, a].tolist()) for a in range(q)])
    bound_sum = np.array([n * 2.0 ** -52 * math.fsum(np.abs(d[:, a]).tolist()) for a in range(q)])
    cross = np.zeros(q * (q + 1) // 2)
    bound_cross = np.zeros_like(cross)
    for a in range(q):
        for b in range(a, q):
            prod = d[:, a] * d[:, b]
            cross[pair_index(q, a, b)] = math.fsum(prod.tolist())
            bound_cross[pair_index(q, a, b)] = n * 2.0 ** -52 * math.fsum(np.abs(prod).tolist())
    return total, cross, bound_sum, bound_cross
