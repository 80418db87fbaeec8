"""Repeat-bearing genomes restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the definition in include/covest_amd.h / DESIGN.md section 6n, not from the kernel, on the stream of
tests/sim_reference.py (Philox4x32-10, key = (seed & 0xffffffff, seed >> 32)):
  family base g = f * unit_len + offset: counter (lo32(g>>2), hi32(g>>2), 0, 3), word g & 3, "ACGT"[word >> 30].
  copy number of family f: u = word 0 of counter (lo32(f), hi32(f), 0, 4); o_f = 1 + #{o in 1 .. max_copies - 1:
          t_o <= u}, t_o = min(2^32, floor(cdf_o * 2^32)); cdf_1 = q1, cdf_2 = cdf_1 + (1 - q1) * q2,
          b = ((1 - q1) * (1 - q2)) * q, cdf_3 = cdf_2 + b, then b = b * (1 - q), cdf_{o+1} = cdf_o + b (doubles).
  unit list: families 0, 1, 2, ... each o_f times until n_units entries; entry j: counter (lo32(j), hi32(j), 0, 5) ->
          w0..w3; stably sorted by w0 | w1 << 32, ties by j; forward iff w2 & 1 or both_orientations is off;
          plan[slot] = f << 1 | forward.
  genome base i: u = i // unit_len, off = i % unit_len, (f, fwd) = plan[u]; forward: family base f * unit_len + off;
          reverse: 3 - code of family base f * unit_len + unit_len - 1 - off; then w = word i & 3 of counter
          (lo32(i>>2), hi32(i>>2), 0, 6): substituted iff w < floor(divergence * 2^32) by code (code + 1 + w % 3) & 3.
"""
import numpy as np

import sim_reference as sr


def thresholds(q1, q2, q, max_copies):
    """[t_1 .. t_{max_copies - 1}] as Python integers."""
    q1, q2, q = float(q1), float(q2), float(q)
    out, cdf, b = [], q1, 0.0
    for o in range(1, int(max_copies)):
        if o == 2:
            cdf = cdf + (1.0 - q1) * q2
        elif o == 3:
            b = ((1.0 - q1) * (1.0 - q2)) * q
            cdf = cdf + b
        elif o > 3:
            b = b * (1.0 - q)
            cdf = cdf + b
        out.append(min(1 << 32, int(np.floor(cdf * 4294967296.0))))
    return out


def copy_numbers(first, count, q1, q2, q, max_copies, seed):
    """o_f of families first .. first + count (an int64 array)."""
    lo, hi = sr.split64(np.arange(first, first + count, dtype=np.uint64))
    u = sr.philox(lo, hi, 0, 4, *sr._key(seed))[0]
    t = np.array(thresholds(q1, q2, q, max_copies), dtype=np.uint64)
    return 1 + np.searchsorted(t, u, side="right").astype(np.int64)  # t ascends: the number of t_o <= u


def plan(n_units, q1, q2, q, seed, max_copies=64, both_orientations=True):
    """(plan (n_units,) int64, n_families)."""
    n_units = int(n_units)
    if n_units == 0:
        return np.zeros(0, dtype=np.int64), 0
    fams, have, first = [], 0, 0
    while have < n_units:  # every family has at least one copy: n_units families always suffice
        o = copy_numbers(first, n_units - have, q1, q2, q, max_copies, seed)
        cut = int(np.searchsorted(np.cumsum(o), n_units - have, side="left")) + 1  # families needed of this batch
        o = o[:cut]
        fams.append(np.repeat(np.arange(first, first + o.size, dtype=np.int64), o))
        have += int(o.sum())
        first += o.size
    family = np.concatenate(fams)[:n_units]
    n_families = int(family[-1]) + 1
    lo, hi = sr.split64(np.arange(n_units, dtype=np.uint64))
    w0, w1, w2, _ = sr.philox(lo, hi, 0, 5, *sr._key(seed))
    order = np.argsort(w0 | (w1 << np.uint64(32)), kind="stable")
    forward = (w2 & np.uint64(1)).astype(np.int64) if both_orientations else np.ones(n_units, dtype=np.int64)
    return (family[order] << 1) | forward[order], n_families


def family_codes(g, seed):
    """Codes 0..3 of the family bases at the 64-bit places g (Python integers or an object/uint64 array)."""
    g = np.asarray(g, dtype=np.uint64)
    lo, hi = sr.split64(g >> np.uint64(2))
    out = sr.philox(lo, hi, 0, 3, *sr._key(seed))
    return (sr._words(out, g & np.uint64(3)) >> np.uint64(30)).astype(np.int64)


def genome_parts(plan_, unit_len, n, divergence, seed):
    """(bases (n,) uint8, code before divergence (n,), substituted (n,) bool)."""
    plan_ = np.asarray(plan_, dtype=np.int64)
    n, unit_len = int(n), int(unit_len)
    i = np.arange(n, dtype=np.int64)
    rec = plan_[i // unit_len]
    off = i % unit_len
    f, fwd = (rec >> 1).astype(np.uint64), (rec & 1).astype(bool)
    g = f * np.uint64(unit_len) + np.where(fwd, off, unit_len - 1 - off).astype(np.uint64)
    code = family_codes(g, seed)
    code = np.where(fwd, code, 3 - code)
    thr = int(np.floor(float(divergence) * 2.0 ** 32))
    hit = np.zeros(n, dtype=bool)
    out = code
    if thr:
        lo, hi = sr.split64(i.astype(np.uint64) >> np.uint64(2))
        w = sr._words(sr.philox(lo, hi, 0, 6, *sr._key(seed)), i & 3)
        hit = w < np.uint64(thr)
        out = np.where(hit, (code + 1 + (w % np.uint64(3)).astype(np.int64)) & 3, code)
    return sr.ACGT[out], code, hit


def genome(plan_, unit_len, n, divergence, seed):
    return genome_parts(plan_, unit_len, n, divergence, seed)[0]


def spectrum(bases, k):
    """{o: distinct k-mers occurring o times} of a uint8 genome, forward strand: a host dictionary count."""
    text = bytes(bases)
    counts = {}
    for i in range(len(text) - k + 1):
        key = text[i:i + k]
        counts[key] = counts.get(key, 0) + 1
    out = {}
    for c in counts.values():
        out[c] = out.get(c, 0) + 1
    return out
