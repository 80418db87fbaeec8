"""Replicate histograms drawn from a weight vector, restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the definition in include/covest_amd.h, not from the kernel:
  thresholds: cdf = cumsum(w) strictly left to right; r_i = cdf_i / cdf_{m-1}; t_i = floor(r_i * 2^63) as uint64.
  draw d of replicate b: Philox4x32-10 (sim_reference.philox) on the counter (lo32(d>>1), hi32(d>>1), b, 7) under the
    key (lo32(seed), hi32(seed)) -> w0..w3; an even d uses u = (w0 | w1 << 32) >> 1, an odd d u = (w2 | w3 << 32) >> 1;
    its cell is the number of i in 0 .. m - 2 with t_i <= u.
  counts[b - first_rep][i] = the number of draws d < n of replicate b in cell i (int64).
"""
import numpy as np

from sim_reference import _key, philox, split64

STREAM_DRAW = 7


def thresholds(weights):
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    cdf = np.cumsum(w)  # one-dimensional doubles: a plain running sum, left to right
    r = cdf / cdf[-1]
    return np.floor(r * 2.0 ** 63).astype(np.uint64)


def draws(n, replicate, seed):
    """u of the draws 0 .. n - 1 of one replicate: a uint64 array."""
    k0, k1 = _key(seed)
    blocks = np.arange((n + 1) // 2, dtype=np.uint64)
    lo, hi = split64(blocks)
    w0, w1, w2, w3 = philox(lo, hi, np.uint64(replicate), np.uint64(STREAM_DRAW), k0, k1)
    u = np.empty(2 * len(blocks), dtype=np.uint64)
    u[0::2] = (w0 | (w1 << np.uint64(32))) >> np.uint64(1)
    u[1::2] = (w2 | (w3 << np.uint64(32))) >> np.uint64(1)
    return u[:n]


def draw_histograms(weights, n, replicates, seed=0, first_replicate=0):
    t = thresholds(weights)
    m = len(t)
    out = np.zeros((replicates, m), dtype=np.int64)
    for row in range(replicates):
        u = draws(n, first_replicate + row, seed)
        cells = np.searchsorted(t[:m - 1], u, side="right")  # #{i <= m - 2 : t_i <= u}
        out[row] = np.bincount(cells, minlength=m)
    return out
