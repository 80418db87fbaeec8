// kmer_influence.h -- the per-read object of every read-level correction: the exact change of
// a sum over the distinct k-mers of a table-valued function of their abundance when ONE read is deleted, and the
// moments of such rows.  k <= 31; read-only on the k-mer table (kmer_table.h), like kmer_lookup.h.
//
// ---- launch_kmer_read_influence ------------------------------------------------------------------------------------
// One wave64 a read, four reads a workgroup of 256 threads, reads with offsets and reads of one length alike; the
// launches are the visits of kmer_plan::for_each_wave_launch.  A window's key is window_key (wave_read.h), so the same
// bytes make the same key as in counting; its abundance a is table_find (the table's 64-bit count).
//
//   table  double[n_rows][n_cols] row-major, n_rows >= 1, 1 <= n_cols <= kInfluenceMaxCols: row i is the value at
//          abundance i, the row of an abundance a is min(a, n_rows - 1).
//   rows   double[n_reads][n_cols + 1]: column c < n_cols is
//              sum over the DISTINCT keys x of the read of  table[row(max(a_x - m_x, 0))][c] - table[row(a_x)][c]
//          with m_x the number of windows of the read whose key is x (deleting the read moves x from a_x to a_x - m_x;
//          a_x < m_x can only happen when the table is not that of these reads and clamps to row 0); the last column is
//          the number of windows W as a double.  A read shorter than k has every column +0.0.
//
// Multiplicity: the wave stages the keys of 64 windows at a time in LDS (an absent window as a key no window has) and
// every lane compares its own window's key with each of the 64, all lanes reading ONE LDS address at a time (a
// broadcast): m is the number of equal keys over the whole read, and a window is FIRST when no window before it has
// its key.  Only a first window looks its key up and contributes; its term is the single subtraction above.
//
// THE ORDER OF THE SUMS IS FIXED, the lookup's: lane l takes windows l, l + 64, ... in ascending order and adds the
// terms of those that are first onto +0.0, per column; the 64 partials are folded by the xor butterfly off = 32, 16,
// ..., 1, p <- p + p[l xor off]; lane 0 stores the row.  No fast-math and no contraction may touch kmer_influence.hip:
// tests hold the rows bit for bit.
//
// Bounded cost: the compare is quadratic in a read's windows (W^2 / 64 compares a lane), and so is the staging: for
// each of its ceil(W / 64) own windows a lane derives the key of one window of every chunk again (window_codes of k
// bases), ceil(W / 64)^2 derivations a lane -- 4 for a 100-base read at k = 21, 4 096 at the cap, where they stay below
// the 262 144 compares beside them.  Keys are not kept from chunk to chunk: 64 chunks of keys do not fit a lane's
// registers, and 32 KiB of LDS a wave would cost the occupancy the table's loads need.  A read with more than
// kInfluenceMaxWindows windows gets NaN in its value columns; W is still written and no compare is done.
//
// LDS: 64 keys of 8 bytes a wave, 2 KiB a workgroup.
//
// ---- launch_rows_moments -------------------------------------------------------------------------------------------
//   rows double[n][q], 1 <= q <= kMomentsMaxQ; centre double[q]; with d_r = rows[r] - centre:
//   sum[k] = sum_r d_r[k];  cross[pair_index(q, k, l)] = sum_r d_r[k] * d_r[l], k <= l (the packed upper triangle of
//   ll_deriv.hip: pair_index(q, k, l) = k q - k (k - 1) / 2 + (l - k)).
//
// No floating-point atomic.  THE SHAPE OF THE REDUCTION IS A FUNCTION OF n ALONE, so the same rows give the same bits
// on every run: block b of 256 threads takes rows [1024 b, 1024 b + 1024); thread t adds rows t, t + 256, t + 512,
// t + 768 of them in ascending order onto +0.0; each wave folds by the xor butterfly 32, ..., 1; thread 0 adds the four
// waves' values in ascending order onto wave 0's and stores the block's partial (scratch: ceil(n / 1024) rows of
// q + q (q + 1) / 2 doubles).  One last block of 256 threads does the same over the partials -- thread t takes partials
// t, t + 256, ... ascending -- and stores sum and cross.  n == 0 gives +0.0 throughout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace covest {

constexpr int kInfluenceMaxCols = 8;
constexpr int64_t kInfluenceMaxWindows = 4096;
constexpr int kMomentsMaxQ = 9;
constexpr int kMomentsBlockRows = 1024;

// Asynchronous on `stream`.
hipError_t launch_kmer_read_influence(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                                      int canonical, const KmerTable &t, const double *table, int64_t n_rows, int n_cols,
                                      double *rows, hipStream_t stream);

inline int moments_width(int q) { return q + q * (q + 1) / 2; }
inline size_t moments_scratch_bytes(int64_t n, int q)
{
    const size_t blocks = (size_t)((n + kMomentsBlockRows - 1) / kMomentsBlockRows);
    return (blocks ? blocks : 1) * (size_t)moments_width(q) * sizeof(double);
}
// Asynchronous on `stream`; `scratch`: moments_scratch_bytes(n, q) bytes, 8-byte aligned.
hipError_t launch_rows_moments(const double *rows, int64_t n, int q, const double *centre, double *sum, double *cross,
                               void *scratch, hipStream_t stream);

} // namespace covest
