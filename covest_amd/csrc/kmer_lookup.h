// kmer_lookup.h -- the read-only walk of the k-mer table (k <= 31, kmer_table.h): for every window of every read the
// count the table holds for its key, and three reductions of those counts per read.
//
// One wave64 a read, four reads a workgroup of 256 threads, reads with offsets and reads of one length alike.  Lane l
// takes windows l, l + 64, ... in ascending order; a window's codes are window_codes + canonical_pair, so the same
// bytes make the same key as in counting, and its count is table_find.  Nothing is stored to the table.
//
// Every output is optional (null: not wanted):
//   abundance  uint32, indexed like the bases (offsets[r] + s; reads of one length: r * read_len + s).  The entry at
//              a window's first base is min(count, kNoWindow - 1); the last k - 1 positions of a read -- all of a read
//              shorter than k -- hold kNoWindow, "no window starts here".  Every position of every read is written
//              exactly once and nothing else is.
//   summary    uint32[n_reads][4] = {min_abundance, weak, first_weak, last_weak}, one 16-byte store by lane 0: the
//              smallest abundance, the number of windows with abundance < cutoff, the first and the last of them
//              (window indices).  No window: {kNoWindow, 0, kNoWindow, kNoWindow}; no weak window: both indices
//              kNoWindow; cutoff 0: no window is weak.  A read has fewer than 2^32 - 1 windows.
//   score      double[n_reads] = sum over the windows of weights[min(abundance, n_weights - 1)], the abundance being
//              the table's 64-bit count, n_weights >= 1.  THE ORDER OF THE SUM IS FIXED: lane l adds its windows in
//              ascending order onto +0.0; the 64 partials are folded by the xor butterfly off = 32, 16, ..., 1,
//              p <- p + p[l xor off] (IEEE addition commutes, so all lanes hold the same bits); lane 0 stores.  A read
//              without windows scores +0.0.  No fast-math may touch this file: tests hold the sum bit for bit.
//
// Reads shorter than k: the counter counts "the hash of what there is" for such a read (bin/kmer_hist.py:36-37 of the
// reference).  The lookup deliberately does NOT look that key up: such a read has no k-mer to judge.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace covest {

constexpr uint32_t kNoWindow = 0xFFFFFFFFu;

// Asynchronous on `stream`; the launches are the visits of kmer_plan::for_each_wave_launch (a wave a read: wave_read.h).
hipError_t launch_kmer_lookup(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                              int canonical, const KmerTable &t, uint32_t cutoff, const double *weights, int n_weights,
                              uint32_t *abundance, uint32_t *summary, double *score, hipStream_t stream);

} // namespace covest
