// wave_read.h -- a wave64 a read, kWaveReadsPerBlock reads a workgroup: how the kernels that walk packed reads against
// the k-mer table open a read, and a window's key.  Their launches: kmer_plan::for_each_wave_launch.
// The kernels that change the table walk a read by kmer_update.h, which stands on this file.
#pragma once
#include "kmer_table.h"

namespace covest {
namespace kmer {

constexpr int kWaveReadsPerBlock = 4;

struct WaveRead {
    int lane;
    int64_t r, p0, len, n_windows; // the read, from the launch's first on; its first byte; its bases; its windows (0:
    const unsigned char *seq;      //   shorter than k); bases + p0
};

// false: no read for this wave, the whole wave leaves.  (kmer_correct.hip keeps these lines with a scalar wave index.)
__device__ __forceinline__ bool wave_read(const unsigned char *bases, const int64_t *__restrict__ offsets, int64_t n_reads,
                                          int64_t fixed_len, int k, WaveRead &w)
{
    w.lane = threadIdx.x & (kWave - 1);
    w.r = (int64_t)blockIdx.x * kWaveReadsPerBlock + threadIdx.x / kWave;
    if (w.r >= n_reads)
        return false;
    w.p0 = offsets ? offsets[w.r] : w.r * fixed_len;
    w.len = offsets ? offsets[w.r + 1] - w.p0 : fixed_len;
    w.n_windows = w.len >= k ? w.len - k + 1 : 0;
    w.seq = bases + w.p0;
    return true;
}

// the key of the window at seq[s]: its code and the reverse complement's, the smaller first where the table is canonical
__device__ __forceinline__ void window_key(const unsigned char *__restrict__ seq, int64_t s, int64_t len, int k, int canonical,
                                           unsigned long long &h, unsigned long long &rc)
{
    window_codes(seq, s, len, k, h, rc);
    canonical_pair(h, rc, canonical);
}

} // namespace kmer
} // namespace covest
