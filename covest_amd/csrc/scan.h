// scan.h -- prefix sums of a wave and of a workgroup, and the in-place scan of a row of (count, bases) pairs: what the
// sampler (sample_reads.hip), the split (split_reads.hip) and the partitioned counter's places (kmer_place.h) share
// (DESIGN.md section 6ag).  Device only; wave64.
#pragma once
#include <hip/hip_runtime.h>

namespace covest {

// inclusive scan over the wave's 64 lanes
template <class T> __device__ __forceinline__ T wave_inclusive_scan(T v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(v, off, 64);
        if (lane >= off)
            v += up;
    }
    return v;
}

// Exclusive scan of K values at once over the WAVES * 64 threads of the workgroup, in thread order: v[k] comes back as
// the sum of the v[k] of the threads before, total[k] as the sum over all of them.  lds: K * WAVES words, value k's at
// lds[k * WAVES ..]; one barrier, between the waves' sums going in and being read.
// The contract: the block is FREE on entry -- there is no leading barrier -- so a second call on the same block needs
// a barrier of the caller's in between (the threads of the first may still be reading it).
template <int WAVES, int K, class T> __device__ __forceinline__ void block_exclusive_scan(T (&v)[K], T *lds, T (&total)[K])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc[K];
#pragma unroll
    for (int k = 0; k < K; ++k)
        inc[k] = wave_inclusive_scan(v[k], lane);
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            lds[k * WAVES + wave] = inc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = inc[k] - v[k];
        total[k] = 0;
    }
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T s = lds[k * WAVES + w];
            if (w < wave)
                v[k] += s;
            total[k] += s;
        }
}

// ... and of one value; returns the exclusive prefix
template <int WAVES, class T> __device__ __forceinline__ T block_exclusive_scan(T v, T *lds, T &total)
{
    T one[1] = {v}, all[1];
    block_exclusive_scan<WAVES, 1>(one, lds, all);
    total = all[0];
    return one[0];
}

// The exclusive scan, in place, of a row of n (count, bases) pairs by ONE workgroup of THREADS threads: a pass takes
// THREADS * PER_LANE pairs, PER_LANE consecutive ones a lane, and carries the sums of the passes before.  total_c /
// total_b: the row's sums, in every lane.  lds: 2 * (THREADS / 64) words, free on entry and free again on return.
template <int THREADS, int PER_LANE>
__device__ __forceinline__ void scan_pair_row(long long *row, const long long n, long long *lds, long long &total_c,
                                              long long &total_b)
{
    const int tid = threadIdx.x;
    long long carry_c = 0, carry_b = 0; // (uniform: every lane keeps its own copy)
    for (long long base = 0; base < n; base += (long long)THREADS * PER_LANE) {
        const long long at = base + (long long)tid * PER_LANE;
        long long c[PER_LANE], b[PER_LANE], s[2] = {0, 0}, all[2];
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const bool in = at + j < n;
            c[j] = in ? row[2 * (at + j)] : 0;
            b[j] = in ? row[2 * (at + j) + 1] : 0;
            s[0] += c[j];
            s[1] += b[j];
        }
        block_exclusive_scan<THREADS / 64, 2>(s, lds, all);
        long long ec = carry_c + s[0], eb = carry_b + s[1];
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            if (at + j < n) {
                row[2 * (at + j)] = ec;
                row[2 * (at + j) + 1] = eb;
            }
            ec += c[j];
            eb += b[j];
        }
        carry_c += all[0];
        carry_b += all[1];
        __syncthreads(); // (lds is written again in the next pass)
    }
    total_c = carry_c;
    total_b = carry_b;
}

} // namespace covest
