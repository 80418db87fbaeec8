// kmer_place.h -- pass 0 of the partitioned k-mer counter, after the count (kmer_bulk.hip includes this once): room per
// bucket and the buckets' places, a prefix sum over the buckets in three launches -- a sum per 1024 buckets, the scan
// of those sums by one workgroup, the places.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "scan.h"

namespace covest {

namespace {

typedef unsigned long long u64;

constexpr int kScanItems = 4;
constexpr int kScanBlock = 256 * kScanItems;

// sampled records of a bucket -> records it gets room for: all of them when everything was counted, else the estimate
// plus three standard deviations of it (the count in a 1-in-s sample of n records scatters by sqrt(n / s))
__device__ __forceinline__ u64 room_for(unsigned sampled, int sample)
{
    if (sample <= 1)
        return sampled;
    const float c = (float)sampled;
    return (u64)((float)sample * (c + 3.0f * sqrtf(c) + 2.0f));
}

// the rooms of a thread's kScanItems buckets, `first` the first of them; returns their sum
__device__ __forceinline__ u64 thread_rooms(const KmerBulk &p, unsigned first, u64 (&room)[kScanItems])
{
    u64 sum = 0;
    for (int j = 0; j < kScanItems; ++j) {
        room[j] = room_for(p.sampled[first + j], p.sample);
        sum += room[j];
    }
    return sum;
}

__global__ __launch_bounds__(256) void kmer_caps_partial_kernel(const KmerBulk p, u64 *__restrict__ partial)
{
    __shared__ u64 lds[4];
    u64 room[kScanItems], total;
    block_exclusive_scan<4>(thread_rooms(p, blockIdx.x * kScanBlock + threadIdx.x * kScanItems, room), lds, total);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = total;
}

// one workgroup: partial[] -> its exclusive prefix, in place; out[0] = the total
__global__ __launch_bounds__(256) void kmer_caps_scan_kernel(u64 *__restrict__ partial, unsigned n, u64 *__restrict__ out)
{
    __shared__ u64 lds[4];
    const unsigned per = (n + 255u) / 256u;
    const unsigned first = threadIdx.x * per;
    u64 mine = 0;
    for (unsigned j = first; j < first + per && j < n; ++j)
        mine += partial[j];
    u64 total;
    u64 run = block_exclusive_scan<4>(mine, lds, total);
    for (unsigned j = first; j < first + per && j < n; ++j) {
        const u64 v = partial[j];
        partial[j] = run;
        run += v;
    }
    if (threadIdx.x == 0)
        out[0] = total;
}

__global__ __launch_bounds__(256) void kmer_caps_place_kernel(const KmerBulk p, const u64 *__restrict__ partial)
{
    __shared__ u64 lds[4];
    const unsigned first = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    u64 room[kScanItems], total;
    u64 at = partial[blockIdx.x] + block_exclusive_scan<4>(thread_rooms(p, first, room), lds, total);
    for (int j = 0; j < kScanItems; ++j) {
        p.ctl[first + j] = make_ulonglong2(at, at + room[j]);
        at += room[j];
    }
}

} // namespace

} // namespace covest
