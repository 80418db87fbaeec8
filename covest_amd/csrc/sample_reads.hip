// sample_reads.hip -- K-sample: keep every read with probability 1 / factor and compact the kept ones, in input order,
// into the packed layout the k-mer counter takes (covest_sample_reads*).
//
// The counterpart of the reference's covest/data.py:57-63 (sample_reads), with the deliberate difference of section 6l:
// where the reference draws from Python's unseeded `random`, read r (64-bit: index in the call + first_read) is kept iff
// word 0 of Philox block (lo32(r), hi32(r), 0, 2) is below thr = floor((1 / factor) * 2^32) (sim_philox.h; the
// simulator's blocks end in (.., 0, 1) and (.., j, 0)).
//
// Four launches on the caller's stream, none of which waits for another workgroup:
//   1. sample_flags   a lane a read: its flag and kept length; a (count, bases) pair a workgroup by a block reduction
//   2. sample_scan    ONE workgroup: the exclusive scan of the pairs, in place; the totals to d_counts, and
//                     d_out_offsets[n_kept] = bases kept
//   3. sample_place   a lane a read again: the flag recomputed (a Philox block is cheaper than a stored flag read back),
//                     a scan within the workgroup; a kept read writes, at its rank, its output offset, its global index
//                     and its SOURCE offset (scratch: the gather never reads d_offsets)
//   4. the gather     the hot path, in a file of its own: gather_reads.hip (launch_gather_reads), which the split shares
// Nothing is written outside d_out_bases[0 .. bases_kept), d_out_offsets[0 .. n_kept], d_kept_index[0 .. n_kept),
// d_counts[0 .. 2) and the library's scratch.
#include <hip/hip_runtime.h>

#include "gather_reads.h"
#include "kmer_plan.h"
#include "sample.h"
#include "scan.h"
#include "sim_philox.h"

namespace covest {

namespace {

constexpr int kThreads = kSampleShare;          // reads a workgroup of stages 1 and 3 owns, one a lane
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;
constexpr int kScanPerLane = 4;                 // pairs a lane of the scan takes per round

__device__ __forceinline__ bool kept(unsigned long long r, unsigned long long thr, uint32_t key0, uint32_t key1)
{
    uint32_t w[4];
    philox_block(r, 0u, kStreamKeep, PhiloxKey{key0, key1}, w);
    return (unsigned long long)w[0] < thr;
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// ---- 1. flags and kept lengths: pairs[2 * workgroup] = (reads kept, bases kept)
__global__ __launch_bounds__(kThreads) void sample_flags_kernel(
    const long long *__restrict__ offsets, const long long read_len, const long long n_reads,
    const unsigned long long first_read, const unsigned long long thr, const uint32_t key0, const uint32_t key1,
    const long long block0, long long *__restrict__ pairs)
{
    __shared__ long long part[2][kWaves];
    const int tid = threadIdx.x;
    const long long blk = block0 + (long long)blockIdx.x;
    const long long idx = blk * kThreads + tid;
    long long cnt = 0, len = 0;
    if (idx < n_reads && kept(first_read + (unsigned long long)idx, thr, key0, key1)) {
        cnt = 1;
        len = offsets ? offsets[idx + 1] - offsets[idx] : read_len;
    }
    cnt = wave_sum_i64(cnt);
    len = wave_sum_i64(len);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = cnt;
        part[1][tid >> 6] = len;
    }
    __syncthreads();
    if (tid == 0) {
        long long c = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            c += part[0][w];
            b += part[1][w];
        }
        pairs[2 * blk] = c;
        pairs[2 * blk + 1] = b;
    }
}

// ---- 2. exclusive scan of the pairs, in place, by one workgroup; the totals
__global__ __launch_bounds__(kScanThreads) void sample_scan_kernel(long long *__restrict__ pairs, const long long n_blocks,
                                                                   long long *__restrict__ counts,
                                                                   long long *__restrict__ out_offsets)
{
    __shared__ long long wsum[2][kScanThreads / 64];
    long long carry_c, carry_b;
    scan_pair_row<kScanThreads, kScanPerLane>(pairs, n_blocks, &wsum[0][0], carry_c, carry_b);
    if (threadIdx.x == 0) {
        counts[0] = carry_c;
        counts[1] = carry_b;
        if (out_offsets)
            out_offsets[carry_c] = carry_b;
    }
}

// ---- 3. every kept read to its rank: output offset, global index, source offset
__global__ __launch_bounds__(kThreads) void sample_place_kernel(
    const long long *__restrict__ offsets, const long long read_len, const long long n_reads,
    const unsigned long long first_read, const unsigned long long thr, const uint32_t key0, const uint32_t key1,
    const long long block0, const long long *__restrict__ pairs, long long *__restrict__ out_offsets,
    long long *__restrict__ kept_index, long long *__restrict__ src_off)
{
    __shared__ long long part[2][kWaves];
    const int tid = threadIdx.x;
    const long long blk = block0 + (long long)blockIdx.x;
    const long long idx = blk * kThreads + tid;
    long long cnt = 0, len = 0, src = 0;
    if (idx < n_reads && kept(first_read + (unsigned long long)idx, thr, key0, key1)) {
        cnt = 1;
        if (offsets) {
            src = offsets[idx];
            len = offsets[idx + 1] - src;
        } else {
            src = idx * read_len;
            len = read_len;
        }
    }
    long long before[2] = {cnt, len}, all[2]; // the workgroup's kept reads, and their bases, before this one
    block_exclusive_scan<kWaves, 2>(before, &part[0][0], all);
    const long long rank = pairs[2 * blk] + before[0], at = pairs[2 * blk + 1] + before[1];
    if (cnt) {
        if (out_offsets)
            out_offsets[rank] = at;
        if (kept_index)
            kept_index[rank] = (long long)(first_read + (unsigned long long)idx);
        src_off[rank] = src;
    }
}

} // namespace

size_t sample_scratch_bytes(int64_t n_reads)
{
    const int64_t n_blocks = (n_reads + kThreads - 1) / kThreads;
    return (size_t)(2 * n_blocks + n_reads) * sizeof(long long);
}

hipError_t launch_sample_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                               int64_t first_read, uint64_t thr, uint64_t seed, unsigned char *out_bases,
                               int64_t *out_offsets, int64_t *kept_index, int64_t *counts, void *scratch,
                               hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    const int64_t n_blocks = (n_reads + kThreads - 1) / kThreads;
    long long *pairs = static_cast<long long *>(scratch), *src_off = pairs + 2 * n_blocks;
    const long long *offs = reinterpret_cast<const long long *>(offsets);
    const uint32_t key0 = philox_key(seed).k0, key1 = philox_key(seed).k1;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, n_blocks));
        hipLaunchKernelGGL(sample_flags_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, (unsigned long long)thr, key0, key1, (long long)b0, pairs);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, pairs, (long long)n_blocks,
                       reinterpret_cast<long long *>(counts), reinterpret_cast<long long *>(out_offsets));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, n_blocks));
        hipLaunchKernelGGL(sample_place_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, (unsigned long long)thr, key0, key1, (long long)b0, pairs,
                           reinterpret_cast<long long *>(out_offsets), reinterpret_cast<long long *>(kept_index), src_off);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (!offsets && read_len == 0)
        return hipSuccess; // nothing but empty reads: no byte to move
    return launch_gather_reads(bases, counts, offsets ? out_offsets : nullptr, read_len,
                               offsets ? -1 : n_reads * read_len, reinterpret_cast<const int64_t *>(src_off), out_bases, stream);
}

} // namespace covest
