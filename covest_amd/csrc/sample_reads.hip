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
//   4. sample_gather  the hot path.  The output goes through the tile image (tile_image.h); a fixed number of
//                     workgroups each walks a contiguous share of the tiles (their count is known on the device
//                     only).  A workgroup finds the kept read that holds its first byte by a 256-way search of the output
//                     offsets (once: from tile to tile the place is carried), loads the offsets of the kept reads that
//                     touch the tile into LDS, kBatch at a time (a run of empty reads is only more batches), and
//                     assembles the tile in an LDS image: a lane an aligned image dword; the read is found by a binary
//                     search in the LDS table; a dword that lies within one read is two aligned source dwords (one
//                     where the source is aligned too) funnel-shifted into one aligned LDS store; a dword that straddles
//                     reads, or the ends of the output, is assembled byte by byte from aligned source dwords -- byte
//                     stores happen in LDS.
// An aligned source dword is loaded only when it holds a byte that is wanted, so no load leaves the 4-byte granule of
// a byte of the caller's buffer.  Nothing is written outside d_out_bases[0 .. bases_kept), d_out_offsets[0 .. n_kept],
// d_kept_index[0 .. n_kept), d_counts[0 .. 2) and the library's scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sample.h"
#include "sim_philox.h"
#include "tile_image.h"

namespace covest {

namespace {

constexpr int kThreads = kSampleShare;          // reads a workgroup of stages 1 and 3 owns, one a lane
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;
constexpr int kScanPerLane = 4;                 // pairs a lane of the scan takes per round
static_assert(kThreads == kImageThreads, "the gather's workgroup is the tile image's");
constexpr int kBatch = kThreads;                // kept reads whose offsets the workgroup holds in LDS at a time
constexpr int64_t kBlocksPerLaunch = (int64_t)1 << 22; // 2^30 threads a launch (HIP wraps grids beyond 2^32 threads)

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

// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ long long wave_scan_i64(long long v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long up = __shfl_up(v, off, 64);
        if (lane >= off)
            v += up;
    }
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry_c = 0, carry_b = 0; // (uniform: every lane keeps its own copy)
    for (long long base = 0; base < n_blocks; base += (long long)kScanThreads * kScanPerLane) {
        const long long at = base + (long long)tid * kScanPerLane;
        long long c[kScanPerLane], b[kScanPerLane], sc = 0, sb = 0;
#pragma unroll
        for (int j = 0; j < kScanPerLane; ++j) {
            const bool in = at + j < n_blocks;
            c[j] = in ? pairs[2 * (at + j)] : 0;
            b[j] = in ? pairs[2 * (at + j) + 1] : 0;
            sc += c[j];
            sb += b[j];
        }
        const long long ic = wave_scan_i64(sc, lane), ib = wave_scan_i64(sb, lane);
        if (lane == 63) {
            wsum[0][wave] = ic;
            wsum[1][wave] = ib;
        }
        __syncthreads();
        long long before_c = 0, before_b = 0, all_c = 0, all_b = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const long long wc = wsum[0][w], wb = wsum[1][w];
            if (w < wave) {
                before_c += wc;
                before_b += wb;
            }
            all_c += wc;
            all_b += wb;
        }
        long long ec = carry_c + before_c + ic - sc, eb = carry_b + before_b + ib - sb;
#pragma unroll
        for (int j = 0; j < kScanPerLane; ++j) {
            if (at + j < n_blocks) {
                pairs[2 * (at + j)] = ec;
                pairs[2 * (at + j) + 1] = eb;
            }
            ec += c[j];
            eb += b[j];
        }
        carry_c += all_c;
        carry_b += all_b;
        __syncthreads(); // (wsum is written again in the next round)
    }
    if (tid == 0) {
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    const long long ic = wave_scan_i64(cnt, lane), ib = wave_scan_i64(len, lane);
    if (lane == 63) {
        part[0][wave] = ic;
        part[1][wave] = ib;
    }
    __syncthreads();
    long long rank = pairs[2 * blk] + ic - cnt, at = pairs[2 * blk + 1] + ib - len;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) {
            rank += part[0][w];
            at += part[1][w];
        }
    if (cnt) {
        if (out_offsets)
            out_offsets[rank] = at;
        if (kept_index)
            kept_index[rank] = (long long)(first_read + (unsigned long long)idx);
        src_off[rank] = src;
    }
}

// ---- 4. the gather
// out_off == nullptr: every read has read_len (> 0) bases, the output offset of rank q is q * read_len
__device__ __forceinline__ long long off_of(const long long *__restrict__ out_off, long long read_len, long long q)
{
    return out_off ? out_off[q] : q * read_len;
}

__device__ __forceinline__ unsigned src_byte(const unsigned char *__restrict__ src, long long a)
{
    const unsigned char *p = src + a;
    const unsigned sh = (unsigned)((uintptr_t)p & 3u);
    return (*reinterpret_cast<const unsigned *>(p - sh) >> (8u * sh)) & 0xffu;
}

__global__ __launch_bounds__(kThreads) void sample_gather_kernel(
    const unsigned char *__restrict__ src, const long long *__restrict__ counts, const long long *__restrict__ out_off,
    const long long read_len, const long long *__restrict__ src_off, unsigned char *__restrict__ out, const int lead)
{
    __shared__ __attribute__((aligned(16))) unsigned char image[kImageTile];
    __shared__ int rel[kBatch + 1];       // output offset of the batch's reads less the tile's, kept within [0, kImageTile + 1]
    __shared__ long long delta[kBatch];   // source offset less output offset

    const int tid = threadIdx.x;
    const long long n_kept = counts[0], total = counts[1];
    if (total <= 0)
        return;
    const long long n_tiles = image_tiles(total, lead);
    const long long share = (n_tiles + gridDim.x - 1) / gridDim.x;
    const long long tile_lo = (long long)blockIdx.x * share;
    const long long tile_hi = tile_lo + share < n_tiles ? tile_lo + share : n_tiles;
    if (tile_lo >= tile_hi)
        return; // (uniform)

    // the last rank whose output offset is not beyond the share's first byte: rank 0 has offset 0
    long long r0;
    {
        const long long target = tile_span(tile_lo, lead, total).o_begin;
        if (!out_off) {
            r0 = target / read_len;
        } else {
            long long lo = 0, hi = n_kept; // off(lo) <= target; the answer is in [lo, hi)
            while (hi - lo > 1) {
                const long long step = (hi - lo + kThreads - 1) / kThreads;
                const long long q = lo + (long long)(tid + 1) * step;
                const int c = __syncthreads_count(q < hi && out_off[q] <= target); // (ascending: the first c lanes)
                const long long top = lo + (long long)(c + 1) * step;
                lo += (long long)c * step;
                hi = top < hi ? top : hi;
            }
            r0 = lo;
        }
        if (r0 > n_kept - 1)
            r0 = n_kept - 1;
    }

    for (long long tile = tile_lo; tile < tile_hi; ++tile) {
        // the caller's part of the tile, in the image's coordinates: [e_begin, e_end)
        const TileSpan span = tile_span(tile, lead, total);
        const long long t_begin = span.t_begin;
        const int e_begin = (int)(span.o_begin - t_begin), e_end = (int)(span.o_end - t_begin);
        long long rb0 = r0;
        int cnt;
        for (;;) {
            cnt = n_kept - rb0 < kBatch ? (int)(n_kept - rb0) : kBatch; // >= 1
            for (int i = tid; i <= cnt; i += kThreads) {
                const long long o = rb0 + i < n_kept ? off_of(out_off, read_len, rb0 + i) : total;
                const long long d = o - t_begin;
                rel[i] = d < 0 ? 0 : d > kImageTile + 1 ? kImageTile + 1 : (int)d;
                if (i < cnt)
                    delta[i] = src_off[rb0 + i] - o;
            }
            __syncthreads();
            const int p_lo = rel[0] > e_begin ? rel[0] : e_begin; // the batch's share of the image: [p_lo, p_hi)
            const int p_hi = rel[cnt] < e_end ? rel[cnt] : e_end;
#pragma unroll
            for (int k = 0; k < kImageTile / (4 * kThreads); ++k) {
                const int p = 4 * (tid + kThreads * k);
                if (p + 4 <= p_lo || p >= p_hi)
                    continue;
                const int first = p > p_lo ? p : p_lo;
                int i = 0, hi = cnt; // the last read of the batch that starts at or before `first`: rel[0] <= first
                while (hi - i > 1) {
                    const int mid = (i + hi) >> 1;
                    if (rel[mid] <= first)
                        i = mid;
                    else
                        hi = mid;
                }
                const int r_end = rel[i + 1] < p_hi ? rel[i + 1] : p_hi;
                if (p >= p_lo && p + 4 <= r_end) {
                    const unsigned char *a = src + (delta[i] + t_begin + p);
                    const unsigned sh = (unsigned)((uintptr_t)a & 3u);
                    const unsigned *w = reinterpret_cast<const unsigned *>(a - sh);
                    unsigned v = w[0];
                    if (sh)
                        v = (v >> (8u * sh)) | (w[1] << (32u - 8u * sh));
                    *reinterpret_cast<unsigned *>(image + p) = v;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int pb = p + b;
                        if (pb < p_lo || pb >= p_hi)
                            continue;
                        while (rel[i + 1] <= pb) // (rel[cnt] >= p_hi > pb: i + 1 stays within the table)
                            ++i;
                        image[pb] = (unsigned char)src_byte(src, delta[i] + t_begin + pb);
                    }
                }
            }
            const bool done = rel[cnt] >= e_end || rb0 + cnt >= n_kept;
            if (done)
                break; // (uniform; the table stays for the step below)
            __syncthreads();
            rb0 += cnt;
        }
        // where the next tile starts: the last read of the table that starts at or before this tile's end
        {
            int i = 0, hi = cnt + 1;
            while (hi - i > 1) {
                const int mid = (i + hi) >> 1;
                if (rel[mid] <= e_end)
                    i = mid;
                else
                    hi = mid;
            }
            r0 = rb0 + i < n_kept - 1 ? rb0 + i : n_kept - 1;
        }
        __syncthreads(); // the image is whole; the table is free

        store_image(out, image, span, tid);
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
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kBlocksPerLaunch) {
        const dim3 grid((unsigned)std::min(n_blocks - b0, kBlocksPerLaunch));
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
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kBlocksPerLaunch) {
        const dim3 grid((unsigned)std::min(n_blocks - b0, kBlocksPerLaunch));
        hipLaunchKernelGGL(sample_place_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, (unsigned long long)thr, key0, key1, (long long)b0, pairs,
                           reinterpret_cast<long long *>(out_offsets), reinterpret_cast<long long *>(kept_index), src_off);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (!offsets && read_len == 0)
        return hipSuccess; // nothing but empty reads: no byte to move
    return launch_sample_gather(bases, counts, offsets ? out_offsets : nullptr, read_len,
                                offsets ? -1 : n_reads * read_len, reinterpret_cast<const int64_t *>(src_off), out_bases, stream);
}

hipError_t launch_sample_gather(const unsigned char *bases, const int64_t *counts, const int64_t *out_offsets,
                                int64_t read_len, int64_t most_bases, const int64_t *src_off, unsigned char *out_bases,
                                hipStream_t stream)
{
    // the tile count is known on the device only: a fixed number of workgroups share the tiles (fewer where the
    // upper bound the caller knows has fewer tiles)
    int64_t n_groups = kSampleGatherGroups;
    if (most_bases >= 0)
        n_groups = std::min<int64_t>(n_groups, image_tiles(most_bases, 15));
    const int lead = image_lead(out_bases);
    hipLaunchKernelGGL(sample_gather_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0, stream, bases,
                       reinterpret_cast<const long long *>(counts), reinterpret_cast<const long long *>(out_offsets),
                       (long long)read_len, reinterpret_cast<const long long *>(src_off), out_bases, lead);
    return hipGetLastError();
}

} // namespace covest
