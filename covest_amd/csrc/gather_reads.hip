// gather_reads.hip -- the gather of the packed-reads layer: a table of reads (a source offset and an output offset a
// read, the counts on the device) to one packed run of bases.  The last launch and the hot path of the sampler
// (sample_reads.hip) and of the split (split_reads.hip, section 6aa).
//
// The output goes through the tile image (tile_image.h); a fixed number of workgroups each walks a contiguous share of
// the tiles (their count is known on the device only).  A workgroup finds the read that holds its first byte by a
// 256-way search of the output offsets (once: from tile to tile the place is carried), loads the offsets of the reads
// that touch the tile into LDS, kBatch at a time (a run of empty reads is only more batches), and assembles the tile in
// an LDS image: a lane an aligned image dword; the read is found by a binary search in the LDS table; a dword that lies
// within one read is two aligned source dwords (one where the source is aligned too) funnel-shifted into one aligned
// LDS store; a dword that straddles reads, or the ends of the output, is assembled byte by byte from aligned source
// dwords -- byte stores happen in LDS.
// An aligned source dword is loaded only when it holds a byte that is wanted, so no load leaves the 4-byte granule of
// a byte of the caller's buffer.  Nothing is written outside out_bases[0 .. counts[1]).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_reads.h"
#include "tile_image.h"

namespace covest {

namespace {

constexpr int kThreads = kImageThreads;         // the gather's workgroup is the tile image's
constexpr int kBatch = kThreads;                // reads whose offsets the workgroup holds in LDS at a time

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

hipError_t launch_gather_reads(const unsigned char *bases, const int64_t *counts, const int64_t *out_offsets,
                               int64_t read_len, int64_t most_bases, const int64_t *src_off, unsigned char *out_bases,
                               hipStream_t stream)
{
    // the tile count is known on the device only: a fixed number of workgroups share the tiles (fewer where the
    // upper bound the caller knows has fewer tiles)
    int64_t n_groups = kGatherGroups;
    if (most_bases >= 0)
        n_groups = std::min<int64_t>(n_groups, image_tiles(most_bases, 15));
    const int lead = image_lead(out_bases);
    hipLaunchKernelGGL(sample_gather_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0, stream, bases,
                       reinterpret_cast<const long long *>(counts), reinterpret_cast<const long long *>(out_offsets),
                       (long long)read_len, reinterpret_cast<const long long *>(src_off), out_bases, lead);
    return hipGetLastError();
}

} // namespace covest
