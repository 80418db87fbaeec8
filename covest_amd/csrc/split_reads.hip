// split_reads.hip -- K-split: deal the reads into G seeded groups and write them group by group, in input order within
// a group, in the packed layout the k-mer counter takes (covest_split_reads*).  After it "all
// reads but group g" is two sub-ranges of ONE buffer: the delete-a-group jackknife over reads (covest_amd/jackknife.py)
// counts them without a copy.
//
// Read r (64-bit: index in the call + first_read) is of group (w * G) >> 32, w = word 0 of Philox block
// (lo32(r), hi32(r), 0, 8) (sim_philox.h kStreamGroup).
//
// Five launches on the caller's stream, none of which waits for another workgroup:
//   1. split_flags   a workgroup owns kSplitShare reads, kSplitPerLane a lane; a (count, bases) pair a group by integer
//                    atomics in LDS (integer sums do not depend on the order), stored GROUP-MAJOR: row g of the pairs
//                    holds every workgroup's pair of group g
//   2. split_rows    a workgroup a group: the exclusive scan of its row, in place, kSplitScanPass pairs a pass; the row's
//                    total
//   3. split_totals  ONE workgroup: the exclusive scan of the G totals, in place; group_first[0 .. G]; (reads, bases)
//                    for the gather; out_offsets[n_reads] = bases
//   4. split_place   a workgroup its kSplitShare reads again, the group recomputed.  A read's rank among the
//                    workgroup's reads of its group -- the number of EARLIER ones, which is what makes the partition
//                    stable -- is: the groups' counts of the rounds before (LDS), of the waves before in this round
//                    (LDS), and of the lanes before in this wave (a ballot a bit of the group number).  With the ranks
//                    the workgroup's lengths are written to LDS in the order of (group, rank) and scanned there, which
//                    gives every read the bases of its group that lie before it.  A read writes, at its global rank, its
//                    output offset, its global index and its SOURCE offset (scratch)
//   5. the gather (gather_reads.hip launch_gather_reads, which the sampler shares) over that table, through the tile image
// Nothing is written outside d_out_bases[0 .. bases), d_out_offsets[0 .. n_reads], d_read_index[0 .. n_reads),
// d_group_first[0 .. G] and the library's scratch.
#include <hip/hip_runtime.h>

#include "gather_reads.h"
#include "kmer_plan.h"
#include "scan.h"
#include "sim_philox.h"
#include "split.h"

namespace covest {

namespace {

constexpr int kThreads = kSplitThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLane = kSplitPerLane;
constexpr int kMaxG = kSplitMaxGroups;
static_assert(kMaxG <= kThreads, "a lane a group where the groups are walked");
static_assert(kMaxG <= 256, "the in-wave match takes eight ballots");

__device__ __forceinline__ unsigned group_of(unsigned long long r, unsigned groups, uint32_t key0, uint32_t key1)
{
    uint32_t w[4];
    philox_block(r, 0u, kStreamGroup, PhiloxKey{key0, key1}, w);
    return (unsigned)(((unsigned long long)w[0] * groups) >> 32);
}

// The read of lane tid in round j of workgroup blk: the workgroup's reads in input order are round 0's lanes, round 1's, ...
__device__ __forceinline__ long long read_of(long long blk, int j, int tid)
{
    return blk * kSplitShare + (long long)j * kThreads + tid;
}

// ---- 1. pairs[2 * (g * n_blocks + workgroup)] = (reads, bases) of group g among the workgroup's reads
__global__ __launch_bounds__(kThreads) void split_flags_kernel(
    const long long *__restrict__ offsets, const long long read_len, const long long n_reads,
    const unsigned long long first_read, const unsigned groups, const uint32_t key0, const uint32_t key1,
    const long long block0, const long long n_blocks, long long *__restrict__ pairs)
{
    __shared__ unsigned cnt[kMaxG];
    __shared__ unsigned long long len[kMaxG];
    const int tid = threadIdx.x;
    const long long blk = block0 + (long long)blockIdx.x;
    cnt[tid] = 0;
    len[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const long long idx = read_of(blk, j, tid);
        if (idx < n_reads) {
            const unsigned g = group_of(first_read + (unsigned long long)idx, groups, key0, key1);
            atomicAdd(&cnt[g], 1u);
            atomicAdd(&len[g], (unsigned long long)(offsets ? offsets[idx + 1] - offsets[idx] : read_len));
        }
    }
    __syncthreads();
    if ((unsigned)tid < groups) {
        long long *p = pairs + 2 * ((long long)tid * n_blocks + blk);
        p[0] = (long long)cnt[tid];
        p[1] = (long long)len[tid];
    }
}

// ---- 2. exclusive scan of row g of the pairs, in place, by workgroup g; totals[2 * g] = the row's (reads, bases)
__global__ __launch_bounds__(kSplitScanThreads) void split_rows_kernel(long long *__restrict__ pairs, const long long n_blocks,
                                                                       long long *__restrict__ totals)
{
    __shared__ long long wsum[2][kSplitScanThreads / 64];
    long long carry_c, carry_b;
    scan_pair_row<kSplitScanThreads, kSplitScanPerLane>(pairs + 2 * (long long)blockIdx.x * n_blocks, n_blocks, &wsum[0][0],
                                                        carry_c, carry_b);
    if (threadIdx.x == 0) {
        totals[2 * blockIdx.x] = carry_c;
        totals[2 * blockIdx.x + 1] = carry_b;
    }
}

// ---- 3. exclusive scan of the groups' totals, in place: where each group starts, in reads and in bases
__global__ __launch_bounds__(kThreads) void split_totals_kernel(long long *__restrict__ totals, const unsigned groups,
                                                                const long long n_reads, long long *__restrict__ counts,
                                                                long long *__restrict__ group_first,
                                                                long long *__restrict__ out_offsets)
{
    __shared__ long long wsum[2][kWaves];
    const int tid = threadIdx.x;
    const bool in = (unsigned)tid < groups;
    long long e[2] = {in ? totals[2 * tid] : 0, in ? totals[2 * tid + 1] : 0}, all[2];
    block_exclusive_scan<kWaves, 2>(e, &wsum[0][0], all);
    const long long all_b = all[1];
    if (in) {
        totals[2 * tid] = e[0];
        totals[2 * tid + 1] = e[1];
        group_first[tid] = e[0];
    }
    if (tid == 0) {
        group_first[groups] = n_reads;
        counts[0] = n_reads;
        counts[1] = all_b;
        if (out_offsets)
            out_offsets[n_reads] = all_b;
    }
}

// ---- 4. every read to its rank: output offset, global index, source offset
__global__ __launch_bounds__(kThreads) void split_place_kernel(
    const long long *__restrict__ offsets, const long long read_len, const long long n_reads,
    const unsigned long long first_read, const unsigned groups, const uint32_t key0, const uint32_t key1,
    const long long block0, const long long n_blocks, const long long *__restrict__ pairs,
    const long long *__restrict__ totals, long long *__restrict__ out_offsets, long long *__restrict__ read_index,
    long long *__restrict__ src_off)
{
    __shared__ int wcnt[kWaves][kMaxG];   // reads of a group in a wave, this round
    __shared__ int run[kMaxG];            // reads of a group in the rounds so far; in the end the workgroup's
    __shared__ int lstart[kMaxG];         // where a group starts among the workgroup's reads in (group, rank) order
    __shared__ int part[kWaves];
    __shared__ long long base_c[kMaxG], base_b[kMaxG]; // where the workgroup's reads of a group start, in reads and bases
    __shared__ long long lens[kSplitShare];            // lengths in (group, rank) order; then their exclusive scan
    __shared__ long long lpart[kWaves];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long blk = block0 + (long long)blockIdx.x;
    run[tid] = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        wcnt[w][tid] = 0;
    if ((unsigned)tid < groups) {
        const long long *p = pairs + 2 * ((long long)tid * n_blocks + blk);
        base_c[tid] = totals[2 * tid] + p[0];
        base_b[tid] = totals[2 * tid + 1] + p[1];
    }
    __syncthreads();

    unsigned g[kPerLane];
    int lr[kPerLane]; // the read's rank among the workgroup's reads of its group
    long long len[kPerLane], src[kPerLane];
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const long long idx = read_of(blk, j, tid);
        const bool in = idx < n_reads;
        g[j] = 0;
        len[j] = src[j] = 0;
        if (in) {
            g[j] = group_of(first_read + (unsigned long long)idx, groups, key0, key1);
            if (offsets) {
                src[j] = offsets[idx];
                len[j] = offsets[idx + 1] - src[j];
            } else {
                src[j] = idx * read_len;
                len[j] = read_len;
            }
        }
        // the lanes of this wave that hold a read of the same group
        unsigned long long same = __ballot(in);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (g[j] >> bit) & 1u;
            const unsigned long long has = __ballot(set);
            same &= set ? has : ~has;
        }
        if (in && (same & below) == 0)
            wcnt[wave][g[j]] = __popcll(same);
        __syncthreads();
        lr[j] = 0;
        if (in) {
            int r = run[g[j]] + __popcll(same & below);
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                if (w < wave)
                    r += wcnt[w][g[j]];
            lr[j] = r;
        }
        __syncthreads();
        {
            int c = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                c += wcnt[w][tid];
                wcnt[w][tid] = 0;
            }
            run[tid] += c;
        }
        __syncthreads();
    }

    // where each group starts in (group, rank) order: the exclusive scan of run[]
    {
        int all;
        lstart[tid] = block_exclusive_scan<kWaves>(run[tid], part, all);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
        if (read_of(blk, j, tid) < n_reads)
            lens[lstart[g[j]] + lr[j]] = len[j];
    __syncthreads();
    // exclusive scan of the lengths in that order; slots beyond the workgroup's reads are not looked at
    {
        long long v[kPerLane], s = 0;
        const long long have = n_reads - blk * kSplitShare; // reads of this workgroup (kSplitShare or fewer)
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            v[j] = kPerLane * tid + j < have ? lens[kPerLane * tid + j] : 0;
            s += v[j];
        }
        long long all, e = block_exclusive_scan<kWaves>(s, lpart, all);
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            lens[kPerLane * tid + j] = e;
            e += v[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const long long idx = read_of(blk, j, tid);
        if (idx < n_reads) {
            const int first = lstart[g[j]];
            const long long rank = base_c[g[j]] + lr[j];
            if (out_offsets)
                out_offsets[rank] = base_b[g[j]] + lens[first + lr[j]] - lens[first];
            if (read_index)
                read_index[rank] = (long long)(first_read + (unsigned long long)idx);
            src_off[rank] = src[j];
        }
    }
}

} // namespace

size_t split_scratch_bytes(int64_t n_reads, int groups)
{
    const int64_t n_blocks = (n_reads + kSplitShare - 1) / kSplitShare;
    return (size_t)(2 * n_blocks * groups + 2 * groups + 2 + n_reads) * sizeof(long long);
}

hipError_t launch_split_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                              int64_t first_read, int groups, uint64_t seed, unsigned char *out_bases,
                              int64_t *out_offsets, int64_t *read_index, int64_t *group_first, void *scratch,
                              hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    const int64_t n_blocks = (n_reads + kSplitShare - 1) / kSplitShare;
    long long *pairs = static_cast<long long *>(scratch), *totals = pairs + 2 * n_blocks * groups;
    long long *counts = totals + 2 * groups, *src_off = counts + 2;
    const long long *offs = reinterpret_cast<const long long *>(offsets);
    long long *out_offs = reinterpret_cast<long long *>(out_offsets);
    const uint32_t key0 = philox_key(seed).k0, key1 = philox_key(seed).k1;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, n_blocks));
        hipLaunchKernelGGL(split_flags_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, (unsigned)groups, key0, key1, (long long)b0, (long long)n_blocks,
                           pairs);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)groups), dim3(kSplitScanThreads), 0, stream, pairs,
                       (long long)n_blocks, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(split_totals_kernel, dim3(1), dim3(kThreads), 0, stream, totals, (unsigned)groups, (long long)n_reads,
                       counts, reinterpret_cast<long long *>(group_first), out_offs);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, n_blocks));
        hipLaunchKernelGGL(split_place_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, (unsigned)groups, key0, key1, (long long)b0, (long long)n_blocks,
                           pairs, totals, out_offs, reinterpret_cast<long long *>(read_index), src_off);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (!offsets && read_len == 0)
        return hipSuccess; // nothing but empty reads: no byte to move
    return launch_gather_reads(bases, reinterpret_cast<const int64_t *>(counts), offsets ? out_offsets : nullptr, read_len,
                               offsets ? -1 : n_reads * read_len, reinterpret_cast<const int64_t *>(src_off), out_bases,
                               stream);
}

} // namespace covest
