// kmer_scatter.h -- passes 0 and 1 of the partitioned k-mer counter (kmer_bulk.hip, which includes this once): the
// bucket of a k-mer, a record behind its bucket's cursor, and the tile kernel as a walk over stages --
//     load      the 16 bases from the thread's byte on                                      load_bases16
//     classify  {the byte's m-mer is whole, the byte starts a window of this launch}        classify_fixed / _ragged
//     bucket    the smallest of the window's w m-mer hashes names it                        window_bucket
//     run       a head lane's windows, from the waves' ballots                              kmer_runs.h run_length
//     emit      pass 0: the run's pieces counted; pass 1: a record a piece                  for_each_piece, piece,
//                                                                                           store_record
// -- and the reads shorter than k, a thread each.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kmer_runs.h"
#include "kmer_table.h"
#include "wave.h"

namespace covest {

namespace {

using namespace kmer;
typedef unsigned long long u64;

using kmer_plan::kTile;          // bytes (threads) of a tile of pass 0/1
using kmer_plan::kTilesPerBlock; // consecutive tiles a workgroup works through (the unit of the sample), one at a time.
// (Measured at 10 Gbp with 1, 2 and 4 tiles side by side, a wave's atomics of all of them in flight together: 1 and 2
// the same, 18.5-18.9 ms a launch, 4 slower, 20.6-21.4 with 80 VGPRs -- the memory side's atomic rate is the bound, more
// atomics in flight per wave buy nothing.  The option is gone for that reason.)
constexpr unsigned kNoBucket = ~0u;

// ---- the bucket of a k-mer ---------------------------------------------------------------------------------------
// m-mers as little-endian codes (base j at bits 2j).  The smaller of one and its reverse complement:
__device__ __forceinline__ unsigned mmer_canonical(unsigned x, int m, int canonical)
{
    if (!canonical)
        return x;
    const unsigned r = reverse_pairs32(~x) >> (32 - 2 * m);
    return r < x ? r : x;
}

__device__ __forceinline__ unsigned mmer_hash(unsigned c)
{
    const unsigned h = (c + 1u) * 0x9E3779B1u; // (a bijection: different m-mers never tie)
    return h ^ (h >> 15);
}

__device__ __forceinline__ unsigned bucket_of_min(unsigned mn, int log2_buckets)
{
    unsigned h = mn * 0x85EBCA77u; // (the minimum of w hashes is small: spread it again)
    h ^= h >> 13;
    h *= 0xC2B2AE3Du;
    return h >> (32 - log2_buckets);
}

// The bucket of ONE window from its little-endian code (the slow way: pass 1's tiles share the m-mer hashes between
// windows).  The rc of the k-mer holds the rc's of its m-mers: with canonical m-mers the function is one of the KEY.
__device__ __forceinline__ unsigned bucket_of_le(u64 le, const KmerBulk &p)
{
    unsigned best = ~0u;
    for (int j = 0; j < p.w; ++j) {
        const unsigned hv = mmer_hash(mmer_canonical((unsigned)low_bases(le >> (2 * j), p.m), p.m, p.canonical));
        best = hv < best ? hv : best;
    }
    return bucket_of_min(best, p.log2_buckets);
}

// One record behind its bucket's cursor.  ctl[b] = {first, end}: places in recs; fill[b]: the cursor.
__device__ __forceinline__ void store_record(unsigned b, u64 code, int n_bases, const KmerBulk &p)
{
    // (the cursors are an array of their own, touched by atomics only: atomics on lines that plain loads of the same
    // kernel keep in the caches run at a tenth of the rate -- measured, DESIGN.md 6b.  Also measured: {cursor, end} in
    // one element with the end read by an agent-scope atomic load -- one line a record instead of two -- is SLOWER,
    // 137-141 against 102-103 ms at 10 Gbp)
    const ulonglong2 place = p.ctl[b];
    const u64 pos = place.x + (u64)atomicAdd(&p.fill[b], (KmerBulk::fill_t)1);
    ulonglong2 *to = p.recs + pos;
    if (pos >= place.y) { // the bucket is full: the record goes to the list, and the WHOLE bucket to the table later (pass 2)
        const unsigned shard = blockIdx.x % kOvfShards;
        const u64 at = atomicAdd(&p.ovf_count[shard * kOvfStride], 1ull);
        to = at < p.overflow_cap ? p.overflow + shard * p.overflow_cap + at : nullptr;
    }
    // (ONE store site: with a store in either branch the compiler writes a record as two 8-byte halves, the second
    // after the branches meet -- pass 1 at 10 Gbp 95 -> 108 ms, profiles/kmer_stages_ab.txt)
    if (to)
        *to = make_ulonglong2(code, (u64)n_bases);
}

// ---- pass 0 / 1, the tiles ---------------------------------------------------------------------------------------
// The read array as one run of bytes (`len` bytes a read, nothing between them): tile t covers bytes
// [t * n_win, t * n_win + 256), its first n_win = kmer_plan::tile_windows(w) bytes are the window starts it answers for.
// `positions`: bytes of this launch (whole reads, < 2^32); `avail`: bytes that may be read from `bases` on.
// RAGGED: the reads are of different lengths -- offsets[r] .. offsets[r + 1] of the byte run are read r -- and a thread
// has to learn which read its byte belongs to: the tile's first read comes from a table made beforehand
// (kmer_tile_first_read_kernel), the starts of the up to 32 reads behind it are brought into LDS, and the thread
// searches those (a tile of shorter reads than that: the thread searches the offsets themselves).  `positions` and
// the tiles then count from byte `pos0` of the run, which need not be a read's start.
struct RaggedReads {
    const int64_t *offsets; // [n_reads + 1], absolute in the caller's byte run
    int64_t n_reads;
    int64_t base0;          // offsets[0]
    int64_t pos0;           // this launch's first byte, relative to base0
    const unsigned *first_read; // [tiles of this launch] read of the tile's first byte
};
constexpr int kTileReads = 32;

// largest r in [lo, n_reads) with offsets[r] - base0 <= pos (reads of no bases share their start with the next one)
__device__ __forceinline__ int64_t read_of(const int64_t *__restrict__ offsets, int64_t n_reads, int64_t base0, int64_t pos,
                                           int64_t lo)
{
    int64_t hi = n_reads; // offsets[hi] - base0 > pos (or hi == n_reads)
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] - base0 <= pos)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void kmer_tile_first_read_kernel(RaggedReads src, unsigned n_tiles, int n_win,
                                                                   unsigned *__restrict__ first_read)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_tiles)
        first_read[t] = (unsigned)read_of(src.offsets, src.n_reads, src.base0, src.pos0 + (int64_t)t * n_win, 0);
}

// Load: the 16 bases from byte `at` on, one unaligned 16-byte load (what lies beyond `avail` reads as 'a')
__device__ __forceinline__ unsigned load_bases16(const unsigned char *__restrict__ bases, unsigned at, u64 avail)
{
    if ((u64)at + 16ull <= avail) {
        uint4 v;
        __builtin_memcpy(&v, bases + at, 16);
        return pack4(v.x) | (pack4(v.y) << 8) | (pack4(v.z) << 16) | (pack4(v.w) << 24);
    }
    unsigned c16 = 0;
    for (int j = 0; j < 16; ++j)
        if ((u64)at + (u64)j < avail)
            c16 |= base_code(bases[at + j]) << (2 * j);
    return c16;
}

// Classify: what a thread learns of its byte
struct ByteClass {
    bool mmer;   // the m-mer that starts here lies within the byte's read (the halo's bytes belong to reads too)
    bool window; // the byte starts a window of this tile and launch
};

// Reads of one length: the byte's place in its read decides.
__device__ __forceinline__ ByteClass classify_fixed(unsigned at, int tid, int n_win, unsigned positions, unsigned len,
                                                    const KmerBulk &p)
{
    const unsigned i = at % len;
    const bool live = at < positions;
    return {live && i + (unsigned)p.m <= len, live && tid < n_win && i + (unsigned)p.k <= len};
}

// Reads of any length: the byte's read is the last of the tile's reads that starts at or before it.  roff: LDS,
// kTileReads + 2 words -- the starts of the tile's first reads (and the end of the last of them), relative to pos0.
// The whole workgroup calls this.
__device__ __forceinline__ ByteClass classify_ragged(unsigned at, unsigned tile, int tid, int n_win, unsigned positions,
                                                     u64 avail, const KmerBulk &p, const RaggedReads &src, int64_t *roff)
{
    const int64_t r0 = (int64_t)src.first_read[tile];
    if (tid <= kTileReads) {
        const int64_t r = r0 + tid < src.n_reads ? r0 + tid : src.n_reads;
        roff[tid] = src.offsets[r] - src.base0 - src.pos0;
    }
    __syncthreads();
    const int64_t here = (int64_t)at;
    int j = 0;
    for (int step = kTileReads / 2; step >= 1; step >>= 1)
        if (roff[j + step] <= here)
            j += step;
    int64_t start = roff[j], end = roff[j + 1];
    if (j == kTileReads - 1 && end <= here && r0 + kTileReads < src.n_reads) { // more reads than the table holds
        const int64_t r = read_of(src.offsets, src.n_reads, src.base0, src.pos0 + here, r0 + kTileReads - 1);
        start = src.offsets[r] - src.base0 - src.pos0;
        end = src.offsets[r + 1] - src.base0 - src.pos0;
    }
    // (the halo's bytes belong to reads too: only the WINDOWS are this launch's or not)
    const bool in_run = (u64)at < avail && here < end;
    return {in_run && here + p.m <= end, in_run && at < positions && tid < n_win && here + p.k <= end && here >= start};
}

// Bucket: of the window that starts at thread `tid`, from the hashes of the m-mers that start at the tile's bytes
__device__ __forceinline__ unsigned window_bucket(const unsigned *hs, int tid, const KmerBulk &p)
{
    unsigned mn = hs[tid];
    for (int j = 1; j < p.w; ++j) {
        const unsigned o = hs[tid + j];
        mn = o < mn ? o : mn;
    }
    return bucket_of_min(mn, p.log2_buckets);
}

// Emit: the n_bases <= 32 bases from thread `a` on as a record's code.  cs: every thread's 16 bases.
__device__ __forceinline__ u64 piece(const unsigned *cs, int a, int n_bases)
{
    return low_bases((u64)cs[a] | ((u64)cs[a + 16] << 32), n_bases);
}

template <bool COUNT, bool RAGGED>
__global__ __launch_bounds__(kTile) void kmer_tile_kernel(const unsigned char *__restrict__ bases, unsigned positions,
                                                          u64 avail, unsigned len, unsigned n_tiles, const KmerBulk p,
                                                          const RaggedReads src)
{
    __shared__ int64_t roff[RAGGED ? kTileReads + 2 : 1];
    __shared__ unsigned hs[kTile]; // hash of the m-mer that starts at the byte
    __shared__ unsigned cs[kTile]; // the 16 bases from the byte on
    __shared__ unsigned bk[kTile]; // bucket of the window that starts at the byte
    __shared__ u64 hmask[kRunWaves], vmask[kRunWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int n_win = kmer_plan::tile_windows(p.w);
    const unsigned block = COUNT ? blockIdx.x * (unsigned)p.sample : blockIdx.x;
    for (int tt = 0; tt < kTilesPerBlock; ++tt) {
        const unsigned tile = block * kTilesPerBlock + tt;
        if (tile >= n_tiles)
            break; // (workgroup-uniform)
        const unsigned at = tile * (unsigned)n_win + (unsigned)tid;
        const unsigned c16 = load_bases16(bases, at, avail);
        const ByteClass is = RAGGED ? classify_ragged(at, tile, tid, n_win, positions, avail, p, src, roff)
                                    : classify_fixed(at, tid, n_win, positions, len, p);
        hs[tid] = is.mmer ? mmer_hash(mmer_canonical((unsigned)low_bases(c16, p.m), p.m, p.canonical)) : ~0u;
        cs[tid] = c16;
        __syncthreads();
        const unsigned b = is.window ? window_bucket(hs, tid, p) : kNoBucket;
        bk[tid] = b;
        __syncthreads();
        // a run starts where the window before is none (a read begins, the tile does) or belongs elsewhere
        const bool head = is.window && (tid == 0 || bk[tid - 1] != b);
        const u64 heads = __ballot(head), valid = __ballot(is.window);
        if (lane == 0) {
            hmask[wave] = heads;
            vmask[wave] = valid;
        }
        __syncthreads();
        if (head) {
            const int run = run_length(lane, wave, heads, valid, hmask, vmask);
            if (COUNT)
                atomicAdd(&p.sampled[b], (unsigned)pieces_of(run, p.max_run));
            else
                for_each_piece(run, p.max_run, p.k, [&](int first, int n_bases) {
                    store_record(b, piece(cs, tid + first, n_bases), n_bases, p);
                });
        }
        __syncthreads(); // (the arrays are the next tile's)
    }
}

// ---- pass 0 / 1, the reads SHORTER than k (reads of any length only) ----------------------------------------------
// hash_kmer of what there is (bin/kmer_hist.py:36-37): an integer below 4^len -- the very key of the k-mer
// "a" * (k - len) + read, which a window elsewhere may spell out (a read of k - 1 bases behind an 'a' in the genome:
// one in four).  So it is counted AS that k-mer, through its bucket: a key must live in one place.  A thread a read.
template <bool COUNT>
__global__ __launch_bounds__(256) void kmer_short_reads_kernel(const unsigned char *__restrict__ bases,
                                                               const int64_t *__restrict__ offsets, int64_t n_reads,
                                                               const KmerBulk p)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (COUNT)
        r *= p.sample;
    if (r >= n_reads)
        return;
    const int64_t p0 = offsets[r];
    const int len = (int)min(offsets[r + 1] - p0, (int64_t)p.k);
    if (len >= p.k)
        return;
    u64 le = 0;
    for (int i = 0; i < len; ++i)
        le |= (u64)base_code(bases[p0 + i]) << (2 * (p.k - len + i));
    const unsigned b = bucket_of_le(le, p);
    if (COUNT)
        atomicAdd(&p.sampled[b], 1u);
    else
        store_record(b, le, p.k, p);
}

} // namespace

} // namespace covest
