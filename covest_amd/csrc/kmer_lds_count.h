// kmer_lds_count.h -- pass 2 of the partitioned k-mer counter (kmer_bulk.hip includes this once): a bucket's records
// counted in a hash table in LDS -- a wave's own (kmer_wave_count_kernel) or, for the few buckets too large for that, a
// workgroup's (kmer_bucket_count_kernel) --, the table swept into count-of-counts bins and cleared for the next bucket.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kmer_table.h"
#include "wave.h"

namespace covest {

namespace {

using namespace kmer;
typedef unsigned long long u64;

constexpr int kWaveSlots = 1024;     // LDS hash table of a wave: 8 KB of keys + 4 KB of counts (or half of it, see the launch)
constexpr int kWaveRecs = 768;       // a bucket with more records than this goes to a workgroup instead
constexpr int kLdsSlots = 4096;      // LDS hash table of a workgroup: 32 KB of keys + 16 KB of counts
constexpr int kLdsHistBins = 1024;   // count-of-counts bins kept in LDS per workgroup
constexpr u64 kLdsEmpty = ~0ull;

// ---- the table -----------------------------------------------------------------------------------------------------
// slots [first, first + stride, ...) of a table emptied, and the workgroup's bins zeroed: before the first bucket
__device__ __forceinline__ void clear_table(u64 *keys, unsigned *cnts, int slots, int first, int stride)
{
    for (int i = first; i < slots; i += stride) {
        keys[i] = kLdsEmpty;
        cnts[i] = 0u;
    }
}

__device__ __forceinline__ void clear_bins(unsigned *bins)
{
    for (int i = threadIdx.x; i < kLdsHistBins; i += blockDim.x)
        bins[i] = 0u;
}

// slots a bucket of n records gets: eight a record, a power of two from lo to hi
__device__ __forceinline__ unsigned slots_for(u64 n, unsigned lo, unsigned hi)
{
    unsigned slots = lo;
    while ((u64)slots < 8ull * n && slots < hi)
        slots <<= 1;
    return slots;
}

// The key a k-mer is counted under in the LDS tables: any one-to-one function of the reference's key does -- the
// smaller of the window's little-endian code and its reverse complement's.  The reverse complement of the RECORD once,
// its windows are then shifts of it.
__device__ __forceinline__ u64 record_revcomp(ulonglong2 rec)
{
    return rec.y == 0 ? 0ull : reverse_pairs64(~rec.x) >> (64 - 2 * (int)rec.y);
}

// the key of the record's next window: `f` the record's code from that window on, `left` windows to go with it --
// window j of the record is window n_k - 1 - j of its reverse complement `rc`
__device__ __forceinline__ u64 window_key(u64 f, u64 rc, int left, u64 kmask, int canonical)
{
    u64 key = f & kmask;
    if (canonical) {
        const u64 r = (rc >> (2 * max(left - 1, 0))) & kmask;
        key = r < key ? r : key;
    }
    return key;
}

// Every k-mer of the lane's record (none: rec.y == 0) into the table, false: the table is full.  The lanes of a wave
// go through their records side by side but each at its own pace -- ONE flat loop, a probe per turn: a lane whose probe
// hit counts and moves on to its next k-mer while its neighbours still probe (nested loops -- k-mers outside, probes
// inside -- cost three scalar instructions of mask bookkeeping per vector instruction).  (Measured and not kept, round 5:
// TWO windows of a record per turn, the even and the odd ones with a probe state each, so that a wave has two
// compare-and-swaps in flight -- pass 2 43.8 -> 55.2 ms at 10 Gbp, profiles/r05_c5_ab_two_windows_per_turn_not_kept.txt:
// the LDS applies a wave's atomics one after the other either way, and the second state costs registers and selects.)
__device__ __forceinline__ bool insert_record(ulonglong2 rec, u64 *keys, unsigned *cnts, unsigned slots, u64 kmask,
                                              const KmerBulk &p)
{
    const unsigned smask = slots - 1u;
    int left = rec.y ? (int)rec.y - p.k + 1 : 0; // k-mers to go (< 0: gave up)
    const u64 rc = p.canonical ? record_revcomp(rec) : 0ull;
    u64 f = rec.x;
    u64 key = window_key(f, rc, left, kmask, p.canonical);
    unsigned at = lds_slot(key, smask), probes = 0;
    while (__ballot(left > 0) != 0ull) {
        if (left > 0) {
            // (no look before the compare-and-swap: one LDS round trip a probe instead of two -- measured, 10 % of pass 2)
            const u64 cur = atomicCAS(&keys[at], kLdsEmpty, key);
            if (cur == kLdsEmpty || cur == key) {
                atomicAdd(&cnts[at], 1u);
                f >>= 2;
                --left;
                key = window_key(f, rc, left, kmask, p.canonical);
                at = lds_slot(key, smask);
                probes = 0;
            } else {
                at = (at + 1u) & smask;
                if (++probes >= slots) // every slot holds another key
                    left = -1;
            }
        }
    }
    return left == 0;
}

// (Measured and not kept, round 3: two records a lane with both probe sequences in flight per turn and no branch inside
// it -- lanes without a k-mer left swap "empty" for "empty" -- 65 against 44 ms at 10 Gbp: the idle lanes' swaps and
// the adds of 0 are LDS traffic too, and that, not the round trip alone, is what the kernel waits for.)

// ---- from the table to the histogram -------------------------------------------------------------------------------
// stats: [0] max count, [1] distinct keys, [2] entries of `big` (counts >= hist_len), [3] records pass 1 sent (to the
// buckets and to the overflow list).  hist: dense count-of-counts for counts < hist_len; bins: its first kLdsHistBins
// entries for this workgroup, in LDS, flushed once at the end.
struct CountOut {
    unsigned *bins;
    u64 *__restrict__ hist;
    u64 hist_len;
    u64 *__restrict__ stats;
    u64 *__restrict__ big;
    u64 big_cap;
};

struct SweepAcc {
    u64 distinct = 0, mx = 0;
};

// one slot's count into the bins
__device__ __forceinline__ void count_into_bins(u64 c, SweepAcc &acc, const CountOut &out)
{
    ++acc.distinct;
    acc.mx = c > acc.mx ? c : acc.mx;
    if (c < (u64)kLdsHistBins) {
        atomicAdd(&out.bins[c], 1u);
    } else if (c < out.hist_len) {
        atomicAdd(&out.hist[c], 1ull);
    } else {
        const u64 at = atomicAdd(&out.stats[2], 1ull);
        if (at < out.big_cap)
            out.big[at] = c;
    }
}

// The keys of slots [first, first + stride, ...) into the bins (counted: unless the bucket goes elsewhere as a whole),
// and the slots emptied: the table is the next bucket's.
__device__ __forceinline__ void sweep_and_clear(u64 *keys, unsigned *cnts, unsigned slots, unsigned first, unsigned stride,
                                                bool counted, SweepAcc &acc, const CountOut &out)
{
    for (unsigned i = first; i < slots; i += stride)
        if (keys[i] != kLdsEmpty) {
            const u64 cnt = cnts[i];
            keys[i] = kLdsEmpty;
            cnts[i] = 0u;
            if (counted)
                count_into_bins(cnt, acc, out);
        }
}

__device__ __forceinline__ void flush_stats(SweepAcc acc, const CountOut &out)
{
    for (int i = threadIdx.x; i < kLdsHistBins; i += blockDim.x)
        if (out.bins[i] != 0u && (u64)i < out.hist_len)
            atomicAdd(&out.hist[i], (u64)out.bins[i]);
    wave_fold_distinct_max(acc.distinct, acc.mx);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMax(&out.stats[0], acc.mx);
        atomicAdd(&out.stats[1], acc.distinct);
    }
}

// ---- a wave per bucket ---------------------------------------------------------------------------------------------
// The look-ahead: which bucket the wave counts after this one is known a bucket early, so that its first 64 records
// are on their way while this bucket's last ones are counted.
struct NextBucket {
    u64 start;  // place of its first record
    unsigned n; // its records (0: there is no next bucket)
    int lane;   // the lane that holds its cursors
};

// the first bucket of `todo` (not 0; a bit a lane); first / filled: the lanes' buckets' first places and records
__device__ __forceinline__ NextBucket next_bucket(u64 todo, u64 first, u64 filled)
{
    NextBucket nb;
    nb.lane = __ffsll((long long)todo) - 1;
    nb.start = __shfl(first, nb.lane, kWave);
    nb.n = (unsigned)__shfl((unsigned)filled, nb.lane, kWave);
    return nb;
}

// later[0]: buckets left to kmer_bucket_count_kernel, listed in later_list.
template <int SLOTS>
__global__ __launch_bounds__(256) void kmer_wave_count_kernel(const KmerBulk p, u64 *__restrict__ hist, u64 hist_len,
                                                              u64 *__restrict__ stats, u64 *__restrict__ big, u64 big_cap,
                                                              unsigned *__restrict__ later, unsigned *__restrict__ later_list)
{
    __shared__ u64 all_keys[256 / kWave][SLOTS];
    __shared__ unsigned all_cnts[256 / kWave][SLOTS];
    __shared__ unsigned bins[kLdsHistBins];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    u64 *keys = all_keys[wave];
    unsigned *cnts = all_cnts[wave];
    const CountOut out{bins, hist, hist_len, stats, big, big_cap};
    clear_bins(bins);
    clear_table(keys, cnts, SLOTS, lane, kWave);
    __syncthreads();
    SweepAcc acc;
    u64 n_records = 0;
    const unsigned n_groups = (1u << p.log2_buckets) / kWave; // (at least 2^10 buckets)
    const unsigned n_waves = gridDim.x * (blockDim.x / kWave);
    const u64 kmask = kmer_mask(p.k);
    for (unsigned g = blockIdx.x * (blockDim.x / kWave) + wave; g < n_groups; g += n_waves) {
        // 64 buckets' cursors at once, a lane each
        const unsigned b_lane = g * kWave + lane;
        const ulonglong2 c = p.ctl[b_lane];
        const u64 first = c.x, filled = p.fill[b_lane], room = c.y - c.x;
        n_records += filled;
        const bool skip = filled > room || filled > (u64)(kWaveRecs * SLOTS / kWaveSlots);
        const u64 skipmask = __ballot(skip);
        if (skipmask) {
            unsigned at = 0;
            if (lane == 0)
                at = atomicAdd(later, (unsigned)__popcll(skipmask));
            at = __builtin_amdgcn_readfirstlane(at);
            if (skip)
                later_list[at + __popcll(skipmask & ((1ull << lane) - 1ull))] = b_lane;
        }
        u64 todo = __ballot(!skip && filled > 0);
        NextBucket next{0ull, 0u, 0};
        ulonglong2 rec = make_ulonglong2(0ull, 0ull);
        if (todo) {
            next = next_bucket(todo, first, filled);
            if ((unsigned)lane < next.n)
                rec = p.recs[next.start + lane];
        }
        while (todo) {
            const NextBucket cur = next;
            todo &= todo - 1ull;
            next.n = 0;
            if (todo)
                next = next_bucket(todo, first, filled);
            const unsigned slots = slots_for(cur.n, 64, SLOTS);
            bool ok = true;
            for (unsigned i0 = 0; i0 < cur.n; i0 += kWave) {
                // the records after these -- the bucket's next 64, or the first of the next bucket -- are on their way
                // while these are counted
                const bool last = i0 + kWave >= cur.n;
                const u64 from = last ? next.start : cur.start + i0 + kWave;
                const unsigned have = last ? next.n : cur.n - (i0 + kWave);
                ulonglong2 rec_next = make_ulonglong2(0ull, 0ull);
                if ((unsigned)lane < have)
                    rec_next = p.recs[from + lane];
                ok = insert_record(rec, keys, cnts, slots, kmask, p) && ok;
                rec = rec_next;
            }
            const bool failed = __ballot(!ok) != 0ull; // more distinct keys than slots: a workgroup takes the bucket
            sweep_and_clear(keys, cnts, slots, lane, kWave, !failed, acc, out);
            if (failed && lane == 0)
                later_list[atomicAdd(later, 1u)] = g * kWave + (unsigned)cur.lane;
        }
    }
    __syncthreads();
    flush_stats(acc, out);
    for (int off = 32; off >= 1; off >>= 1)
        n_records += __shfl_xor(n_records, off, kWave);
    if (lane == 0 && n_records)
        atomicAdd(&stats[3], n_records);
}

// ---- a workgroup per bucket: those of later_list ------------------------------------------------------------------
// What does not fit here either is listed for the table in HBM (to_table[0] buckets, to_table[1] their k-mer
// occurrences -- the table is sized AFTER this is known --, to_table_list).
__global__ __launch_bounds__(256) void kmer_bucket_count_kernel(const KmerBulk p, u64 *__restrict__ hist, u64 hist_len,
                                                                u64 *__restrict__ stats, u64 *__restrict__ big, u64 big_cap,
                                                                const unsigned *__restrict__ later,
                                                                const unsigned *__restrict__ later_list,
                                                                u64 *__restrict__ to_table, unsigned *__restrict__ to_table_list)
{
    __shared__ u64 keys[kLdsSlots];
    __shared__ unsigned cnts[kLdsSlots];
    __shared__ unsigned bins[kLdsHistBins];
    const int tid = threadIdx.x;
    const CountOut out{bins, hist, hist_len, stats, big, big_cap};
    clear_bins(bins);
    clear_table(keys, cnts, kLdsSlots, tid, blockDim.x);
    __syncthreads();
    SweepAcc acc;
    const unsigned n_later = later[0];
    const u64 kmask = kmer_mask(p.k);
    for (unsigned at = blockIdx.x; at < n_later; at += gridDim.x) {
        const unsigned b = later_list[at];
        const ulonglong2 c = p.ctl[b];
        const u64 first = c.x, filled = p.fill[b], room = c.y - c.x;
        const u64 n = filled < room ? filled : room;
        const ulonglong2 *recs = p.recs + first;
        // records of this bucket in the overflow list too, or more distinct keys than the table holds: to the table
        // ... or so many records that one key's count could pass the 32 bits of the LDS counters (a low-complexity input
        // with 2^32 windows and more in one bucket): the table's counters are 64-bit
        bool fall_back = filled > room || filled * (u64)p.max_run >= (1ull << 32);
        u64 n_kmers = 0;
        if (!fall_back) {
            const unsigned slots = slots_for(n, 1024, kLdsSlots);
            bool ok = true;
            for (u64 i = tid; i < n; i += blockDim.x) {
                const ulonglong2 rec = recs[i];
                const int n_k = (int)rec.y - p.k + 1;
                n_kmers += (u64)n_k;
                ok = insert_record(rec, keys, cnts, slots, kmask, p) && ok;
            }
            fall_back = __syncthreads_or(!ok) != 0;
            sweep_and_clear(keys, cnts, slots, tid, blockDim.x, !fall_back, acc, out);
            __syncthreads();
        }
        if (fall_back) {
            if (n_kmers == 0) // (not read yet)
                for (u64 i = tid; i < n; i += blockDim.x)
                    n_kmers += (u64)((int)recs[i].y - p.k + 1);
            for (int off = 32; off >= 1; off >>= 1)
                n_kmers += __shfl_xor(n_kmers, off, kWave);
            if ((tid & (kWave - 1)) == 0)
                atomicAdd(&to_table[1], n_kmers);
            if (tid == 0)
                to_table_list[atomicAdd(&to_table[0], 1ull)] = b;
        }
    }
    __syncthreads();
    flush_stats(acc, out);
}

} // namespace

} // namespace covest
