// kmer_table.h -- the open-addressing k-mer table of K-kmer (k <= 31) as device functions: shared by
// kmer_count.hip (every occurrence goes to the table), kmer_bulk.hip (only what its LDS path hands back does), and
// kmer_lookup.hip, kmer_correct.hip and kmer_influence.hip (which only read it: table_find; a wave a read: wave_read.h),
// kmer_join.hip (which reads two: every key of one table looked up in the other), and kmer_remove.hip (which lowers
// counts and never clears a key: "held" and "occupied" below).  The walk over the reads that kmer_count.hip and
// kmer_remove.hip share, with table_add or table_locate and a returning atomic as its operation: kmer_update.h.
// See kmer_count.hip for the reference it restates and for why a key's first slot is a function of its minimizer.
// The arithmetic on the codes themselves: kmer_codes.h.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kmer_codes.h"
#include "wave.h"

namespace covest {
namespace kmer {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kMaxProbe = 1 << 16;

// canonical keys: the smaller of a code and its reverse complement's comes first
__device__ __forceinline__ void canonical_pair(unsigned long long &h, unsigned long long &rc, int canonical)
{
    if (canonical && rc < h) {
        const unsigned long long x = h;
        h = rc;
        rc = x;
    }
}

// workgroups of 256 threads for n items, `cap` at most (the kernels stride over the rest)
inline unsigned grid_for(unsigned long long n, unsigned cap = 256 * 16)
{
    const unsigned long long blocks = (n + 255) / 256;
    return (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
}

__device__ __forceinline__ unsigned long long slot_of(unsigned long long key, int log2_slots)
{
    return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots); // Fibonacci hashing
}

// A key's FIRST slot: [ line | slot in the line ], a line being 8 slots = 128 bytes.
//   line  a hash of the key's MINIMIZER -- the canonical m-mer of smallest hash among its k - m + 1 = 8 windows
//         (m = k - 7).  Neighbouring windows of a read mostly share their minimizer, so the 64 k-mers a wave inserts
//         at a time fall into a dozen lines instead of 64 unrelated ones;
//   slot  the POSITION of the minimizer inside the key (plus a rotation taken from its hash): the k-mers of one run
//         -- same minimizer, positions 7, 6, 5, ... as the window moves on -- get slots of their own by construction.
// Why: what bounds this kernel is the rate at which the memory side retires scattered 8-byte operations, about 2e10
// load+add pairs a second whatever the table's size (tools/microbench_atomics.hip), and requests of one wave
// instruction that fall into one 128-byte line are retired together (3.8x the rate with 8 lanes per line).
// A key that finds its first slot taken by ANOTHER key does not probe on from there -- the k-mers that differ from
// a genomic one by a substitution mostly share its minimizer and its position, and would walk through the run's
// occupied slots -- but goes to the plain hash of the key and probes linearly from there (table_add).  Slots never
// change their key, so every occurrence of a key takes the same decisions: exact counts.  `rc`: the reverse
// complement of `key` as a 2k-bit code (the function is symmetric in the two up to the mirrored position).
constexpr int kLineLog2 = 3;
constexpr int kLineSlots = 1 << kLineLog2;

__device__ __forceinline__ bool has_first_slot(const KmerTable &t)
{
    return t.k - (kLineSlots - 1) >= 6 && t.log2_slots > kLineLog2 + 4;
}

__device__ __forceinline__ unsigned long long first_slot(unsigned long long key, unsigned long long rc, const KmerTable &t)
{
    const int m = t.k - (kLineSlots - 1);
    const unsigned long long mm = (1ull << (2 * m)) - 1ull;
    unsigned long long best = ~0ull;
    int at = 0;
#pragma unroll
    for (int i = 0; i < kLineSlots; ++i) {
        const unsigned long long a = (key >> (2 * i)) & mm;                    // m-mer i of the key ...
        const unsigned long long b = (rc >> (2 * (kLineSlots - 1 - i))) & mm;  // ... and its reverse complement
        const unsigned long long c = a < b ? a : b;
        const unsigned long long x = (c + 1ull) * 0x9E3779B97F4A7C15ull;
        if (x < best) {
            best = x;
            at = i;
        }
    }
    const unsigned long long h2 = best * 0xD6E8FEB86659FD93ull; // (the minimum of 8 hashes is small: spread it again)
    const unsigned long long line = h2 >> (64 - (t.log2_slots - kLineLog2));
    return (line << kLineLog2) | (unsigned long long)((at + (int)(h2 & 7ull)) & (kLineSlots - 1));
}

// true: the key was counted in slot h (found there, or put there)
__device__ __forceinline__ bool try_slot(const KmerTable &t, unsigned long long h, unsigned long long key,
                                         unsigned long long add)
{
    KmerSlot *slot = t.slots + h;
    unsigned long long cur = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmptyKey)
        cur = atomicCAS(&slot->key, kEmptyKey, key); // returns the previous value
    if (cur == kEmptyKey || cur == key) {
        atomicAdd(&slot->count, add);
        return true;
    }
    return false;
}

__device__ __forceinline__ void table_add(const KmerTable t, unsigned long long key, unsigned long long rc,
                                          unsigned long long add, int *overflow)
{
    if (has_first_slot(t) && try_slot(t, first_slot(key, rc, t), key, add))
        return; // (a second try in the same line before leaving it was measured: no change)
    unsigned long long h = slot_of(key, t.log2_slots);
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        if (try_slot(t, h, key, add))
            return;
        h = (h + 1) & t.mask;
    }
    *overflow = 1;
}

// A slot as ONE 16-byte load of {key, count} (x = key, y = count): a plain load -- the kernels that look counts up run
// after the kernels that added them, so no atomic and no agent-scope load is needed (kmer_lookup.hip).
__device__ __forceinline__ ulonglong2 slot_load(const KmerTable &t, unsigned long long h)
{
    static_assert(sizeof(KmerSlot) == sizeof(ulonglong2), "a slot is one 16-byte load");
    return *reinterpret_cast<const ulonglong2 *>(t.slots + h);
}

// ---- held and occupied ------------------------------------------------------------------------
// A slot is OCCUPIED if it carries a key at all; a key is HELD if its slot carries it with a count of at least 1.  On a
// table that was only added to the two coincide.  A removal (kmer_remove.hip) lowers a count and never clears a key: a
// count may reach 0 while the key stays where every probe chain expects it, so table_add and table_find keep replaying
// the same decisions, also past keys whose count is 0.  Every scan of this table -- the stats, the histogram, the join,
// the rehash -- speaks of held keys through slot_held; the stats also count the occupied slots, which is what bounds
// how full the table is.
__device__ __forceinline__ bool slot_occupied(unsigned long long key)
{
    return key != kEmptyKey;
}

__device__ __forceinline__ bool slot_held(unsigned long long key, unsigned long long count)
{
    return slot_occupied(key) && count != 0ull;
}

// The slot that carries `key` (kNoSlot: none does) and, in `count`, the count loaded with it, without a store.  It
// replays table_add's decisions: the first slot carries the key, is empty (the key would have been put there: none) or
// carries another key; then from the plain hash on, a slot with the key is the one and an empty one ends the walk;
// after kMaxProbe probes none -- the add would have overflowed.  Slots never change their key and no key is ever
// cleared, so every slot an add of `key` passed over still carries the key it carried then: exact for every key, also
// after a rehash (it inserts by table_add) and past keys whose count a removal has brought to 0.
constexpr unsigned long long kNoSlot = ~0ull;
__device__ __forceinline__ unsigned long long table_locate(const KmerTable &t, unsigned long long key, unsigned long long rc,
                                                           unsigned long long &count)
{
    if (has_first_slot(t)) {
        const unsigned long long h = first_slot(key, rc, t);
        const ulonglong2 e = slot_load(t, h);
        if (e.x == key) {
            count = e.y;
            return h;
        }
        if (e.x == kEmptyKey)
            return kNoSlot;
    }
    unsigned long long h = slot_of(key, t.log2_slots);
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        const ulonglong2 e = slot_load(t, h);
        if (e.x == key) {
            count = e.y;
            return h;
        }
        if (e.x == kEmptyKey)
            return kNoSlot;
        h = (h + 1) & t.mask;
    }
    return kNoSlot;
}

// The count the table holds for `key` (0: it holds none -- no slot carries it, or one does with a count of 0), without
// a store: table_locate's walk, written out.  (Built over table_locate the readers' kernels -- kmer_lookup.hip,
// kmer_correct.hip, kmer_influence.hip -- came out as other code; the two walks stand side by side instead, and
// tests/test_gpu_remove.py holds them to the same answers.)
__device__ __forceinline__ unsigned long long table_find(const KmerTable &t, unsigned long long key, unsigned long long rc)
{
    if (has_first_slot(t)) {
        const ulonglong2 e = slot_load(t, first_slot(key, rc, t));
        if (e.x == key)
            return e.y;
        if (e.x == kEmptyKey)
            return 0ull;
    }
    unsigned long long h = slot_of(key, t.log2_slots);
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        const ulonglong2 e = slot_load(t, h);
        if (e.x == key)
            return e.y;
        if (e.x == kEmptyKey)
            return 0ull;
        h = (h + 1) & t.mask;
    }
    return 0ull;
}

// from the little-endian code of a window (base i at bits 2i, masked to 2k bits): the window's own code (mirrored:
// first base in the highest bits) and its reverse complement's
__device__ __forceinline__ void codes_from_le(unsigned long long le, int k, unsigned long long &h, unsigned long long &rc)
{
    rc = ~le & kmer_mask(k);
    h = reverse_pairs64(le) >> (64 - 2 * k);
}

// The window starting at seq[s] of a read of `len` bases as 2-bit codes, little-endian (base i of the window at bits
// 2i) -- that IS the reverse complement's code once complemented -- and mirrored (first base in the highest bits:
// hash_kmer, bin/kmer_hist.py:18-23).  Four bases per (unaligned) 32-bit load where the read has them.
__device__ __forceinline__ void window_codes(const unsigned char *__restrict__ seq, int64_t s, int64_t len, int k,
                                             unsigned long long &h, unsigned long long &rc)
{
    const int n_words = (k + 3) >> 2; // 32-bit words of 4 bases that cover a window
    if (s + 4 * n_words <= len) {
        unsigned long long le = 0;
        for (int j = 0; j < n_words; ++j) {
            unsigned w;
            __builtin_memcpy(&w, seq + s + 4 * j, 4);
            le |= (unsigned long long)pack4(w) << (8 * j);
        }
        codes_from_le(low_bases(le, k), k, h, rc);
    } else { // the last windows of a read: byte by byte (a word would reach past the read's end)
        h = 0;
        rc = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned long long c = base_code(seq[s + i]);
            h = (h << 2) | c;                  // hash_kmer, :18-23 (rehash :26-31 yields the same window code)
            rc |= (3ull - c) << (2 * i);       // reverse complement, built back to front
        }
    }
}

// {distinct keys, largest count} of a wave's lanes, in every lane (the stats kernels of both tables and pass 2 of
// kmer_bulk.hip end with it)
__device__ __forceinline__ void wave_fold_distinct_max(unsigned long long &distinct, unsigned long long &mx)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        distinct += __shfl_xor(distinct, off, kWave);
        const unsigned long long o = __shfl_xor(mx, off, kWave);
        mx = o > mx ? o : mx;
    }
}

} // namespace kmer
} // namespace covest
