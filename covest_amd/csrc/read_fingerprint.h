// read_fingerprint.h -- the fingerprint of a whole read, and the size of the table keyed by it: what the duplicate
// remover (dedup_reads.hip, covest_dedup_reads*) decides candidates by, in plain C++.  No HIP in
// it: tests/read_fingerprint_check.cpp runs it under the host compiler's sanitizers, tests/dedup_reference.py restates it.
//
//   mix64(z)    the finaliser of SplitMix64 (Steele, Lea, Flood 2014; Stafford's "Mix13"), a bijection of 64-bit words:
//                   z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
//   salt(seed)  mix64(seed + 0x9E3779B97F4A7C15)
//   S(x)        the sum mod 2^64 over the positions j of mix64(salt + 256 * j + x[j]): (j, byte) -> 256 * j + byte is
//               one to one, and a SUM gives the same bits in whatever order lanes and waves add their shares
//   F(x)        mix64(mix64(S(x) + seed) + len(x))
// Forward only the fingerprint of a read is F(x); with the reverse complement it is min(F(x), F(rc(x))), both sums
// formed in one pass over the bases: base j of x is base len - 1 - j of rc(x), complemented (a <-> t, c <-> g in either
// case, the case kept; every other byte is its own complement).
// The KEY is the fingerprint's low fp_bits bits, fp_bits in 1 .. 63, so bit 63 of a key is never set and the table's
// empty sentinel, ~0 (what a byte-wise memset of 0xff leaves), is no possible key.  fp_bits below 63 only makes more
// reads collide: it exists so that the collision route can be tested exactly, and has no other use.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define FP_HD __host__ __device__
#else
#define FP_HD
#endif

namespace covest {
namespace fingerprint {

constexpr uint64_t kEmptyKey = ~0ull;        // of a slot's key; as a slot's value: no read yet (above every index)
constexpr int kDefaultBits = 63;
constexpr int kMinLog2Slots = 10, kMaxLog2Slots = 62;

FP_HD inline uint64_t mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

FP_HD inline uint64_t salt_of(uint64_t seed)
{
    return mix64(seed + 0x9E3779B97F4A7C15ull);
}

FP_HD inline unsigned complement(unsigned b)
{
    // without a branch: 'a' ^ 't' == 'A' ^ 'T' == 0x15, 'c' ^ 'g' == 'C' ^ 'G' == 0x04; bit 5 is the case
    const unsigned lower = b | 0x20u;
    const unsigned flip = (lower == 'a' || lower == 't') ? 0x15u : (lower == 'c' || lower == 'g') ? 0x04u : 0u;
    return b ^ flip;
}

// base j of a read: its term of S(x) ...
FP_HD inline uint64_t term(uint64_t salt, uint64_t j, unsigned b)
{
    return mix64(salt + 256ull * j + (uint64_t)b);
}

// ... and of S(rc(x)), where it stands at len - 1 - j, complemented
FP_HD inline uint64_t term_rc(uint64_t salt, uint64_t j, uint64_t len, unsigned b)
{
    return mix64(salt + 256ull * (len - 1ull - j) + (uint64_t)complement(b));
}

FP_HD inline uint64_t finish(uint64_t sum, uint64_t len, uint64_t seed)
{
    return mix64(mix64(sum + seed) + len);
}

FP_HD inline uint64_t key_mask(int fp_bits) // fp_bits in 1 .. 63
{
    return (1ull << fp_bits) - 1ull;
}

// the key of a read from its two sums (sum_rc is not looked at forward only)
FP_HD inline uint64_t key_of(uint64_t sum, uint64_t sum_rc, uint64_t len, uint64_t seed, int reverse_complement, int fp_bits)
{
    uint64_t f = finish(sum, len, seed);
    if (reverse_complement) {
        const uint64_t g = finish(sum_rc, len, seed);
        f = g < f ? g : f;
    }
    return f & key_mask(fp_bits);
}

// the sums of bases [lo, hi) of a read of len bases: a lane's share, or with (0, len) the whole read
FP_HD inline void add_share(const unsigned char *x, uint64_t lo, uint64_t hi, uint64_t len, uint64_t salt, uint64_t &sum,
                            uint64_t &sum_rc)
{
    for (uint64_t j = lo; j < hi; ++j) {
        sum += term(salt, j, x[j]);
        sum_rc += term_rc(salt, j, len, x[j]);
    }
}

// log2 of the table's slots (16 bytes each): the smallest power of two that is at least 2 * n_reads, and 2^10
FP_HD inline int table_log2_slots(int64_t n_reads)
{
    int lg = kMinLog2Slots;
    while (lg < kMaxLog2Slots && ((int64_t)1 << lg) / 2 < n_reads)
        ++lg;
    return lg;
}

FP_HD inline uint64_t slot_of(uint64_t key, int log2_slots)
{
    return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots); // Fibonacci hashing, as kmer_table.h's
}

} // namespace fingerprint
} // namespace covest
