// sim_philox.h -- the random stream and the base code of the generators (sim_reads.hip, sample_reads.hip,
// sim_repeats.hip, abi_repeat.cpp): Philox4x32-10 as in Random123 (Salmon, Moraes, Dror, Shaw:
// "Parallel random numbers: as easy as 1, 2, 3", SC 2011), the table of its streams, and A, C, G, T = 0, 1, 2, 3.
// Plain C++ for device and host: the known answers are checked on the host too (tests/tile_image_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define COVEST_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define COVEST_HD inline
#endif

namespace covest {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u; // the round's multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u; // the key's increments

// Ten rounds of (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped
// after each.  The products are formed as 64-bit ones: one multiply-add instruction gives both halves on gfx950.
COVEST_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// w % 3 without a 32-bit multiply-high (a quarter-rate instruction, and the kernel's bound is those of the rounds):
// 4 = 1 (mod 3), so w is congruent to the sum of its base-4 digits -- the set even bits plus twice the set odd bits,
// at most 48 --, and d / 3 = (d * 171) >> 9 for d < 512.
COVEST_HD uint32_t mod3(uint32_t w)
{
    const uint32_t d = (uint32_t)__builtin_popcount(w & 0x55555555u) + 2u * (uint32_t)__builtin_popcount(w & 0xAAAAAAAAu);
    return d - 3u * ((d * 171u) >> 9);
}

// THE STREAMS.  A block's counter is (lo32(index), hi32(index), c2, stream) and its key (lo32(seed), hi32(seed)): the
// code-side twin of the table in include/covest_amd.h, which the numpy restatements under tests/ check.
//   stream      index             c2                            words used
//   read        read r            0: the header                 w0 | w1 << 32 the position, w2 & 1 the strand
//                                 1 + j: bases 4j .. 4j + 3     one a base: substituted()
//   genome      base i >> 2       0                             one a base: "ACGT"[w >> 30]
//   keep        read r            0                             w0 < thr: the sampler keeps the read
//   family      family base g>>2  0                             one a base: "ACGT"[w >> 30]
//   copies      family f          0                             w0 against the copy-number thresholds
//   shuffle     unit-list entry j 0                             w0 | w1 << 32 the sort key, w2 & 1 the orientation
//   divergence  genome base i>>2  0                             one a base: substituted()
//   draw        draw d >> 1       replicate b                   (w0 | w1 << 32) >> 1 an even d, (w2 | w3 << 32) >> 1 an odd
//   group       read r            0                             (w0 * G) >> 32: the read's group of G (split_reads.hip)
//   bootstrap   read r            replicate b                   w0 against kPoisson1Cdf: the read's multiplicity
// A new generator takes the next free number (and a row here and in the header); c2 is free in all but `read`, `draw` and
// `bootstrap`.
constexpr uint32_t kStreamRead = 0, kStreamGenome = 1, kStreamKeep = 2, kStreamFamily = 3, kStreamCopies = 4,
                   kStreamShuffle = 5, kStreamDivergence = 6, kStreamDraw = 7, kStreamGroup = 8, kStreamBootstrap = 9;

struct PhiloxKey { uint32_t k0, k1; };
COVEST_HD PhiloxKey philox_key(uint64_t seed) { return PhiloxKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
COVEST_HD void philox_block(uint64_t index, uint32_t c2, uint32_t stream, PhiloxKey key, uint32_t out[4])
{
    philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), c2, stream, key.k0, key.k1, out);
}

// THE READ BOOTSTRAP'S MULTIPLICITY (bootstrap_weights.hip): Poisson(1) by inversion on one word,
// m = #{i : w >= T_i}, T_i = floor(2^32 P(Poisson(1) <= i)), i = 0 .. 12.  The mass beyond 12 is 0.27 * 2^-32: the table is
// complete at 32 bits, and the largest m is 13.  The compares are a fixed thirteen: no lane takes a branch of its own.
constexpr int kPoisson1Steps = 13;
COVEST_HD uint32_t poisson1_multiplicity(uint32_t w)
{
    constexpr uint32_t kPoisson1Cdf[kPoisson1Steps] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u,
                                                       4292415291u, 4294609777u, 4294923276u, 4294962463u, 4294966817u,
                                                       4294967252u, 4294967292u, 4294967295u};
    uint32_t m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < kPoisson1Steps; ++i)
        m += w >= kPoisson1Cdf[i] ? 1u : 0u;
    return m;
}
// the multiplicity of read r in replicate b under `key`
COVEST_HD uint32_t bootstrap_weight(uint64_t r, uint32_t b, PhiloxKey key)
{
    uint32_t w[4];
    philox_block(r, b, kStreamBootstrap, key, w);
    return poisson1_multiplicity(w[0]);
}

// THE BASE CODE.  A, C, G, T = 0, 1, 2, 3, the complement of c is 3 - c.  ASCII a/c/g/t in either case: (byte >> 1) & 3
// gives 0, 1, 3, 2, and the Gray step puts G and T in order.  Any other byte gives SOME code: nothing is indexed by it.
constexpr uint32_t kAcgt = 0x54474341u; // "ACGT", code 0 in the low byte
COVEST_HD uint32_t code_of(uint32_t byte)
{
    const uint32_t c = (byte >> 1) & 3u;
    return c ^ (c >> 1);
}

COVEST_HD uint32_t char_of(uint32_t code) { return (kAcgt >> (8 * code)) & 0xffu; }
// the characters of four codes, the first in the low byte
COVEST_HD uint32_t pack_chars(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    return char_of(c0) | (char_of(c1) << 8) | (char_of(c2) << 16) | (char_of(c3) << 24);
}

// The substitution rule of reads and of divergence: the base changes iff its word w is below thr = floor(rate * 2^32),
// to one of the three others -- which, w % 3 says (other() of the reference's read_simulator.py:16-20).
COVEST_HD uint32_t other_base(uint32_t code, uint32_t w) { return (code + 1u + mod3(w)) & 3u; }
COVEST_HD uint32_t substituted(uint32_t code, uint32_t w, uint64_t thr)
{
    return (uint64_t)w < thr ? other_base(code, w) : code;
}

} // namespace covest
