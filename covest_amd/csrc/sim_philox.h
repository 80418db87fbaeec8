// sim_philox.h -- the random stream of the read simulator (sim_reads.hip): Philox4x32-10 as in
// Random123 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011).  Plain C++ for
// device and host: the known answers are checked on the host too.
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

} // namespace covest
