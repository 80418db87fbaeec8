// factored_contract.h -- K-factored, PHASE B (ll_factored.hip): P' = G' x b on the fp64 matrix pipe, for the six
// accumulator slots of a wave -- the steps of the contraction that stand on their own.  (The slot loop of the first
// MFMAs and the six loops of the remaining steps are written out in the kernel: as functions they move the walk's
// registers)
//   reads   the item's buffer of G' (LDS), the slots' offsets, cut-offs and weights, the lanes' bands
//   writes  the accumulators acc[slot] (f64 C/D layout: register r of a lane is row (lane >> 4) + 4 r, column lane & 15),
//           the running weights wrun, advanced
#pragma once
#include "band.h"
#include "factored_diag.h"
#include "factored_state.h"
#include "fastmath.h"
#include "tiles.h"
#include "wave.h"

namespace covest {

// One MFMA step of the first N accumulator slots of a wave (they are sorted by length, so the active
// slots are always a prefix): all A fragments first -- N independent LDS reads in flight -- then per
// slot the weight b_o (advanced by (1-q)^4, cut off at o >= T: models.py:198-206,239) and the MFMA.
// Straight-line code: no per-slot branch separates the reads from their MFMAs.
// (Measured and not kept, round 3: the fragments of step i + 1 read during step i -- 0.896 against 0.864 ms: the
// registers of the second set are spilled elsewhere.)
template <int N, int MU>
__device__ __forceinline__ void contract_step(int i, const double *cur, const int (&a_off)[MU], const int (&cut)[MU],
                                              const double (&r4)[MU], double (&wrun)[MU], d4 (&acc)[MU])
{
    double a[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
        a[k] = cur[a_off[k] + 4 * i];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double w = (i < cut[k]) ? wrun[k] : 0.0; // this lane's o has reached T: models.py:239
        wrun[k] *= r4[k];
        acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k], w, acc[k], 0, 0, 0);
    }
}

// this item's bands, out of the lanes' (lane = item of the walk, the last lane: every item from the 64th on)
__device__ __forceinline__ BandBytes bands_of_item(const BandBytes &lanes, int t)
{
    const int bl = min(__builtin_amdgcn_readfirstlane(t), kWave - 1);
    BandBytes b;
    b.w0 = (unsigned)__builtin_amdgcn_readlane((int)lanes.w0, bl);
    b.w1 = (unsigned)__builtin_amdgcn_readlane((int)lanes.w1, bl);
    return b;
}

// THE SHARED STEPS of a unit (tiles.h), summed on the vector unit:
//     sum_{i = 1 .. nsh} G'[key][1 + 4 i + kq] r^(i - 1),   r = (1-q)^4 (wave-uniform: the tile has one q)
// for this lane's key and o mod 4 -- weights RELATIVE TO THE FIRST shared step, so they only fall (the
// unscaled rows reach 1e297; with weights relative to the step AFTER the shared ones, up to 1e10, the sum
// could leave the range) -- as four Horner chains in r^4 (chain c: the steps i = 1 + c + 4 m) walked from
// the last step down, eight loads in flight per trip.  (Measured and not kept, round 3: the loads issued
// three groups ahead of their FMAs through a ring of four register sets, 0.934 against 0.872 ms -- the
// registers it takes are spilled elsewhere; and one fused pass over all the wave's units with one chain
// each, 1.08 ms.)
// g1: step 0 of the unit (o = 1 .. 4), step i at g1[4 i]; zp: the zeroed slack behind the buffers; rr16 = r^4, rr4 = r.
__device__ __forceinline__ double shared_steps_sum(const double *g1, int nsh_k, const double *zp, double rr16, double rr4)
{
    const int n4 = nsh_k >> 2, rem = nsh_k & 3;
    // the top `rem` steps (m = n4) are the heads of chains 0 .. rem - 1
    const double *top = g1 + 4 * (1 + 4 * n4);
    // the heads WITHOUT branches: a head that does not exist is read from the zeroed slack behind the buffers
    // (one select on the address), so that the three loads, the slot's constants above and the first trip's
    // eight are in flight together -- one LDS round trip at the top of a slot instead of three or four
    double h0 = *(rem > 0 ? top : zp), h1 = *(rem > 1 ? top + 4 : zp), h2 = *(rem > 2 ? top + 8 : zp), h3 = 0.0;
    {
        // The trips' reads are written out as ds_read_b64: left alone the compiler pairs them into
        // ds_read2_b64, which the LDS serves at half the rate and with banks counted mod 32 -- rows 8 apart
        // collide there (the row stride is 4 dwords mod 64: conflict-free for ds_read_b64 only).  The
        // compiler does not count reads it cannot see: the wait is part of the statement.
        unsigned qa = (unsigned)(uintptr_t)(top - 32); // LDS byte address of the trip's lowest step
        int gq = n4;
        for (; gq >= 2; gq -= 2, qa -= 256) { // eight loads in flight per trip
            double b0, b1, b2, b3, c0, c1, c2, c3;
            asm volatile("ds_read_b64 %0, %8 offset:128\n\tds_read_b64 %1, %8 offset:160\n\t"
                         "ds_read_b64 %2, %8 offset:192\n\tds_read_b64 %3, %8 offset:224\n\t"
                         "ds_read_b64 %4, %8\n\tds_read_b64 %5, %8 offset:32\n\t"
                         "ds_read_b64 %6, %8 offset:64\n\tds_read_b64 %7, %8 offset:96\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3), "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(c3)
                         : "v"(qa));
            h0 = fma_vvv(fma(h0, rr16, b0), rr16, c0); // (three-address: no copy back into the chain's register)
            h1 = fma_vvv(fma(h1, rr16, b1), rr16, c1);
            h2 = fma_vvv(fma(h2, rr16, b2), rr16, c2);
            h3 = fma_vvv(fma(h3, rr16, b3), rr16, c3);
        }
        if (gq > 0) {
            double b0, b1, b2, b3;
            asm volatile("ds_read_b64 %0, %4 offset:128\n\tds_read_b64 %1, %4 offset:160\n\t"
                         "ds_read_b64 %2, %4 offset:192\n\tds_read_b64 %3, %4 offset:224\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3)
                         : "v"(qa));
            h0 = fma_vvv(h0, rr16, b0);
            h1 = fma_vvv(h1, rr16, b1);
            h2 = fma_vvv(h2, rr16, b2);
            h3 = fma_vvv(h3, rr16, b3);
        }
    }
    return fma(fma(fma(h3, rr4, h2), rr4, h1), rr4, h0);
}

// pieces of one unit: add the accumulators into the unit's first slot.  A BRANCH per slot (the empty asm
// keeps the compiler from turning it into four adds and eight selects for every slot, taken or not)
template <int MU>
__device__ __forceinline__ void add_pieces(unsigned m_cont, d4 (&acc)[MU])
{
#pragma unroll
    for (int k = MU - 1; k >= 1; --k)
        if ((m_cont >> k) & 1u) { // wave-uniform
            asm volatile("" ::: "memory");
            acc[k - 1] += acc[k];
        }
}

} // namespace covest
