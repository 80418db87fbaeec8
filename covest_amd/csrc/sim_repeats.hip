// sim_repeats.hip -- K-repeat: a genome whose k-mers have a prescribed copy-number distribution, written where the
// read simulator takes it (covest_repeat_genome*).  The genome is n_units units of unit_len
// bases; unit u is a copy of family plan[u] >> 1, forward iff plan[u] & 1, else reverse-complemented; the copy is then
// mutated away from its family at rate `divergence`.  Philox4x32-10 (sim_philox.h), key = seed:
//   family base g = f * unit_len + offset   block (lo32(g>>2), hi32(g>>2), 0, 3), word g & 3, "ACGT"[word >> 30]
//   genome base i, divergence               block (lo32(i>>2), hi32(i>>2), 0, 6), word w = out[i & 3]: substituted iff
//                                           w < thr, by the base of code (code + 1 + w % 3) & 3 (the reads' rule)
//
// LAYOUT.  The cost is the Philox blocks, not the stores, so a block is computed once.  A family block is aligned to
// g, a divergence block to i, the caller's buffer to neither: the output goes through tile_image.h; a workgroup
//   1. loads the plan entries of the units that touch its tile into LDS,
//   2. computes the family blocks that touch the tile -- an item is (unit of the tile, block of four family bases) --
//      and puts those of their characters that lie in the unit's part of the tile into the image (a reverse unit
//      fills its dword from the top: the same store),
//   3. after a barrier, applies the divergence blocks that touch the tile to the image (skipped when thr == 0),
//   4. stores the image.
// Nothing outside [out, out + n) is written.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sim_philox.h"
#include "tile_image.h"

namespace covest {

namespace {

constexpr int kRepMaxUnits = kImageTile;       // units that can touch a tile (unit_len 1: a unit a byte)

// The part of one unit that lies in the tile, in family coordinates: the family bases [glo, ghi] go to the image; base
// g of them to place q_fwd + (g - g0) of a forward unit, q_rev - (g - g0) of a reverse one.
struct UnitPart {
    unsigned long long g0, glo, ghi;
    long long q_fwd, q_rev;
    bool fwd;
};

__device__ __forceinline__ UnitPart unit_part(const long long rec, const long long unit, const int unit_len,
                                              const long long t_begin, const long long o_begin, const long long o_end)
{
    UnitPart p;
    p.fwd = rec & 1;
    p.g0 = ((unsigned long long)rec >> 1) * (unsigned long long)unit_len;
    const long long start = unit * (long long)unit_len;
    // offsets [a, b] of the unit that lie in [o_begin, o_end): the unit touches the tile, so a <= b
    const long long a = o_begin > start ? o_begin - start : 0;
    const long long b = o_end - 1 - start < unit_len - 1 ? o_end - 1 - start : unit_len - 1;
    p.glo = p.g0 + (unsigned long long)(p.fwd ? a : unit_len - 1 - b);
    p.ghi = p.g0 + (unsigned long long)(p.fwd ? b : unit_len - 1 - a);
    p.q_fwd = start - t_begin;
    p.q_rev = start - t_begin + (unit_len - 1);
    return p;
}

__global__ __launch_bounds__(kImageThreads) void repeat_genome_kernel(
    const long long *__restrict__ plan, const int unit_len, const long long n, const unsigned long long thr,
    const uint32_t key0, const uint32_t key1, unsigned char *__restrict__ out, const int lead, const long long tile0)
{
    __shared__ long long unit_rec[kRepMaxUnits];                 // family << 1 | forward, per unit of the tile
    __shared__ __attribute__((aligned(16))) unsigned char image[kImageTile];

    const int tid = threadIdx.x;
    const PhiloxKey key{key0, key1};
    const TileSpan span = tile_span(tile0 + (long long)blockIdx.x, lead, n);
    const long long t_begin = span.t_begin, o_begin = span.o_begin, o_end = span.o_end;
    if (o_begin >= o_end)
        return; // (uniform: never taken for the tiles the host launches)
    const long long u_first = o_begin / unit_len;
    const int n_ut = (int)((o_end - 1) / unit_len - u_first) + 1; // <= kRepMaxUnits

    // 1. the plan's entries
    for (int t = tid; t < n_ut; t += kImageThreads)
        unit_rec[t] = plan[u_first + t];
    __syncthreads();

    // 2. items: (unit of the tile, block of four family bases).  A part of `len` bases spans at most (len + 2) / 4 + 1
    // blocks, and no part is longer than the tile: nb slots a unit.  The first unit's blocks sit at the END of its
    // slots and the last unit's at the beginning, so the items [t_lo, t_hi) hold no idle run but the one slot by which
    // a unit's alignment to g may fall short of nb.
    // (Where unit_len % 4 == 0 a family starts on a block, and a part within a unit spans at most unit_len / 4.)
    const int part_max = unit_len < kImageTile ? unit_len : kImageTile;
    const int nb = (unit_len & 3) == 0 && unit_len <= kImageTile ? unit_len >> 2 : ((part_max + 2) >> 2) + 1;
    int t_lo, t_hi;
    {
        const UnitPart first = unit_part(unit_rec[0], u_first, unit_len, t_begin, o_begin, o_end);
        const UnitPart last = unit_part(unit_rec[n_ut - 1], u_first + n_ut - 1, unit_len, t_begin, o_begin, o_end);
        t_lo = nb - ((int)((first.ghi >> 2) - (first.glo >> 2)) + 1);
        t_hi = n_ut == 1 ? nb : (n_ut - 1) * nb + (int)((last.ghi >> 2) - (last.glo >> 2)) + 1;
    }
    for (int t = t_lo + tid; t < t_hi; t += kImageThreads) {
        const int ul = (int)((unsigned)t / (unsigned)nb);
        const int j = t - ul * nb - (ul == 0 ? t_lo : 0);
        const UnitPart p = unit_part(unit_rec[ul], u_first + ul, unit_len, t_begin, o_begin, o_end);
        const unsigned long long blk = (p.glo >> 2) + (unsigned)j;
        if (blk > (p.ghi >> 2))
            continue;
        uint32_t w[4];
        philox_block(blk, 0u, kStreamFamily, key, w);
        const unsigned long long g4 = blk << 2;
        const long long d4 = (long long)(g4 - p.g0); // offset of the block's base 0 in the family: >= -3
        // byte b of the dword at q_low is family base g4 + b (forward) or the complement of g4 + 3 - b (reverse)
        const int q_low = (int)(p.fwd ? p.q_fwd + d4 : p.q_rev - d4 - 3);
        unsigned packed = 0;
        bool all = true;
        bool have[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned long long g = p.fwd ? g4 + (unsigned)b : g4 + (unsigned)(3 - b);
            have[b] = g >= p.glo && g <= p.ghi;
            all = all && have[b];
            const unsigned code = p.fwd ? w[b] >> 30 : 3u - (w[3 - b] >> 30);
            packed |= char_of(code) << (8 * b);
        }
        // one 32-bit LDS store where the place is aligned and the block lies within the unit's part, else bytes in LDS
        if (all && (q_low & 3) == 0) { // (all: the four places lie in the tile)
            *reinterpret_cast<unsigned *>(image + q_low) = packed;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (have[b])
                    image[q_low + b] = (unsigned char)(packed >> (8 * b));
        }
    }
    __syncthreads();

    // 3. divergence: the blocks of four GENOME bases that touch the tile, over the image
    if (thr != 0) {
        const long long b_first = o_begin >> 2;
        const int n_blk = (int)(((o_end - 1) >> 2) - b_first) + 1; // <= kImageTile / 4 + 1
        for (int t = tid; t < n_blk; t += kImageThreads) {
            const unsigned long long blk = (unsigned long long)(b_first + t);
            uint32_t w[4];
            philox_block(blk, 0u, kStreamDivergence, key, w);
            const long long i0 = (long long)(blk << 2);
            const int q0 = (int)(i0 - t_begin); // in (-4, kImageTile)
            if (i0 >= o_begin && i0 + 4 <= o_end && (q0 & 3) == 0) {
                const unsigned v = *reinterpret_cast<const unsigned *>(image + q0);
                unsigned packed = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    packed |= char_of(substituted(code_of((v >> (8 * b)) & 0xffu), w[b], thr)) << (8 * b);
                *reinterpret_cast<unsigned *>(image + q0) = packed;
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (i0 + b >= o_begin && i0 + b < o_end && (unsigned long long)w[b] < thr)
                        image[q0 + b] = (unsigned char)char_of(other_base(code_of(image[q0 + b]), w[b]));
            }
        }
        __syncthreads();
    }

    // 4. the image to memory
    store_image(out, image, span, tid);
}

} // namespace

hipError_t launch_repeat_genome(const int64_t *plan, int unit_len, int64_t n, uint64_t thr, uint64_t seed,
                                unsigned char *out, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    if (unit_len < 1)
        return hipErrorInvalidValue;
    const int lead = image_lead(out);
    const PhiloxKey key = philox_key(seed);
    return for_tile_launches(image_tiles(n, lead), [&](int64_t tile0, unsigned count) {
        hipLaunchKernelGGL(repeat_genome_kernel, dim3(count), dim3(kImageThreads), 0, stream,
                           reinterpret_cast<const long long *>(plan), unit_len, (long long)n, (unsigned long long)thr,
                           key.k0, key.k1, out, lead, (long long)tile0);
    });
}

} // namespace covest
