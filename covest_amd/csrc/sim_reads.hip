// sim_reads.hip -- K-sim: sequencing reads of known coverage and error rate, written where the k-mer counter reads
// them (covest_simulate_reads*, covest_random_genome*).
//
// The counterpart of the reference's tools/simulator/generate_sequence.py and read_simulator.py:60-88, with one
// deliberate difference: every output byte is a stated function of (seed, read index, base index) -- Philox4x32-10
// as in Random123 (sim_philox.h) -- where the reference draws from Python's unseeded `random`.
//   genome base i     block (lo32(i>>2), hi32(i>>2), 0, 1), word i & 3, "ACGT"[word >> 30]
//   read r, header    block (lo32(r), hi32(r), 0, 0): pos = mulhi64(w0 | w1 << 32, genome_len - read_len) (the
//                     exclusive end of randrange(genome_size - read_length), :75); forward if w2 & 1 (:77-78)
//   read r, base i    block (lo32(r), hi32(r), 1 + (i >> 2), 0), word w = out[i & 3]: substituted iff w < thr, by the
//                     base of code (code + 1 + w % 3) & 3 -- one of the three others, as other() at :16-20
//
// LAYOUT.  The cost is the Philox blocks (ten rounds of two 32 x 32 -> 64 multiplies for four bases), not the stores,
// so a block is computed once: an item is (read, block of four bases), one a lane.  A read starts at r * read_len,
// which is dword-aligned only when read_len % 4 == 0, and the caller's buffer need not be aligned either.  So the
// output goes through the tile image (tile_image.h); a workgroup
//   1. computes the header of every read that touches its tile, once, into LDS (and writes the read's origin record
//      if the read STARTS in the tile: one writer a read),
//   2. computes the items that touch the tile and puts their (up to) four characters at their place in the image,
//   3. stores the image.
// Nothing outside [d_bases, d_bases + n_reads * read_len) and d_origin[0 .. n_reads) is written.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sim_philox.h"
#include "tile_image.h"

namespace covest {

namespace {

constexpr int kSimMaxReads = kImageTile;       // reads that can touch a tile (read_len 1: a read a byte)
constexpr int kGenomeThreads = 256;

__global__ __launch_bounds__(kImageThreads) void sim_reads_kernel(
    const unsigned char *__restrict__ genome, const unsigned long long span, const int read_len,
    const unsigned long long first_read, const long long n_reads, const unsigned long long thr, const uint32_t key0,
    const uint32_t key1, const int both_strands, unsigned char *__restrict__ out, const int lead,
    const long long tile0, long long *__restrict__ origin)
{
    __shared__ long long hdr[kSimMaxReads];                      // pos << 1 | forward, per read of the tile
    __shared__ __attribute__((aligned(16))) unsigned char image[kImageTile];

    const int tid = threadIdx.x;
    const PhiloxKey key{key0, key1};
    const TileSpan span_t = tile_span(tile0 + (long long)blockIdx.x, lead, n_reads * (long long)read_len);
    const long long t_begin = span_t.t_begin, o_begin = span_t.o_begin, o_end = span_t.o_end;
    if (o_begin >= o_end)
        return; // (uniform: never taken for the tiles the host launches)
    const long long r_first = o_begin / read_len;
    const int n_rt = (int)((o_end - 1) / read_len - r_first) + 1; // <= kSimMaxReads

    // 1. headers
    for (int t = tid; t < n_rt; t += kImageThreads) {
        const unsigned long long r = first_read + (unsigned long long)(r_first + t);
        uint32_t w[4];
        philox_block(r, 0u, kStreamRead, key, w);
        const unsigned long long u = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
        const unsigned long long pos = __umul64hi(u, span);
        const long long rec = (long long)(pos << 1) | (long long)((w[2] & 1u) | (both_strands ? 0u : 1u));
        hdr[t] = rec;
        const long long start = (r_first + t) * (long long)read_len;
        if (origin && start >= o_begin) // (start < o_end: the read touches the tile)
            origin[r_first + t] = rec;
    }
    __syncthreads();

    // 2. items: (read of the tile, block of four bases)
    // numbered read by read, nb to a read; of the first and the last read only the blocks that touch the tile
    const int nb = (int)(((long long)read_len + 3) >> 2);
    const long long q_base = r_first * (long long)read_len - t_begin; // place of the first read's base 0 in the image: (-read_len, 16)
    const long long last_start = (r_first + n_rt - 1) * (long long)read_len;
    const int t_lo = (int)((o_begin - r_first * (long long)read_len) >> 2);
    const int t_hi = (n_rt - 1) * nb + (int)((o_end - 1 - last_start) >> 2) + 1; // <= kImageTile / 4 + 2 * n_rt
    for (int t = t_lo + tid; t < t_hi; t += kImageThreads) {
        const int rl = (int)((unsigned)t / (unsigned)nb);
        const int j = t - rl * nb;
        const int i0 = 4 * j;
        const int q0 = (int)(q_base + (long long)rl * read_len + i0); // in (-4, kImageTile): the block touches the tile
        const int n_here = read_len - i0 < 4 ? read_len - i0 : 4;
        const unsigned long long r = first_read + (unsigned long long)(r_first + rl);
        const long long rec = hdr[rl];
        const unsigned long long pos = (unsigned long long)rec >> 1;
        const bool forward = rec & 1;
        uint32_t w[4];
        philox_block(r, 1u + (uint32_t)j, kStreamRead, key, w);
        unsigned packed = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (b < n_here) {
                const int i = i0 + b;
                // pos + i and pos + read_len - 1 - i are at most pos + read_len - 1 < genome_len
                const unsigned c = code_of(genome[forward ? pos + (unsigned)i : pos + (unsigned)(read_len - 1 - i)]);
                packed |= char_of(substituted(forward ? c : 3u - c, w[b], thr)) << (8 * b);
            }
        }
        // one 32-bit LDS store where the place is aligned and whole, byte stores in LDS where it is not
        if (n_here == 4 && (q0 & 3) == 0 && q0 >= 0 && q0 + 4 <= kImageTile) {
            *reinterpret_cast<unsigned *>(image + q0) = packed;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < n_here && q0 + b >= 0 && q0 + b < kImageTile)
                    image[q0 + b] = (unsigned char)(packed >> (8 * b));
        }
    }
    __syncthreads();

    // 3. the image to memory
    store_image(out, image, span_t, tid);
}

// bases [4 * blk, 4 * blk + 4) of a random genome, one Philox block a lane; `aligned`: out is dword-aligned
__global__ __launch_bounds__(kGenomeThreads) void random_genome_kernel(const long long n, const uint32_t key0,
                                                                       const uint32_t key1, const int aligned,
                                                                       unsigned char *__restrict__ out)
{
    const long long n_blocks = (n + 3) >> 2;
    const long long stride = (long long)gridDim.x * kGenomeThreads;
    for (long long blk = (long long)blockIdx.x * kGenomeThreads + threadIdx.x; blk < n_blocks; blk += stride) {
        uint32_t w[4];
        philox_block((unsigned long long)blk, 0u, kStreamGenome, PhiloxKey{key0, key1}, w);
        const unsigned packed = pack_chars(w[0] >> 30, w[1] >> 30, w[2] >> 30, w[3] >> 30);
        const long long at = 4 * blk;
        if (aligned && at + 4 <= n) {
            *reinterpret_cast<unsigned *>(out + at) = packed;
        } else {
            for (int b = 0; b < 4; ++b)
                if (at + b < n)
                    out[at + b] = (unsigned char)(packed >> (8 * b));
        }
    }
}

} // namespace

hipError_t launch_random_genome(int64_t n, uint64_t seed, unsigned char *out, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    const int64_t n_blocks = (n + 3) >> 2;
    const int64_t want = (n_blocks + kGenomeThreads - 1) / kGenomeThreads;
    const dim3 block(kGenomeThreads), grid((unsigned)std::min<int64_t>(want, (int64_t)1 << 20)); // (the kernel strides)
    const PhiloxKey key = philox_key(seed);
    hipLaunchKernelGGL(random_genome_kernel, grid, block, 0, stream, (long long)n, key.k0, key.k1,
                       (int)(((uintptr_t)out & 3u) == 0), out);
    return hipGetLastError();
}

hipError_t launch_sim_reads(const unsigned char *genome, int64_t genome_len, int read_len, int64_t first_read,
                            int64_t n_reads, uint64_t thr, uint64_t seed, int both_strands, unsigned char *out,
                            int64_t *origin, hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    if (read_len < 1 || genome_len <= read_len || first_read < 0)
        return hipErrorInvalidValue;
    const int lead = image_lead(out);
    const PhiloxKey key = philox_key(seed);
    return for_tile_launches(image_tiles(n_reads * (int64_t)read_len, lead), [&](int64_t tile0, unsigned count) {
        hipLaunchKernelGGL(sim_reads_kernel, dim3(count), dim3(kImageThreads), 0, stream, genome,
                           (unsigned long long)(genome_len - read_len), read_len, (unsigned long long)first_read,
                           (long long)n_reads, (unsigned long long)thr, key.k0, key.k1, both_strands, out, lead,
                           (long long)tile0, reinterpret_cast<long long *>(origin));
    });
}

} // namespace covest
