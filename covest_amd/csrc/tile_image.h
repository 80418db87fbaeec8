// tile_image.h -- the tile image of the generators (sim_reads.hip, sim_repeats.hip, sample_reads.hip; DESIGN.md
// section 6o): how a kernel that produces bytes at any alignment, for a buffer of any alignment, stores 16 bytes a lane.
// The output [0, total) of the caller's buffer `out` is cut into tiles of kImageTile bytes that are 16-byte aligned IN
// MEMORY.  A workgroup of kImageThreads lanes assembles a tile in an LDS image (byte stores happen there, in LDS)
// and store_image sends it out with one 16-byte vector store a lane, 1 KiB a wave instruction; only a lane whose 16
// bytes hang over either end of the caller's buffer (the first and the last tile) stores bytes.  This is the one piece
// of index arithmetic that decides whether a store leaves the caller's buffer: tests/tile_image_check.cpp walks it on
// the host for every alignment.  Two layers, as sim_philox.h: plain C++ first, what needs HIP under __HIPCC__.
#pragma once
#include <cstdint>

#include "sim_philox.h" // COVEST_HD

namespace covest {

constexpr int kImageThreads = 256;
constexpr int kImageTile = 16 * kImageThreads; // bytes of output a workgroup assembles at a time
constexpr int64_t kImageTilesPerLaunch = (int64_t)1 << 20; // 4 GiB and 2^28 threads a launch (HIP wraps grids beyond 2^32 threads)

// out & 15, the bytes by which the buffer starts behind a 16-byte boundary; the tiles that cover [0, total), total > 0
inline int image_lead(const void *out) { return (int)((uintptr_t)out & 15u); }
COVEST_HD long long image_tiles(long long total, int lead) { return (total + lead + kImageTile - 1) / kImageTile; }

// A tile in output bytes: [t_begin, t_begin + kImageTile), t_begin + lead a multiple of kImageTile (-lead for tile 0);
// the caller's part of it is [o_begin, o_end), empty only for a tile that image_tiles does not count.
struct TileSpan { long long t_begin, o_begin, o_end; };
COVEST_HD TileSpan tile_span(long long tile, int lead, long long total)
{
    const long long t_begin = tile * kImageTile - lead;
    return TileSpan{t_begin, t_begin > 0 ? t_begin : 0, t_begin + kImageTile < total ? t_begin + kImageTile : total};
}

// The store step's rule for lane tid, whose 16 bytes are the image's [16 * tid, 16 * tid + 16) and the output's
// [lane_at, lane_at + 16): lane_vector -- all 16 are the caller's, and the lane takes the 16-byte store (out + lane_at
// is 16-byte aligned: t_begin + lead is); else it stores the bytes b of 0..15 for which lane_byte holds, one by one.
COVEST_HD long long lane_at(const TileSpan &s, int tid) { return s.t_begin + 16 * tid; }
COVEST_HD bool lane_vector(const TileSpan &s, long long at) { return at >= s.o_begin && at + 16 <= s.o_end; }
COVEST_HD bool lane_byte(const TileSpan &s, long long at, int b) { return at + b >= s.o_begin && at + b < s.o_end; }

} // namespace covest

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace covest {

// The image (16-byte aligned, and whole: after a barrier) to memory, lane tid's 16 bytes by the lane rule above.
__device__ __forceinline__ void store_image(unsigned char *__restrict__ out, const unsigned char *image, const TileSpan s,
                                            const int tid)
{
    const long long at = lane_at(s, tid);
    if (lane_vector(s, at)) {
        *reinterpret_cast<uint4 *>(out + at) = *reinterpret_cast<const uint4 *>(image + 16 * tid);
        return;
    }
    for (int b = 0; b < 16; ++b)
        if (lane_byte(s, at, b))
            out[at + b] = image[16 * tid + b];
}

// fn(tile0, count) launches the workgroups of tiles [tile0, tile0 + count); stops at the first launch that fails
template <class Fn> hipError_t for_tile_launches(int64_t n_tiles, Fn fn)
{
    hipError_t e = hipSuccess;
    for (int64_t tile0 = 0; tile0 < n_tiles && e == hipSuccess; tile0 += kImageTilesPerLaunch) {
        fn(tile0, (unsigned)(n_tiles - tile0 < kImageTilesPerLaunch ? n_tiles - tile0 : kImageTilesPerLaunch));
        e = hipGetLastError();
    }
    return e;
}

} // namespace covest
#endif
