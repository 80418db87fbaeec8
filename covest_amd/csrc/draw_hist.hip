// draw_hist.hip -- K-draw: replicate histograms drawn from a weight vector, the generator of the parametric bootstrap
// (covest_draw_histograms*; the definition is in include/covest_amd.h).
//
//   draw d of replicate b   block (lo32(d>>1), hi32(d>>1), b, 7): u = (w0 | w1 << 32) >> 1 for an even d,
//                           (w2 | w3 << 32) >> 1 for an odd one; its cell = #{i <= m - 2 : t_i <= u}
//   out[b - first_rep][i]   the number of draws d < n of replicate b in cell i (int64; the host zeroes it first)
//
// LAYOUT.  A workgroup takes one chunk of kDrawChunk draws of one replicate (grid: chunks x replicates); a lane a
// Philox block, both of its draws.  Everything is integer, every atomic a vector instruction: the counts are exact and
// do not depend on the chunk size or on the order of anything.
//   thresholds  t_0 .. t_{m-2} in LDS while they fit (m <= kDrawLdsThrCells), else read through L2
//   guide       guide[g] = #{i <= m - 2 : t_i < g << 52}, g = 0 .. 2048, built by the workgroup: a draw's cell lies in
//               [guide[u >> 52], guide[(u >> 52) + 1]], and the binary search runs over that range only -- over
//               nothing at all where a cell is wider than a guide bucket, which is where most draws land
//   counters    32-bit in LDS while they fit beside the thresholds (m <= kDrawLdsBothCells), flushed after a barrier
//               with one 64-bit atomic add a non-zero counter; else every draw adds to HBM
//   hot cells   the modal cell of a model histogram takes a tenth of all draws: six lanes of a wave on one address,
//               which the LDS serialises.  The up to kHot widest cells (of those at least 2^-6 wide) are counted by
//               ballot into scalar registers of the wave instead, and only the other lanes issue an atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "kernels.h"
#include "sim_philox.h"

#ifndef COVEST_DRAW_HOT
#define COVEST_DRAW_HOT 8 // (0: every draw takes an atomic -- the A/B of DESIGN.md 6p, built beside the library)
#endif

namespace covest {

namespace {

using u64 = unsigned long long;

constexpr int kDrawThreads = 1024;
constexpr int kGuideShift = 63 - kDrawGuideBits;
constexpr int kHot = COVEST_DRAW_HOT;
constexpr int kHotSlots = kHot > 0 ? kHot : 1;
constexpr int kCandMax = 64;                 // cells at least 2^-6 wide: there are at most 64
constexpr u64 kCandWidth = 1ull << (63 - 6);
constexpr unsigned kNoCell = 0xffffffffu;    // an unused hot slot
constexpr unsigned kNoDraw = 0xfffffffeu;    // the cell of a lane without a draw
constexpr size_t kDynMaxBytes = (size_t)kDrawLdsBothCells * 12; // >= (kDrawLdsThrCells - 1) * 8
static_assert((size_t)(kDrawLdsThrCells - 1) * 8 <= kDynMaxBytes, "dynamic LDS of the two layouts");
static_assert(kDynMaxBytes + 8192 <= 160 * 1024, "LDS of a CU: the dynamic part and (at most 8 KiB of) the static one");
static_assert(kDrawMaxCells - 1 <= 0xffff, "the guide holds 16-bit counts");
static_assert(kDrawChunk % 2 == 0 && kDrawChunk < (1ll << 32), "a chunk starts on a Philox block and fits 32-bit counters");

template <bool THR_LDS>
__device__ inline u64 thr_at(const u64 *thr_s, const u64 *__restrict__ thr_g, const unsigned i)
{
    return THR_LDS ? thr_s[i] : thr_g[i];
}

// #{i < n_thr : t_i <= u}, the guide narrowing the range first
template <bool THR_LDS>
__device__ inline unsigned cell_of(const u64 u, const unsigned short *guide, const u64 *thr_s, const u64 *__restrict__ thr_g)
{
    const unsigned g = (unsigned)(u >> kGuideShift); // < kDrawGuide: u < 2^63
    unsigned lo = guide[g], hi = guide[g + 1];
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1; // < hi <= m - 1
        if (thr_at<THR_LDS>(thr_s, thr_g, mid) <= u)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo; // <= m - 1
}

template <bool THR_LDS, bool CNT_LDS>
__global__ __launch_bounds__(kDrawThreads) void draw_hist_kernel(const u64 *__restrict__ thr, const unsigned m, const long long n,
                                                                 const long long chunk0, const unsigned rep0,
                                                                 const uint32_t key0, const uint32_t key1,
                                                                 u64 *__restrict__ out)
{
    extern __shared__ u64 dyn[]; // t_0 .. t_{m-2} (THR_LDS), then m counters (CNT_LDS)
    __shared__ unsigned short guide[kDrawGuide + 1];
    __shared__ u64 cand_w[kCandMax];
    __shared__ unsigned cand_i[kCandMax];
    __shared__ unsigned n_cand;
    __shared__ unsigned hot_s[kHotSlots], hot_total[kHotSlots];

    const unsigned tid = threadIdx.x;
    const unsigned n_thr = m - 1;
    u64 *thr_s = dyn;
    unsigned *cnt_s = reinterpret_cast<unsigned *>(dyn + (THR_LDS ? n_thr : 0));
    u64 *row = out + (long long)blockIdx.y * (long long)m;

    if (tid == 0)
        n_cand = 0;
    if (tid < (unsigned)kHotSlots)
        hot_s[tid] = kNoCell, hot_total[tid] = 0;
    if (THR_LDS)
        for (unsigned i = tid; i < n_thr; i += kDrawThreads)
            thr_s[i] = thr[i];
    if (CNT_LDS)
        for (unsigned i = tid; i < m; i += kDrawThreads)
            cnt_s[i] = 0;
    __syncthreads();

    // the guide: lower bounds of the bucket edges g << 52, g = 0 .. 2048 (the last edge is 2^63)
    for (unsigned g = tid; g <= (unsigned)kDrawGuide; g += kDrawThreads) {
        const u64 edge = (u64)g << kGuideShift;
        unsigned lo = 0, hi = n_thr;
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if (thr_at<THR_LDS>(thr_s, thr, mid) < edge)
                lo = mid + 1;
            else
                hi = mid;
        }
        guide[g] = (unsigned short)lo;
    }
    // the hot cells: the (at most 64) cells at least 2^-6 wide, then the kHot widest of them (ties: the lower index)
    if (kHot > 0) {
        for (unsigned i = tid; i < m; i += kDrawThreads) {
            const u64 below = i ? thr_at<THR_LDS>(thr_s, thr, i - 1) : 0ull;
            const u64 above = i < n_thr ? thr_at<THR_LDS>(thr_s, thr, i) : (1ull << 63);
            if (above - below >= kCandWidth) { // (ascending thresholds: no wrap)
                const unsigned slot = atomicAdd(&n_cand, 1u);
                if (slot < (unsigned)kCandMax)
                    cand_w[slot] = above - below, cand_i[slot] = i;
            }
        }
    }
    __syncthreads();
    if (kHot > 0) {
        const unsigned nc = n_cand < (unsigned)kCandMax ? n_cand : (unsigned)kCandMax;
        if (tid < nc) {
            const u64 w = cand_w[tid];
            const unsigned idx = cand_i[tid];
            unsigned rank = 0;
            for (unsigned o = 0; o < nc; ++o)
                rank += (cand_w[o] > w || (cand_w[o] == w && cand_i[o] < idx)) ? 1u : 0u;
            if (rank < (unsigned)kHot)
                hot_s[rank] = idx;
        }
        __syncthreads();
    }
    unsigned hot[kHotSlots], hot_n[kHotSlots];
#pragma unroll
    for (int h = 0; h < kHotSlots; ++h) {
        hot[h] = __builtin_amdgcn_readfirstlane(hot_s[h]);
        hot_n[h] = 0;
    }

    // the chunk's draws [d0, d1) are the Philox blocks [j0, j1); every wave runs the same number of rounds (ballots)
    const long long d0 = (chunk0 + (long long)blockIdx.x) * kDrawChunk;
    const long long d1 = n - d0 < kDrawChunk ? n : d0 + kDrawChunk;
    const long long j0 = d0 >> 1, j1 = (d1 + 1) >> 1;
    const PhiloxKey key{key0, key1};
    const uint32_t rep = rep0 + blockIdx.y;
    for (long long base = j0; base < j1; base += kDrawThreads) {
        const long long j = base + tid;
        uint32_t w[4];
        philox_block((u64)j, rep, kStreamDraw, key, w);
        const u64 u[2] = {((u64)w[0] | ((u64)w[1] << 32)) >> 1, ((u64)w[2] | ((u64)w[3] << 32)) >> 1};
        const bool has[2] = {j < j1, j < j1 && 2 * j + 1 < d1}; // (the last block of an odd n: its first draw only)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned cell = kNoDraw;
            if (has[s])
                cell = cell_of<THR_LDS>(u[s], guide, thr_s, thr);
            bool pending = has[s];
            if (kHot > 0) {
#pragma unroll
                for (int h = 0; h < kHotSlots; ++h) {
                    const bool is = cell == hot[h];
                    hot_n[h] += (unsigned)__popcll(__ballot(is));
                    pending = pending && !is;
                }
            }
            if (pending) {
                if (CNT_LDS)
                    atomicAdd(&cnt_s[cell], 1u);
                else
                    atomicAdd(&row[cell], 1ull);
            }
        }
    }
    if (kHot > 0 && (tid & 63u) == 0) {
#pragma unroll
        for (int h = 0; h < kHotSlots; ++h)
            if (hot_n[h])
                atomicAdd(&hot_total[h], hot_n[h]);
    }
    __syncthreads();
    if (CNT_LDS)
        for (unsigned i = tid; i < m; i += kDrawThreads) {
            const unsigned c = cnt_s[i];
            if (c)
                atomicAdd(&row[i], (u64)c);
        }
    if (kHot > 0 && tid < (unsigned)kHot && hot_s[tid] != kNoCell && hot_total[tid])
        atomicAdd(&row[hot_s[tid]], (u64)hot_total[tid]); // hot_s[tid] < m
}

template <bool THR_LDS, bool CNT_LDS>
hipError_t launch_variant(const u64 *thr, unsigned m, long long n, uint64_t first_rep, int64_t n_rep, PhiloxKey key,
                          u64 *out, hipStream_t stream)
{
    const size_t lds = (THR_LDS ? (size_t)(m - 1) * 8 : 0) + (CNT_LDS ? (size_t)m * 4 : 0);
    if (lds > 48 * 1024) { // the dynamic-LDS ceiling is a per-device attribute of the kernel: raised once per device
        static bool configured[64] = {false};
        static std::mutex configured_lock;
        std::lock_guard<std::mutex> guard(configured_lock);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
            dev = 0;
        if (!configured[dev]) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&draw_hist_kernel<THR_LDS, CNT_LDS>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDynMaxBytes);
            if (e != hipSuccess)
                return e;
            configured[dev] = true;
        }
    }
    const long long n_chunks = n / kDrawChunk + (n % kDrawChunk != 0);
    constexpr long long kChunksPerLaunch = 1ll << 30, kRepsPerLaunch = 65535; // (what a grid's x and y hold)
    for (int64_t r0 = 0; r0 < n_rep; r0 += kRepsPerLaunch)
        for (long long c0 = 0; c0 < n_chunks; c0 += kChunksPerLaunch) {
            const dim3 grid((unsigned)std::min(kChunksPerLaunch, n_chunks - c0),
                            (unsigned)std::min<int64_t>(kRepsPerLaunch, n_rep - r0));
            hipLaunchKernelGGL((draw_hist_kernel<THR_LDS, CNT_LDS>), grid, dim3(kDrawThreads), lds, stream, thr, m, n, c0,
                               (unsigned)(first_rep + (uint64_t)r0), key.k0, key.k1, out + r0 * (int64_t)m);
        }
    return hipGetLastError();
}

} // namespace

hipError_t launch_draw_hist(const uint64_t *thr, int64_t m, int64_t n, uint64_t first_rep, int64_t n_rep, uint64_t seed,
                            int64_t *out, hipStream_t stream)
{
    if (m < 1 || m > kDrawMaxCells || n < 0 || n_rep < 0 || first_rep + (uint64_t)n_rep > (1ull << 32))
        return hipErrorInvalidValue;
    if (n_rep == 0)
        return hipSuccess;
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)n_rep * (size_t)m * sizeof(int64_t), stream);
    if (e != hipSuccess || n == 0)
        return e;
    const PhiloxKey key = philox_key(seed);
    const u64 *t = reinterpret_cast<const u64 *>(thr);
    u64 *o = reinterpret_cast<u64 *>(out);
    if (m <= kDrawLdsBothCells)
        return launch_variant<true, true>(t, (unsigned)m, n, first_rep, n_rep, key, o, stream);
    if (m <= kDrawLdsThrCells)
        return launch_variant<true, false>(t, (unsigned)m, n, first_rep, n_rep, key, o, stream);
    return launch_variant<false, false>(t, (unsigned)m, n, first_rep, n_rep, key, o, stream);
}

} // namespace covest
