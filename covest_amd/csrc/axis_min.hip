// axis_min.hip -- K-axis-min: the selection scan of covest/grid.py:65-70 (cand.h: strict <, the lowest flat index
// wins a tie, NaN never wins, +inf never wins) run once PER CELL of the product of the kept axes, over the LL buffer
// of one GPU's block of the grid.  Mask 0 keeps nothing and is K-argmin's pair; all-ones keeps every point.
//
// The axes are first brought to a canonical form on the host (axis_min_plan): axes of length 1 drop out, adjacent axes
// that are both kept or both reduced merge into one group.  What is left alternates kept / reduced: at most three
// groups of each for five axes, so a point's flat index is
//     flat = sum_k coord_k * kstride_k  +  sum_r coord_r * rstride_r
// with at most two divisions on either side.  For a fixed cell the flat index rises with the row-major number of the
// reduced coordinates (`r`), so "ascending r" is "ascending flat index" and strict < keeps the first occurrence.
//
// Streaming read of 8 bytes a point; loads run along the fastest group whichever side it is on:
//   * fastest group REDUCED: one WAVE per (cell, slice of r) -- lane l takes r = begin + l, + 64, ...: adjacent lanes read
//     adjacent doubles -- and a butterfly of better() over the lanes;
//   * fastest group KEPT: one THREAD per (cell, slice of r), adjacent threads adjacent cells, i.e. adjacent doubles.
// A cell's r range is cut into slices where the cells alone would not fill the chip; every (cell, slice) leaves one
// candidate and a second launch walks a cell's slices in ascending order.  No atomics: better() is a total order on
// the candidates, so the result does not depend on the launch shape.  A block [flat_begin, flat_end) that begins or
// ends inside a cell contributes the points it holds; the slowest group's coordinates it does not touch are not walked.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cand.h"
#include "kernels.h"
#include "wave.h"

namespace covest {

namespace {

// x / d and x % d; both below 2^32 (every grid but the very largest): one 32-bit division
__host__ __device__ __forceinline__ void div_mod(int64_t x, int64_t d, int64_t &quot, int64_t &rem)
{
    if (((x | d) >> 32) == 0) {
        const uint32_t q = (uint32_t)x / (uint32_t)d;
        quot = q;
        rem = (uint32_t)x - q * (uint32_t)d;
    } else {
        quot = x / d;
        rem = x - quot * d;
    }
}

// sum coord_g * stride_g of the row-major number `idx` over n groups (lengths len[], last fastest); *lead: coord_0
__host__ __device__ __forceinline__ int64_t offset_of(int64_t idx, int n, const int64_t *len, const int64_t *stride, int64_t *lead)
{
    int64_t off = 0;
#pragma unroll
    for (int g = 2; g >= 1; --g)
        if (g < n) {
            int64_t c;
            div_mod(idx, len[g], idx, c);
            off += c * stride[g];
        }
    *lead = idx;
    return n > 0 ? off + idx * stride[0] : 0;
}

// the candidate of one (cell, slice) as lane `lane` of `n_lanes` sees it: r = begin + lane, + n_lanes, ...
__host__ __device__ __forceinline__ Cand scan_slice(const AxisMinPlan &p, const double *__restrict__ ll, int64_t cell, int64_t slice,
                                                    int lane, int n_lanes)
{
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    int64_t lead;
    const int64_t cell_off = offset_of(cell, p.n_kept, p.klen, p.kstride, &lead);
    if (p.first_kept && (lead < p.lead_lo || lead > p.lead_hi))
        return c; // (a cell the block does not touch)
    const int64_t begin = p.r_begin + slice * p.per_slice, end = begin + p.per_slice < p.r_end ? begin + p.per_slice : p.r_end;
    for (int64_t r0 = begin + lane; r0 < end; r0 += 4 * (int64_t)n_lanes) {
        double v[4];
        int64_t f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { // four loads in flight
            const int64_t r = r0 + (int64_t)u * n_lanes;
            int64_t unused;
            f[u] = r < end ? cell_off + offset_of(r, p.n_red, p.rlen, p.rstride, &unused) : -1;
            const bool in_block = f[u] >= p.flat_begin && f[u] < p.flat_end;
            v[u] = in_block ? -ll[f[u] - p.flat_begin] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v[u] < c.v) { // ascending flat index within a lane: strict < keeps the first occurrence
                c.v = v[u];
                c.i = f[u];
            }
    }
    return c;
}

__device__ __forceinline__ void store(Cand c, bool final, int64_t at, double *__restrict__ v, int64_t *__restrict__ i)
{
    v[at] = c.v;
    i[at] = (final && c.i == INT64_MAX) ? -1 : c.i;
}

// unit u = slice * n_cells + cell: a slice's candidates lie side by side.  final: one slice -- they are the result.
__global__ __launch_bounds__(256) void axis_min_wave(const AxisMinPlan p, const double *__restrict__ ll, double *__restrict__ pv,
                                                     int64_t *__restrict__ pi)
{
    const int64_t unit = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (unit >= p.n_cells * p.n_slices)
        return; // (wave-uniform)
    int64_t slice, cell;
    div_mod(unit, p.n_cells, slice, cell);
    const Cand c = wave_best(scan_slice(p, ll, cell, slice, threadIdx.x & (kWave - 1), kWave));
    if ((threadIdx.x & (kWave - 1)) == 0)
        store(c, p.n_slices == 1, unit, pv, pi);
}

__global__ __launch_bounds__(256) void axis_min_thread(const AxisMinPlan p, const double *__restrict__ ll, double *__restrict__ pv,
                                                       int64_t *__restrict__ pi)
{
    const int64_t unit = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= p.n_cells * p.n_slices)
        return;
    int64_t slice, cell;
    div_mod(unit, p.n_cells, slice, cell);
    store(scan_slice(p, ll, cell, slice, 0, 1), p.n_slices == 1, unit, pv, pi);
}

// a cell's slices in ascending order (= ascending flat index)
__global__ __launch_bounds__(256) void axis_min_merge(int64_t n_cells, int64_t n_slices, const double *__restrict__ pv,
                                                      const int64_t *__restrict__ pi, double *__restrict__ out_v,
                                                      int64_t *__restrict__ out_i)
{
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells)
        return;
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    for (int64_t s = 0; s < n_slices; ++s) {
        Cand o;
        o.v = pv[s * n_cells + cell];
        o.i = pi[s * n_cells + cell];
        c = better(c, o);
    }
    store(c, true, cell, out_v, out_i);
}

} // namespace

bool axis_min_plan(const int64_t *len, int n_axes, uint32_t keep_mask, int64_t flat_begin, int64_t flat_end, AxisMinPlan *out)
{
    AxisMinPlan p{};
    for (int g = 0; g < 3; ++g)
        p.klen[g] = p.rlen[g] = 1, p.kstride[g] = p.rstride[g] = 0;
    p.n_cells = p.n_red_total = 1;
    p.flat_begin = flat_begin;
    p.flat_end = flat_end;
    int64_t stride[kMaxParams];
    int64_t total = 1;
    for (int d = n_axes - 1; d >= 0; --d) {
        stride[d] = total;
        total *= len[d];
    }
    int last_side = -1, first_side = -1; // 1: kept, 0: reduced (of the group before / the slowest group)
    int64_t lead_len = 1, lead_stride = total;
    for (int d = 0; d < n_axes; ++d) {
        if (len[d] == 1)
            continue;
        const int side = (keep_mask >> d) & 1;
        int32_t &n = side ? p.n_kept : p.n_red;
        int64_t *glen = side ? p.klen : p.rlen, *gstride = side ? p.kstride : p.rstride;
        if (side == last_side) { // merges with the group before: the strides nest
            glen[n - 1] *= len[d];
            gstride[n - 1] = stride[d];
        } else {
            if (n == 3)
                return false; // (cannot happen with five axes)
            glen[n] = len[d];
            gstride[n] = stride[d];
            ++n;
        }
        (side ? p.n_cells : p.n_red_total) *= len[d];
        if (first_side < 0)
            first_side = side;
        if (first_side == side && n == 1)
            lead_len = glen[0], lead_stride = gstride[0];
        last_side = side;
    }
    p.last_kept = last_side == 1;
    p.first_kept = first_side == 1;
    // the slowest group's coordinates the block touches
    const bool empty = flat_end <= flat_begin;
    p.lead_lo = empty ? 1 : flat_begin / lead_stride;
    p.lead_hi = empty ? 0 : (flat_end - 1) / lead_stride;
    p.r_begin = 0;
    p.r_end = empty ? 0 : p.n_red_total;
    if (!empty && first_side == 0) {
        const int64_t inner = p.n_red_total / lead_len;
        p.r_begin = p.lead_lo * inner;
        p.r_end = (p.lead_hi + 1) * inner;
    }
    // slices: where the cells alone are fewer than the units that fill the chip, and a slice keeps a few loads a lane
    const int64_t span = std::max<int64_t>(p.r_end - p.r_begin, 1);
    const int64_t want_units = p.last_kept ? (int64_t)2048 * kWave : 2048, min_slice = p.last_kept ? 8 : 8 * kWave;
    int64_t n_slices = std::min((want_units + p.n_cells - 1) / p.n_cells, (span + min_slice - 1) / min_slice);
    n_slices = std::max<int64_t>(n_slices, 1);
    p.per_slice = (span + n_slices - 1) / n_slices;
    if (!p.last_kept)
        p.per_slice = (p.per_slice + kWave - 1) / kWave * kWave;
    p.n_slices = (span + p.per_slice - 1) / p.per_slice;
    *out = p;
    return true;
}

hipError_t launch_axis_min(const AxisMinPlan &p, const double *ll, double *partial_val, int64_t *partial_idx, double *out_val,
                           int64_t *out_idx, hipStream_t stream)
{
    const int64_t units = p.n_cells * p.n_slices;
    const int64_t blocks = p.last_kept ? (units + 255) / 256 : (units + 256 / kWave - 1) / (256 / kWave);
    if (blocks < 1 || blocks > 0x7fffffff)
        return hipErrorInvalidValue;
    const bool one = p.n_slices == 1; // the first launch's candidates are the result
    if (p.last_kept)
        hipLaunchKernelGGL(axis_min_thread, dim3((unsigned)blocks), dim3(256), 0, stream, p, ll, one ? out_val : partial_val,
                           one ? out_idx : partial_idx);
    else
        hipLaunchKernelGGL(axis_min_wave, dim3((unsigned)blocks), dim3(256), 0, stream, p, ll, one ? out_val : partial_val,
                           one ? out_idx : partial_idx);
    if (!one)
        hipLaunchKernelGGL(axis_min_merge, dim3((unsigned)((p.n_cells + 255) / 256)), dim3(256), 0, stream, p.n_cells, p.n_slices,
                           partial_val, partial_idx, out_val, out_idx);
    return hipGetLastError();
}

} // namespace covest
