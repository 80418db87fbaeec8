// ll_batch.hip -- K-batch: many histograms on ONE key set, scored in one pass.
//
// For a fixed key set p_j(theta) does not depend on the counts, and all of the likelihood's expensive work is in p_j
// (n_keys * S * (T - 1) pmf terms a point, ~30 fp64 instructions each in K-direct).  The counts enter through one dot
// product per histogram:
//     LL_b(theta_i) = sum_j h_bj log p_j(theta_i) + tail_b [sp_i < 1] log(1 - sp_i)
// so B histograms at n points are n evaluations of p and a B x n_keys x n contraction, not B n evaluations.
//
//   batch_table_kernel    one wave a point: direct_point_ll<P, true> (K-direct's arithmetic after clamp_point, bit for
//                         bit what covest_probabilities(clamp = 1) returns) writes p_ij into the point's table row, and
//                         the same wave turns the row into log p_ij.  Each lane re-reads exactly the elements it wrote
//                         itself (index = lane mod 64 in both loops), so no fence stands between the two passes.
//   batch_cross_kernel    out = H L^T by v_mfma_f64_16x16x4_f64.  Both operands are K-contiguous (H is B x n_keys, L is
//                         n x n_keys): a lane (r = lane & 15, kq = lane >> 4) loads FOUR consecutive keys
//                         j0 + 4 kq .. + 3 of row r of either operand -- 32 bytes a lane, 128 contiguous bytes a row
//                         per 16 keys -- and feeds them to four MFMA steps: step s contracts the keys j0 + 4 k + s,
//                         k = 0..3, the same permutation of the key order in A and in B.  A wave owns 16 histograms x
//                         64 points: one A fragment against four B fragments, four independent accumulators (the
//                         instruction's dependent latency is longer than its issue interval).  No LDS: every element
//                         is used by one lane only.  Padding of B, n and n_keys is a select IN THE LOAD (0 in both
//                         operands: 0 x garbage could be NaN).
//                         Operand maps (A[r][k = kq], B[k = kq][c = lane & 15], D: col = lane & 15, row = kq + 4 reg).
//   batch_fix_dead_kernel the reference's h * safe_log(0) = -inf: a key with p_ij <= 0 carries +0.0 in the table (so the
//                         contraction adds nothing for it) and the point is listed; one wave per (histogram, listed
//                         point) sets -inf where the histogram counts such a key.  A key with h_bj = 0 contributes
//                         nothing (covest/models.py:105-107, `if h`).
//   batch_pairs_kernel<R> histogram index[i] at point i, one wave a request, the dead-key rule inline; R rows a point,
//                         a request's R dot products in one sweep (R = 1: the value form).
//   batch_tail_pack_kernel, batch_grad_specials_kernel  the gradient and the Hessian of a batch (DESIGN.md sections 6u,
//                         6x): the same contraction over the derivative kernel's table, R = P + 1 rows a point for the
//                         gradient, R2 = 1 + P + P (P + 1) / 2 (6 and 21) with the curvature rows c_kl behind them.
//   batch_argmin_kernel   per histogram the first index of the strictly smallest -LL (covest/grid.py:65-70), carried
//                         across table chunks on the device.
//   batch_from_draw_kernel  int64 rows of draw_hist.hip to double counts and tails.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_host.h"
#include "cand.h"
#include "direct_point.h"
#include "kernels.h"

namespace covest {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kWavesPerBlock = 4;
constexpr int64_t kMaxBlocks = kBatchHostMaxBlocks; // HIP wraps a grid of more than 2^32 threads silently; the cuts are
                                                    // batch_host.h's (checked without a device)

__device__ __forceinline__ bool is_dead_entry(double l) { return __double_as_longlong(l) == 0ll; } // the bits of +0.0

template <int P>
__global__ __launch_bounds__(256) void batch_table_kernel(const DevModel m, const PointSource src, const int64_t n,
                                                          double *table, double *__restrict__ tl,
                                                          int32_t *__restrict__ dead, const int keep_p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t pt = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
    if (pt >= n)
        return; // wave-uniform
    const int64_t nk = m.bins.n;
    double *row = table + pt * nk;
    // counts 0 and tail 1 (the launcher's DevModel): the value IS log(1 - sp), or 0 where sp is not < 1
    const double t = direct_point_ll<P, true>(m, src, pt, row);
    int n_dead = 0;
    for (int64_t j = lane; j < nk; j += kWave) { // (the lane's own elements: see the head of the file)
        const double p = row[j];
        if (p <= 0.0) {
            ++n_dead;
            if (!keep_p)
                row[j] = 0.0;
        } else if (!keep_p) { // (NaN comes here and stays NaN)
            const double l = log(p);
            row[j] = l == 0.0 ? -0.0 : l; // p == 1: the bits of +0.0 are the dead keys' alone
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        n_dead += __shfl_xor(n_dead, off, kWave);
    if (lane == 0) {
        tl[pt] = t;
        dead[pt] = n_dead;
    }
}

// grid: x = groups of 64 points (from x0 on), y = groups of 4 histogram tiles; a wave = one tile of 16 histograms
__global__ __launch_bounds__(256) void batch_cross_kernel(const double *__restrict__ H, const double *__restrict__ tails,
                                                          const int64_t n_hist, const double *__restrict__ L,
                                                          const double *__restrict__ tl, const int64_t n, const int64_t nk,
                                                          double *__restrict__ out, const int64_t ld, const int64_t x0)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, kq = lane >> 4;
    const int64_t b0 = ((int64_t)blockIdx.y * kWavesPerBlock + (threadIdx.x / kWave)) * 16;
    const int64_t i0 = (x0 + (int64_t)blockIdx.x) * 64;
    if (b0 >= n_hist || i0 >= n)
        return; // wave-uniform: the MFMAs below run with every lane
    const bool b_ok = b0 + r < n_hist;
    const double *hrow = H + (b_ok ? b0 + r : 0) * nk;
    bool i_ok[4];
    const double *lrow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t i = i0 + t * 16 + r;
        i_ok[t] = i < n;
        lrow[t] = L + (i_ok[t] ? i : 0) * nk;
    }
    double4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
        acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int64_t j0 = 0; j0 < nk; j0 += 16) {
        const int64_t j = j0 + 4 * kq;
        double a[4], b[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool in = j + s < nk;
            a[s] = (b_ok && in) ? hrow[j + s] : 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                b[t][s] = (i_ok[t] && in) ? lrow[t][j + s] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[t][s], acc[t], 0, 0, 0);
    }
    // D: column (point) = lane & 15, row (histogram) = kq + 4 * reg
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t i = i0 + t * 16 + r;
        if (i >= n)
            continue;
        const double tl_i = tl[i];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = b0 + kq + 4 * reg;
            if (b < n_hist)
                out[b * ld + i] = acc[t][reg] + tails[b] * tl_i;
        }
    }
}

__global__ __launch_bounds__(256) void batch_fix_dead_kernel(const double *__restrict__ H, const int64_t n_hist,
                                                             const double *__restrict__ L, const int64_t nk,
                                                             const int32_t *__restrict__ dead_list, const int64_t n_dead,
                                                             double *out, const int64_t ld, const int64_t w0)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = w0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
    if (w >= n_hist * n_dead)
        return; // wave-uniform
    const int64_t b = w / n_dead, i = dead_list[w % n_dead];
    const double *hrow = H + b * nk, *lrow = L + i * nk;
    bool hit = false;
    for (int64_t j = lane; j < nk; j += kWave)
        hit = hit || (hrow[j] != 0.0 && is_dead_entry(lrow[j]));
    if (__any(hit) && lane == 0) {
        const double v = out[b * ld + i];
        if (v == v) // (a NaN stays: NaN + -inf is NaN in the reference's sum)
            out[b * ld + i] = -INFINITY;
    }
}

// a wave a request: histogram index[i] against the R rows of point i (value, then the scores), one sweep over the keys.
// R = 1 is the value form: the one row a point of launch_batch_table's table, and tl.
template <int R>
__global__ __launch_bounds__(256) void batch_pairs_kernel(const double *__restrict__ H, const double *__restrict__ tails,
                                                          const int64_t *__restrict__ index, const double *__restrict__ rows,
                                                          const double *__restrict__ tc, const int64_t n, const int64_t nk,
                                                          double *__restrict__ out, const int64_t w0)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = w0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
    if (i >= n)
        return; // wave-uniform
    const int64_t b = index[i];
    const double *hrow = H + b * nk, *lrow = rows + i * R * nk;
    double acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q)
        acc[q] = 0.0;
    bool hit = false;
    for (int64_t j = lane; j < nk; j += kWave) {
        const double h = hrow[j], l = lrow[j];
        acc[0] += h * l;
        hit = hit || (h != 0.0 && is_dead_entry(l));
#pragma unroll
        for (int q = 1; q < R; ++q)
            acc[q] += h * lrow[(int64_t)q * nk + j];
    }
    const double tail = tails[b];
    double v = wave_sum(acc[0]) + tail * tc[i * R];
    if (__any(hit) && v == v)
        v = -INFINITY;
    const bool finite = v - v == 0.0;
    if (lane == 0)
        out[i * R] = v;
#pragma unroll
    for (int q = 1; q < R; ++q) {
        const double g = wave_sum(acc[q]) + tail * tc[i * R + q];
        if (lane == 0)
            out[i * R + q] = finite ? g : NAN;
    }
}

// (R > P + 1: behind the value and the P first-order coefficients the upper triangle of the finishing pass's P x P, k <= l
// row by row)
__global__ __launch_bounds__(256) void batch_tail_pack_kernel(const double *__restrict__ fin_ll,
                                                              const double *__restrict__ fin_grad,
                                                              const double *__restrict__ fin_hess, const int64_t n, const int P,
                                                              const int R, double *__restrict__ tc)
{
    const int64_t total = n * R;
    for (int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = at / R;
        const int q = (int)(at - i * R);
        if (q <= P) {
            tc[at] = q == 0 ? fin_ll[i] : fin_grad[i * P + (q - 1)];
        } else {
            int k = 0, first = 1 + P; // row k of the triangle begins at entry `first` and holds P - k pairs
            while (q >= first + (P - k)) {
                first += P - k;
                ++k;
            }
            tc[at] = fin_hess[(i * P + k) * P + k + (q - first)];
        }
    }
}

__global__ __launch_bounds__(256) void batch_grad_specials_kernel(const int64_t n_hist, const int64_t n, const int R,
                                                                  double *out, const int64_t ld)
{
    const int64_t total = n_hist * n;
    for (int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = at / n, i = at - b * n;
        double *e = out + b * ld + i * R;
        const double v = e[0];
        if (!(v - v == 0.0))
            for (int q = 1; q < R; ++q)
                e[q] = NAN;
    }
}

__global__ void batch_argmin_init_kernel(const int64_t n_hist, double *run_val, int64_t *run_idx)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n_hist) {
        run_val[b] = INFINITY;
        run_idx[b] = -1;
    }
}

__global__ __launch_bounds__(256) void batch_argmin_kernel(const double *__restrict__ ll, const int64_t ld,
                                                           const int64_t n_hist, const int64_t n, const int64_t first,
                                                           double *run_val, int64_t *run_idx, const int64_t w0)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = w0 + (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
    if (b >= n_hist)
        return; // wave-uniform
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX; // none yet (cand.h)
    for (int64_t i = lane; i < n; i += kWave) { // ascending per lane: the first of equal values stays
        const double v = -ll[b * ld + i];
        if (v < c.v) { // (NaN never wins; +inf neither)
            c.v = v;
            c.i = i;
        }
    }
    c = wave_best(c);
    if (lane == 0 && c.i != INT64_MAX && c.v < run_val[b]) { // an earlier chunk keeps a tie: its index is the lower
        run_val[b] = c.v;
        run_idx[b] = first + c.i; // (run_idx stays at the host's -1 while nothing is < +inf)
    }
}

__global__ __launch_bounds__(256) void batch_from_draw_kernel(const int64_t *__restrict__ draw, const int64_t n_hist,
                                                              const int64_t nk, const int has_tail, double *__restrict__ H,
                                                              double *__restrict__ tails)
{
    const int64_t m = nk + (has_tail ? 1 : 0), total = n_hist * m;
    for (int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = at / m, c = at - b * m;
        if (c < nk)
            H[b * nk + c] = (double)draw[at];
        else
            tails[b] = (double)draw[at];
        if (!has_tail && c == 0)
            tails[b] = 0.0;
    }
}

} // namespace

namespace {

// `n` items, one wave each, in launches of at most kWavesPerBlock * kMaxBlocks waves: launch(grid, block, first item)
template <class Launch>
hipError_t launch_waves(int64_t n, Launch launch)
{
    if (n <= 0)
        return hipSuccess;
    const int64_t per_launch = kWavesPerBlock * kMaxBlocks;
    for (int64_t k = 0; k < batch_launch_parts(n, per_launch); ++k) {
        int64_t first, cnt;
        batch_launch_part(n, per_launch, k, &first, &cnt);
        launch(dim3((unsigned)((cnt + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWavesPerBlock * kWave), first);
    }
    return hipGetLastError();
}

// the grid of an elementwise kernel over `total` items: workgroups of 256 threads, each in a grid-stride loop
dim3 elementwise_grid(int64_t total) { return dim3((unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 16)); }

} // namespace

hipError_t launch_batch_table(const DevModel &m, const PointSource &src, int64_t n, double *table, double *tl, int32_t *dead,
                              bool keep_p, hipStream_t stream)
{
    const int P = m.kind == 0 ? 2 : 5;
    return launch_waves(n, [&](dim3 grid, dim3 block, int64_t first) {
        // a part is its own list; n - first bounds it (a part before the last has a wave for each of its points)
        const auto kernel = m.kind == 0 ? batch_table_kernel<2> : batch_table_kernel<5>;
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, m, points_from(src, first, P), n - first, table + first * m.bins.n,
                           tl + first, dead + first, keep_p ? 1 : 0);
    });
}

hipError_t launch_batch_cross(const double *H, const double *tails, int64_t n_hist, const double *table, const double *tl,
                              int64_t n, int64_t n_keys, double *out, int64_t ld, int64_t *tiles, hipStream_t stream)
{
    if (tiles)
        *tiles = 0;
    if (n_hist <= 0 || n <= 0)
        return hipSuccess;
    if (n_hist > kBatchMaxHist)
        return hipErrorInvalidValue;
    const int64_t tiles_y = (n_hist + 15) / 16, gy = batch_cross_groups_y(n_hist), gx = batch_cross_groups_x(n);
    const int64_t x_per = batch_cross_x_per_launch(gy, kMaxBlocks);
    for (int64_t k = 0; k < batch_launch_parts(gx, x_per); ++k) {
        int64_t x0, cnt;
        batch_launch_part(gx, x_per, k, &x0, &cnt);
        hipLaunchKernelGGL(batch_cross_kernel, dim3((unsigned)cnt, (unsigned)gy), dim3(kWavesPerBlock * kWave), 0, stream, H,
                           tails, n_hist, table, tl, n, n_keys, out, ld, x0);
    }
    if (tiles)
        *tiles = tiles_y * ((n + 15) / 16);
    return hipGetLastError();
}

hipError_t launch_batch_fix_dead(const double *H, int64_t n_hist, const double *table, int64_t n_keys,
                                 const int32_t *dead_list, int64_t n_dead, double *out, int64_t ld, hipStream_t stream)
{
    return launch_waves(n_hist * n_dead, [&](dim3 grid, dim3 block, int64_t w0) {
        hipLaunchKernelGGL(batch_fix_dead_kernel, grid, block, 0, stream, H, n_hist, table, n_keys, dead_list, n_dead, out, ld, w0);
    });
}

hipError_t launch_batch_pairs(const double *H, const double *tails, const int64_t *index, const double *rows,
                              const double *tc, int64_t n, int64_t n_keys, int rows_per_point, double *out, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    const auto kernel = rows_per_point == 1   ? batch_pairs_kernel<1>
                        : rows_per_point == 3 ? batch_pairs_kernel<3>
                        : rows_per_point == 6 ? batch_pairs_kernel<6>
                        : rows_per_point == 21 ? batch_pairs_kernel<21>
                                               : nullptr;
    if (!kernel)
        return hipErrorInvalidValue;
    return launch_waves(n, [&](dim3 grid, dim3 block, int64_t w0) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, H, tails, index, rows, tc, n, n_keys, out, w0);
    });
}

hipError_t launch_batch_tail_pack(const double *fin_ll, const double *fin_grad, const double *fin_hess, int64_t n, int n_par,
                                  int rows_per_point, double *tc, hipStream_t stream)
{
    const int64_t total = n * rows_per_point;
    if (total <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(batch_tail_pack_kernel, elementwise_grid(total), dim3(256), 0, stream, fin_ll, fin_grad, fin_hess, n,
                       n_par, rows_per_point, tc);
    return hipGetLastError();
}

hipError_t launch_batch_grad_specials(int64_t n_hist, int64_t n, int rows_per_point, double *out, int64_t ld,
                                      hipStream_t stream)
{
    const int64_t total = n_hist * n;
    if (total <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(batch_grad_specials_kernel, elementwise_grid(total), dim3(256), 0, stream, n_hist, n, rows_per_point,
                       out, ld);
    return hipGetLastError();
}

hipError_t launch_batch_argmin_init(int64_t n_hist, double *run_val, int64_t *run_idx, hipStream_t stream)
{
    if (n_hist <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(batch_argmin_init_kernel, dim3((unsigned)((n_hist + 255) / 256)), dim3(256), 0, stream, n_hist,
                       run_val, run_idx);
    return hipGetLastError();
}

hipError_t launch_batch_argmin(const double *ll, int64_t ld, int64_t n_hist, int64_t n, int64_t first, double *run_val,
                               int64_t *run_idx, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    return launch_waves(n_hist, [&](dim3 grid, dim3 block, int64_t w0) {
        hipLaunchKernelGGL(batch_argmin_kernel, grid, block, 0, stream, ll, ld, n_hist, n, first, run_val, run_idx, w0);
    });
}

hipError_t launch_batch_from_draw(const int64_t *draw, int64_t n_hist, int64_t n_keys, bool has_tail, double *H,
                                  double *tails, hipStream_t stream)
{
    const int64_t total = n_hist * (n_keys + (has_tail ? 1 : 0));
    if (total <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(batch_from_draw_kernel, elementwise_grid(total), dim3(256), 0, stream, draw, n_hist, n_keys,
                       has_tail ? 1 : 0, H, tails);
    return hipGetLastError();
}

} // namespace covest
