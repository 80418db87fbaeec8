// posterior.hip -- K-post: the posterior shares of error classes and copy numbers per key, in the log domain
// (covest_posterior_classes; posterior.h has the definitions).
//
// The shares are the terms of the sum compute_probabilities adds up (covest/models.py:92-97, :235-241) before they are
// added, each over the total.  They are formed from logs from the start: ln w_os(j) = w + j * lx - ln j! per component,
// the maximum over the components taken off before any exp, so that a share exists where p_j itself is a subnormal
// double or 0.  a_os, b_o, ln x and -D(x) are prepare_mix_lot's (mix_lot.h, LibmMath: K-direct's doubles); a class whose
// 1.0 - exp(-x) is 0 in double has weight 0 in the likelihood that was fitted, and share exactly 0 here.
//
// Stage 1 (posterior_table_kernel): a point's components into a table in HBM, 16 bytes each -- (T - 1) * S of them, 350 KB
//   at T = 1000, S = 22: beyond LDS; every wave of stage 2 reads it at wave-uniform addresses, out of L2.
// Stage 2 (posterior_walk_kernel): a lane owns a key.  One walk for the maximum; one class-major, one accumulator, a
//   class's sum staged when the class ends; one copy-major, one accumulator per column in flight and the mean beside it.
//   Sums go through LDS in groups of kPostGroup columns and are stored along the rows of the output, then divided by the
//   family's own total by the thread that stored them.  No register array is indexed at run time; no workgroup waits for
//   another.
#include <hip/hip_runtime.h>

#include "mix_lot.h"
#include "point_fetch.h"
#include "posterior.h"
#include "wave.h"

namespace covest {

namespace {

constexpr int kPostKeys = kWave;            // keys per workgroup, one a lane (one wave)
constexpr int kPostGroup = 16;              // columns of a family staged in LDS at a time
constexpr int kPostLd = kPostGroup + 1;     // a key's staged row, padded

template <int P>
__global__ __launch_bounds__(kWave) void posterior_table_kernel(const DevModel m, const PointSource src, const int64_t stride,
                                                                PostComp *__restrict__ table)
{
    const int lane = threadIdx.x;
    const int64_t pt = blockIdx.y;
    double par[kMaxParams];
    int T;
    fetch_point<P>(src, pt, par, T);
    clamp_point<P>(m, par);
    const int S = m.n_err;
    const int OT = kWave / S; // copy numbers of a lot
    const int o0 = 1 + (int)blockIdx.x * OT;
    if (o0 >= T)
        return; // wave-uniform: the grid is sized for the list's largest threshold_o
    const int s = lane % S;
    const int og = lane / S;
    const int o = o0 + og;
    const bool live = og < OT && o < T;
    const double lam = error_class_rate(m, par[0], par[1], s);
    MixLot c;
    prepare_mix_lot<P>(LibmMath{}, par, m.comb[s], (double)o * lam, live, o, og * S, S, c);
    if (live) {
        PostComp e;
        e.lx = c.lx;
        e.w = -INFINITY; // a_os b_o = 0 or x_os = 0: the component weighs nothing
        if (c.a != 0.0 && c.b != 0.0 && c.nd != -INFINITY)
            e.w = (log(c.b) + log(c.a)) + c.nd;
        table[pt * stride + (int64_t)(o - 1) * S + s] = e;
    }
}

// The group of columns [g0, g0 + gw) of the workgroup's kPostKeys rows, from LDS (stage[key][column of the group]) to
// rows[key * row_len + column]: consecutive threads store consecutive columns of a row.  Thread `lane` stores the
// elements i = lane, lane + kPostKeys, ... of the group's block, i = key * gw + column: scale_group below walks the same
// elements with the same thread, so it reads back its own stores.
__device__ __forceinline__ void store_group(const double *stage, double *rows, int64_t row_len, int g0, int gw, int n_rows,
                                            int lane)
{
    __syncthreads();
    for (int i = lane; i < kPostKeys * gw; i += kPostKeys) {
        const int r = i / gw, c = i - r * gw;
        if (r < n_rows)
            rows[(int64_t)r * row_len + g0 + c] = stage[r * kPostLd + c];
    }
    __syncthreads();
}

// Every stored sum over its row's total (tot[key], in LDS): a family is normalised by its own total.
__device__ __forceinline__ void scale_groups(const double *tot, double *rows, int64_t row_len, int n_cols, int n_rows, int lane)
{
    for (int g0 = 0; g0 < n_cols; g0 += kPostGroup) {
        const int gw = min(kPostGroup, n_cols - g0);
        for (int i = lane; i < kPostKeys * gw; i += kPostKeys) {
            const int r = i / gw, c = i - r * gw;
            if (r < n_rows) {
                double *p = rows + (int64_t)r * row_len + g0 + c;
                *p = *p / tot[r];
            }
        }
    }
}

__global__ __launch_bounds__(kPostKeys) void posterior_walk_kernel(const BinView bins, const int S, const int32_t *__restrict__ t_list,
                                                                   const int64_t stride, const PostComp *__restrict__ table,
                                                                   const int copy_columns, const int live, const PostOut out)
{
    __shared__ double stage[kPostKeys * kPostLd];
    __shared__ double tot_row[kPostKeys];
    const int lane = threadIdx.x;
    const int64_t pt = blockIdx.y;
    const int64_t n_keys = bins.n;
    const int64_t first = (int64_t)blockIdx.x * kPostKeys;
    const int64_t idx = first + lane;
    const bool mine = idx < n_keys;
    const int n_rows = (int)(n_keys - first < kPostKeys ? n_keys - first : kPostKeys);
    const double key = mine ? bins.key[idx] : 1.0; // (a lane beyond the keys walks along and stores nothing)
    const double lgam = mine ? bins.lgam[idx] : 0.0;
    const int T = t_list ? t_list[pt] : 2; // wave-uniform
    const int n_o = T > 1 ? T - 1 : 0;
    const PostComp *__restrict__ tab = table + pt * stride;

    // ---- the maximum of ln w_os(j) + ln j! over the components
    double mx = -INFINITY;
    for (int i = 0; i < n_o * S; ++i) {
        const PostComp e = tab[i];
        mx = fmax(mx, fma(key, e.lx, e.w));
    }

    // ---- class-major: E_s, and ln p_j from the family's total
    double tot = 0.0;
    double *err_rows = out.err ? out.err + (pt * n_keys + first) * S : nullptr;
    for (int g0 = 0; g0 < S; g0 += kPostGroup) {
        const int gw = min(kPostGroup, S - g0);
        for (int c = 0; c < gw; ++c) {
            const PostComp *__restrict__ col = tab + (g0 + c);
            double acc = 0.0;
            for (int o = 0; o < n_o; ++o) {
                const PostComp e = col[(int64_t)o * S];
                acc += exp(fma(key, e.lx, e.w) - mx);
            }
            tot += acc;
            stage[lane * kPostLd + c] = acc;
        }
        if (err_rows)
            store_group(stage, err_rows, S, g0, gw, n_rows, lane);
    }
    if (mine) // (no component with weight: no posterior exists, ln p_j = -inf and the shares are 0 / 0)
        out.log_p[pt * n_keys + idx] = mx == -INFINITY ? -INFINITY : (mx + log(tot)) - lgam;
    if (err_rows) {
        tot_row[lane] = tot;
        __syncthreads();
        scale_groups(tot_row, err_rows, S, S, n_rows, lane);
        __syncthreads();
    }

    // ---- copy-major: column c < copy_columns - 1 is o = c + 1, the last column everything from o = copy_columns on
    if (!out.copy && !out.mean)
        return; // (uniform over the launch)
    // (the columns are divided by the sum of the columns as they are stored, so a row sums to 1 within half an ulp a
    // column however many copy numbers the last one holds; the mean by the sum copy number by copy number, so it is the
    // same bytes at every copy_columns)
    double tot_c = 0.0, tot_o = 0.0, mean = 0.0;
    double *copy_rows = out.copy ? out.copy + (pt * n_keys + first) * live : nullptr;
    for (int g0 = 0; g0 < live; g0 += kPostGroup) {
        const int gw = min(kPostGroup, live - g0);
        for (int c = 0; c < gw; ++c) {
            const int column = g0 + c;
            const int o_end = column < copy_columns - 1 ? min(column + 2, T) : T; // (exclusive)
            double col_acc = 0.0;
            for (int o = column + 1; o < o_end; ++o) {
                const PostComp *__restrict__ row = tab + (int64_t)(o - 1) * S;
                double acc = 0.0;
                for (int s = 0; s < S; ++s) {
                    const PostComp e = row[s];
                    acc += exp(fma(key, e.lx, e.w) - mx);
                }
                col_acc += acc;
                tot_o += acc;
                mean += (double)o * acc;
            }
            tot_c += col_acc;
            stage[lane * kPostLd + c] = col_acc;
        }
        if (copy_rows)
            store_group(stage, copy_rows, live, g0, gw, n_rows, lane);
    }
    if (out.mean && mine)
        out.mean[pt * n_keys + idx] = mean / tot_o;
    if (copy_rows) {
        tot_row[lane] = tot_c;
        __syncthreads();
        scale_groups(tot_row, copy_rows, live, live, n_rows, lane);
    }
}

} // namespace

hipError_t launch_posterior_table(const DevModel &m, const PointSource &src, int64_t n, int t_max, int64_t stride,
                                  PostComp *table, hipStream_t stream)
{
    if (n <= 0 || t_max < 2)
        return hipSuccess;
    const int S = m.n_err;
    if (n > 65535 || S < 1 || S > kWave || stride < (int64_t)(t_max - 1) * S)
        return hipErrorInvalidValue;
    const int OT = kWave / S;
    const dim3 block(kWave), grid((unsigned)((t_max - 1 + OT - 1) / OT), (unsigned)n);
    if (m.kind == 0)
        hipLaunchKernelGGL((posterior_table_kernel<2>), grid, block, 0, stream, m, src, stride, table);
    else
        hipLaunchKernelGGL((posterior_table_kernel<5>), grid, block, 0, stream, m, src, stride, table);
    return hipGetLastError();
}

hipError_t launch_posterior_walk(const DevModel &m, const int32_t *t_list, int64_t n, int64_t stride, const PostComp *table,
                                 int copy_columns, int live, const PostOut &out, hipStream_t stream)
{
    if (n <= 0 || m.bins.n <= 0)
        return hipSuccess;
    const int S = m.n_err;
    if (n > 65535 || S < 1 || S > kWave || copy_columns < 1 || live < 1 || live > copy_columns || !out.log_p ||
        m.bins.n > ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    const dim3 block(kPostKeys), grid((unsigned)((m.bins.n + kPostKeys - 1) / kPostKeys), (unsigned)n);
    hipLaunchKernelGGL(posterior_walk_kernel, grid, block, 0, stream, m.bins, S, t_list, stride, table, copy_columns, live, out);
    return hipGetLastError();
}

} // namespace covest
