// tp_eval.hip -- K-tp: the truncated-Poisson pmf itself, value by value (covest_truncated_poisson,
// covest_truncated_poisson_table).
//
// Every likelihood kernel rests on the reference's covest_poisson.truncated_poisson(l, j)
// (c_src/covest_poissonmodule.c:7-35).  The library evaluates it by two routes, and each has a kernel here that
// shows it on its own -- with the arithmetic of the headers the likelihood kernels include, none of it restated:
//   tp_pairs_kernel   term by term, K-direct's expressions in K-direct's order (direct_point.h): lx = log(x),
//                     nd = -log_trunc_norm(x, lx), exp(fma(j, lx, nd - ln j!)); ln j! from the host's table
//   tp_table_kernel   the recurrence K-basic and K-factored walk (streams.h): one stream per lane with a = 1,
//                     c = -D(x), anchored by enter_tile and advanced by one multiply a key along the tiles the host
//                     cuts from the key list (tiles.h, tiles_host.cpp), the per-key factor from the tile table
// Neither launch is entered in the launch records or in covest_compiled_variants.
#include <hip/hip_runtime.h>

#include "direct_point.h"
#include "kernels.h"
#include "streams.h"

namespace covest {

namespace {

// Where the extension's running long-double product passes LDBL_MAX (direct_point.h REF_OVF, restated: there the rule
// is spread over a component's preparation and the bins' loop).  prod_{i <= j} (x / i) grows until i = floor(x), so
// its largest value is x^m / m! at m = min(j, floor(x)); lgam_m = ln m! (host table).
__device__ __forceinline__ bool reference_product_overflows(double x, double lx, double m, double lgam_m)
{
    return x >= 1.0 && fma(m, lx, -lgam_m) > kLnLdblMax;
}

// in: [4][n] = rate | key j as a double | ln j! | ln m!, m = min(j, floor(rate)) (0 where rate < 1); out[n]
template <int MODE>
__global__ __launch_bounds__(256) void tp_pairs_kernel(const int64_t n, const double *__restrict__ in,
                                                       double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const double x = in[i], key = in[n + i], lgam = in[2 * n + i];
    // x == 0 or NaN: the extension returns 0 (c_src/covest_poissonmodule.c:15); a negative rate is no rate, and is
    // treated as K-direct treats it (direct_point.h: `x > 0.0`, else the component contributes exactly 0)
    double r = MODE == kTpLog ? -INFINITY : 0.0;
    if (x > 0.0) {
        const double lx = log(x);
        const double nd = -log_trunc_norm(x, lx);
        const double a = fma(key, lx, nd - lgam);
        if (MODE == kTpLog) {
            r = a;
        } else {
            r = exp(a);
            if (MODE == kTpReference && reference_product_overflows(x, lx, fmin(key, floor(x)), in[3 * n + i]))
                r = INFINITY;
        }
    }
    out[i] = r;
}

constexpr int kTableLanes = kWave;          // rates per workgroup, one a lane
constexpr int kTableLd = kTableLanes + 1;   // a staged key row, padded: the transposed reads are conflict-free

// out[n_l][n_j] row-major.  A workgroup is one wave; lane = rate.  A tile's values are staged in LDS as
// [key row][rate] and written out transposed -- lane = (rate, key), a half wave the tile's keys of one rate -- so the
// stores run along the keys of a rate, which is how the output lies in memory: 32 consecutive doubles of one row of
// `out` where the tile holds 32 keys of consecutive index, fewer for a short tile or one with filler keys.
__global__ __launch_bounds__(kTableLanes) void tp_table_kernel(const int n_l, const double *__restrict__ rates, const int n_j,
                                                              const int32_t n_tiles, const int32_t n_items,
                                                              const double *__restrict__ tile_dbl,
                                                              const int32_t *__restrict__ tile_int, double *__restrict__ out)
{
    __shared__ double stage[kTileBins * kTableLd];
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    const int lane = threadIdx.x;
    const int64_t first_rate = (int64_t)blockIdx.x * kTableLanes;
    const int64_t mine = first_rate + lane;
    const double x = mine < n_l ? rates[mine] : 0.0;

    StreamSet<1> st; // comb = 1: a = 1, c = ln a - D(x) = -D(x)
    st.gone = 0u;
    st.v[0] = 0.0;
    if (x > 0.0) {
        const double lx = log(x);
        st.x[0] = x;
        st.an.set(0, lx, -log_trunc_norm(x, lx));
    } else { // contributes exactly 0, as in StreamSet::init
        st.x[0] = 0.0;
        st.an.set(0, 0.0, -INFINITY);
    }

    for (int t = 0; t < tv.n_tiles; ++t) {
        const TileRec rc = tv.rec[t];
        const int nb = rc.nb;
        st.enter_tile(rc.k0 - 1.0, rc.k0 + (double)(nb - 1), rc.lgam_prev, rc.lgam_last, rc.run_start != 0);
        const double *scal = tv.scal + (int64_t)t * kTileBins;
        // the key's scale carries 2^kBasicShift (tiles.h): the product is rounded as a normal double, and onto the
        // doubles' own grid by the exact power of two behind it
        for (int b = 0; b < nb; ++b)
            stage[b * kTableLd + lane] = (st.step() * scal[b]) * (1.0 / kBasicScale);
        st.leave_tile(rc.renorm);
        __syncthreads();
        const int32_t *row_bin = tv.row_bin + (int64_t)t * kTileBins;
        const int b = lane % kTileBins;
        const int col = b < nb ? row_bin[b] : -1; // (-1: a filler key of a bridged gap, or padding)
        for (int r = lane / kTileBins; r < kTableLanes; r += kTableLanes / kTileBins) {
            const int64_t rate = first_rate + r;
            if (col >= 0 && col < n_j && rate < n_l)
                out[rate * n_j + col] = stage[b * kTableLd + r];
        }
        __syncthreads();
    }
}

} // namespace

hipError_t launch_tp_pairs(int mode, int64_t n, const double *in, double *out, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    if (n > kTpMaxPairs) // (HIP wraps a grid of more than 2^32 threads silently; the entry point refuses longer lists)
        return hipErrorInvalidValue;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    if (mode == kTpValue)
        hipLaunchKernelGGL((tp_pairs_kernel<kTpValue>), grid, block, 0, stream, n, in, out);
    else if (mode == kTpReference)
        hipLaunchKernelGGL((tp_pairs_kernel<kTpReference>), grid, block, 0, stream, n, in, out);
    else if (mode == kTpLog)
        hipLaunchKernelGGL((tp_pairs_kernel<kTpLog>), grid, block, 0, stream, n, in, out);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_tp_table(const TileView &tv, int64_t n_l, const double *rates, int64_t n_j, double *out,
                           hipStream_t stream)
{
    if (n_l <= 0 || n_j <= 0)
        return hipSuccess;
    if (n_l > (int64_t)1 << 30 || n_j > (int64_t)1 << 20)
        return hipErrorInvalidValue;
    const dim3 block(kTableLanes), grid((unsigned)((n_l + kTableLanes - 1) / kTableLanes));
    hipLaunchKernelGGL(tp_table_kernel, grid, block, 0, stream, (int)n_l, rates, (int)n_j, tv.n_tiles, tv.n_items, tv.dbl_base,
                       tv.int_base, out);
    return hipGetLastError();
}

} // namespace covest
