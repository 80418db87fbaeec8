// ll_factored_launch.hip -- K-factored's common translation unit: the finishing kernels of the chunked shapes (tiles.h
// list modes 2 and 3), the proof of the LDS layout, and the dispatcher that picks a variant of ll_factored.hip's kernel
// from the table of factored_launch.h.  The variants are linked in, one translation unit each.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "direct_point.h" // strict_pj_wave, for finish_point
#include "factored_launch.h"
#include "handback.h"
#include "kernels.h"
#include "point_fetch.h"
#include "wave.h"

namespace covest {

const char *const kFactoredFinishNames[2] = {"ll_finish_dense", "ll_finish_partials"};

namespace {

// One wave finishes ONE point whose p_j lie in HBM, summed over chunks of copy numbers (tiles.h list modes 2, 3):
// LL = sum_j h_j log p_j + tail log(1 - sp), covest/models.py:100-107.  read_pj(row): the p_j of row `row` of the
// items (tiles.h: a key, or the sum over a count-less tile), TIMES kShareScale.  A subnormal p_j at a key with h_j != 0
// -- down to kZeroSteps of a grid step, below which it is 0 in the reference whatever the roundings (handback.h) -- is
// replaced on the spot by its strict evaluation (direct_point.h: the whole wave, K-direct's arithmetic).  par: the
// point's parameters, clamped; every lane returns the value.
template <class ReadPj>
__device__ __forceinline__ double finish_point(const DevModel &m, const TileView &tv, const double *par, int T,
                                               ReadPj read_pj)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_rows = (int64_t)tv.n_items * kTileBins;
    double ll = 0.0;
    bool dead = false, poisoned = false;
    CompSum sp = {0.0, 0.0};
    for (int64_t base = 0; base < n_rows; base += kWave) { // wave-uniform trip count
        const int64_t row = base + lane;
        const bool valid = row < n_rows;
        const double pj_scaled = valid ? read_pj(row) : 0.0;
        double pj = pj_scaled * (1.0 / kShareScale); // (one rounding, onto the doubles' grid)
        const double h = valid ? tv.item_cnt[row] : 0.0;
        uint64_t sub = __ballot(h != 0.0 && pj_scaled > zero_steps_scaled(kShareScale) &&
                                pj < 2.2250738585072014e-308); // a subnormal p_j, or one the product above flushed
        while (sub) { // wave-uniform, rare
            const int who = __builtin_ctzll(sub);
            sub &= sub - 1;
            const int64_t r = base + who;
            const int item = (int)(r / kTileBins);
            const int bin = tv.row_bin[(int64_t)tv.item_first[item] * kTileBins + (r - (int64_t)item * kTileBins)];
            const double strict = strict_pj_wave<5>(m, par, T, m.bins.key[bin], -m.bins.lgam[bin]);
            if (lane == who)
                pj = strict;
        }
        if (m.tail != 0.0)
            sp.add(pj);
        if (h != 0.0) {
            dead |= pj <= 0.0; // utils.safe_log
            poisoned |= pj != pj; // a NaN parameter: NaN, as in the reference (math.log(nan))
            ll = fma(h, log(pj > 0.0 ? pj : 1.0), ll);
        }
    }
    ll = wave_sum(ll);
    double tail_term = 0.0;
    if (m.tail != 0.0) {
        double s = wave_comp_sum(sp);
        if (!(s < 1.0))
            s = 1.0;
        if (s < 1.0)
            tail_term = m.tail * log(1.0 - s);
    }
    if (__ballot(dead))
        ll = isnan(ll) ? ll : -INFINITY;
    double v = ll + tail_term;
    if (__ballot(poisoned) || !(isfinite(par[0]) && isfinite(par[1])))
        v = NAN;
    return v;
}

// Chunked point list (tiles.h list_mode 2): one wave per point adds the chunks' shares of p_j in chunk order and
// takes the logs.  point_par[5 n_points], point_T[n_points]: the points' parameters and threshold_o.
__global__ __launch_bounds__(kWave) void ll_finish_partials(const DevModel m, const int32_t n_tiles, const int32_t n_items,
                                                           const double *__restrict__ tile_dbl,
                                                           const int32_t *__restrict__ tile_int,
                                                           const double *__restrict__ partial,
                                                           const int32_t *__restrict__ first_item,
                                                           const double *__restrict__ point_par,
                                                           const int32_t *__restrict__ point_T, double *__restrict__ out_ll)
{
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    const int p = blockIdx.x;
    const int c0 = first_item[p], c1 = first_item[p + 1];
    const int64_t n_rows = (int64_t)n_items * kTileBins;
    double par[kMaxParams];
#pragma unroll
    for (int d = 0; d < kMaxParams; ++d)
        par[d] = point_par[(int64_t)p * kMaxParams + d];
    clamp_point<5>(m, par);
    const double v = finish_point(m, tv, par, point_T[p], [&](int64_t row) {
        double pj = 0.0;
        for (int c = c0; c < c1; ++c)
            pj += partial[(int64_t)c * n_rows + row];
        return pj;
    });
    if (threadIdx.x == 0)
        out_ll[p] = v;
}

// The long weight vectors of a dense grid (tiles.h list_mode 3: threshold_o beyond a workgroup's lanes): one wave
// per ((c, e), slot) takes the logs of the p_j the chunk launches summed into `partial`.
__global__ __launch_bounds__(kWave) void ll_finish_dense(const DevModel m, const int32_t n_tiles, const int32_t n_items,
                                                        const double *__restrict__ tile_dbl,
                                                        const int32_t *__restrict__ tile_int, const PointSource src,
                                                        const double *__restrict__ partial, const int64_t ce_first,
                                                        const int64_t n_cols, const int32_t *__restrict__ q_orig,
                                                        const int64_t n_q, const int64_t flat_end,
                                                        double *__restrict__ out_ll)
{
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    const int64_t ce_local = blockIdx.x / n_cols, slot = blockIdx.x - ce_local * n_cols;
    const int32_t qo = q_orig[slot];
    if (qo < 0)
        return; // padding column
    const int64_t flat = (ce_first + ce_local) * n_q + qo;
    if (flat < src.flat_begin || flat >= flat_end)
        return; // (ragged block ends)
    double par[kMaxParams];
    int T;
    fetch_point<5>(src, flat - src.flat_begin, par, T);
    clamp_point<5>(m, par);
    const int64_t n_rows = (int64_t)n_items * kTileBins;
    const double *mine = partial + (ce_local * n_cols + slot) * n_rows;
    const double v = finish_point(m, tv, par, T, [&](int64_t row) { return mine[row]; });
    if (threadIdx.x == 0)
        out_ll[flat - src.flat_begin] = v;
}

// The layout of tiles.h FactoredLds over the shapes the planners make (row strides 34 .. 546, both workgroup sizes, one
// and two buffers, with and without SPO, both parities of the walk's length): every area inside the allocation, the SPO
// parts clear of what the last interval still reads -- the buffer it contracts (one buffer: the two rows of S in it) --
// and of the slack, part_ll clear of part_hi / part_lo, and the allocation within the CU's LDS wherever the planners
// choose that n_buf.
constexpr bool lds_overlap(int a0, int a1, int b0, int b1) { return a0 < b1 && b0 < a1; }
constexpr bool factored_lds_sound()
{
    for (int nt = 256; nt <= 512; nt += 256)
        for (int n_buf = 1; n_buf <= 2; ++n_buf)
            for (int k = 1; k <= 17; ++k)
                for (int spo = 0; spo <= 1; ++spo)
                    for (int t_end = 1; t_end <= 2; ++t_end) {
                        const FactoredLds l{nt, n_buf, kTileBins * k + 2, spo != 0};
                        const int ne = l.entries(), total = l.total();
                        if (l.buf(n_buf - 1) + kTileBins * l.ld > l.slack() || l.slack() + FactoredLds::kSlack > total ||
                            l.rates() + FactoredLds::kRates > total || l.pad(l.rows() - 1) + 2 > l.slack())
                            return false;
                        if (l.part_ll() + ne > total || l.part_hi(t_end) + ne > total || l.part_lo(t_end) + ne > total ||
                            lds_overlap(l.part_ll(), l.part_ll() + ne, l.part_hi(t_end), l.part_lo(t_end) + ne))
                            return false;
                        if (spo) {
                            const int s0 = l.spo_parts(t_end), s1 = s0 + 2 * ne, live = l.buf(t_end);
                            if (s1 > total || lds_overlap(s0, s1, l.slack(), l.slack() + FactoredLds::kSlack) ||
                                lds_overlap(s0, s1, live, live + (n_buf == 2 ? kTileBins : 2) * l.ld))
                                return false;
                            const int other = l.buf(t_end + 1);
                            if (n_buf == 2 && s0 < l.slack() && (s0 < other || s1 > other + kTileBins * l.ld))
                                return false;
                        }
                        if (factored_n_buf(l.ld) == n_buf && !l.fits())
                            return false;
                    }
    return true;
}
static_assert(factored_lds_sound(), "K-factored's LDS layout (tiles.h FactoredLds)");
// the headline shape (C3: 512 threads, plain, no tail, kLdWide) allocates two buffers and the slack, as it always has
static_assert(FactoredLds{512, 2, kLdWide, false}.total() == 2 * kTileBins * kLdWide + FactoredLds::kSlack, "C3's LDS");

// row v of the table and up: the launcher of variant number v
template <int V = 0>
hipError_t launch_variant(int v, const DevModel &m, const TileView &tv, const FactoredPlan &plan, double *out_ll,
                          const SubList &sub_list, hipStream_t stream)
{
    if constexpr (V < kFactoredVariants)
        return v == V ? launch_ll_factored_variant<V>(m, tv, plan, out_ll, sub_list, stream)
                      : launch_variant<V + 1>(v, m, tv, plan, out_ll, sub_list, stream);
    return hipErrorInvalidValue;
}

} // namespace

hipError_t launch_ll_finish_partials(const DevModel &m, const TileView &tv, const double *partial,
                                     const int32_t *first_item, const double *point_par, const int32_t *point_T,
                                     int64_t n_points, double *out_ll, hipStream_t stream)
{
    if (n_points <= 0)
        return hipSuccess;
    record_launch(kFactoredFinishNames[1]);
    hipLaunchKernelGGL(ll_finish_partials, dim3((unsigned)n_points), dim3(kWave), 0, stream, m, tv.n_tiles, tv.n_items, tv.dbl_base,
                       tv.int_base, partial, first_item, point_par, point_T, out_ll);
    return hipGetLastError();
}

hipError_t launch_ll_finish_dense(const DevModel &m, const TileView &tv, const PointSource &src, const double *partial,
                                  int64_t ce_first, int64_t n_ce, int64_t n_cols, const int32_t *q_orig, int64_t n_q,
                                  int64_t flat_end, double *out_ll, hipStream_t stream)
{
    // HIP wraps a grid of more than 2^32 threads silently: at most 2^24 waves per launch
    const int64_t per_launch = std::max<int64_t>(1, ((int64_t)1 << 24) / n_cols);
    for (int64_t first = 0; first < n_ce; first += per_launch) {
        const int64_t cnt = std::min(per_launch, n_ce - first);
        record_launch(kFactoredFinishNames[0]);
        hipLaunchKernelGGL(ll_finish_dense, dim3((unsigned)(cnt * n_cols)), dim3(kWave), 0, stream, m, tv.n_tiles, tv.n_items,
                           tv.dbl_base, tv.int_base, src, partial + first * n_cols * (int64_t)tv.n_items * kTileBins,
                           ce_first + first, n_cols, q_orig, n_q, flat_end, out_ll);
    }
    return hipGetLastError();
}

hipError_t launch_ll_factored(const DevModel &m, const TileView &tv, const FactoredPlan &plan,
                              double *out_ll, const SubList &sub_list, hipStream_t stream)
{
    if (plan.ce_end <= plan.ce_begin)
        return hipSuccess;
    if (m.kind != 1 || plan.n_columns > plan.n_threads || 8 * plan.n_pass < m.n_err || plan.half_units != kHalfUnits)
        return hipErrorInvalidValue;
    const bool plain = plan.list_mode == 0 && plan.n_pass == 1;
    const int v = factored_variant_of(plan.n_threads, m.tail != 0.0, plain, plan.ld);
    if (v < 0)
        return hipErrorInvalidValue;
    const int64_t rows = plan.ce_end - plan.ce_begin, per_launch = factored_rows_per_launch(plan);
    record_launch(kFactoredVariantTable[v].name, (rows + per_launch - 1) / per_launch);
    return launch_variant(v, m, tv, plan, out_ll, sub_list, stream);
}

} // namespace covest
