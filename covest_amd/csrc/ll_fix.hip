// ll_fix.hip -- K-fix: the pass that patches the points a recurrence kernel handed back (handback.h), by the strict,
// term-by-term evaluation of the rows they named (mix_lot.h: K-direct's arithmetic).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fastmath.h"
#include "handback.h"
#include "kernels.h"
#include "mix_lot.h"
#include "point_fetch.h"
#include "wave.h"

namespace covest {

namespace {

// The hand-back of the recurrence kernels (handback.h): the queued points' values are corrected in place.
// `fast` (the recurrence kernel's value, in which every p_j below p_clamp counted as p_clamp) gets, for every counted
// row of the range named in the side word whose STRICT p_j is below p_clamp, h_j (safe_log(p_j) - log(p_clamp)) added,
// in ascending row order.  The strict p_j is K-direct's (direct_point.h) to the letter: LANE r of a wave keeps the
// p_j of row r of a 64-row chunk; the mixture components are prepared 64 at a time (one per lane) and broadcast
// through the scalar unit, every term rounded to a double on its own, error classes inside, copy numbers outside, both
// ascending.  A point takes ONE wave, four points a workgroup, and nothing inside the loop over the queue synchronises
// the workgroup.  (Until round 5 a repeats-model point was shared by the 4 waves of a workgroup: lots of copy numbers
// dealt to them in turn, the partial p_j added through LDS.  But the points that are handed back are the
// ones whose LAST keys underflow, which are the ones with a SMALL threshold_o -- three to six lots, most of them out
// of the rows' reach -- and every one of the four waves repeated the point's loads, its two pows and the rows' bins:
// C3's 2 962 queued points 46.8 us with four waves a point, 35.8 us with one, profiles/r05_c3_kstat_fix_one_wave_a_point.txt.)
// Launched after every K-basic / K-factored launch, before anything reads the values -- a grid handle's plain evaluation
// puts it off until somebody does (abi_grid.cpp grid_complete: the arg-min needs no more than the bound that a queued
// point's value only falls here); with an empty queue it costs a launch and one load.  The queued points of a wide
// grid come in clusters (whole (c, e) rows of it) and the work of one grows with its threshold_o, which is why they are compacted into a queue and spread over the chip instead
// of being patched by whichever thread meets them.  The queue's counter is reset by whoever runs next on the
// stream: the arg-min pass (grids; it leaves the queue's length in the word behind the counter, which is the `count` of
// a pass that was put off) or the host (point lists).
// (Measured and not kept, round 5: the kernel held to 96 registers for five waves a SIMD -- it takes 155, three waves --
// spills 27 of them and is slower, 42.9 against 35.8 us on C3's 2 962 queued points (threshold_o 11 .. 87, 27 rows
// each); to 128 for four waves, 36.4.  The launch is one trip of every wave: by the counters a point is 2 750 vector
// instructions at 17 cycles apiece -- the two pows of its rates, the preparation of the one or two lots of copy numbers
// that reach its rows, an exp per component kept -- profiles/r05_c3_kstat_fix_occupancy_not_kept.txt.)
template <int P>
__global__ __launch_bounds__(256) void ll_fix_list_kernel(const DevModel m, const int32_t n_tiles, const int32_t n_items,
                                                          const double *__restrict__ tile_dbl,
                                                          const int32_t *__restrict__ tile_int, const PointSource src,
                                                          double *__restrict__ ll, const SubList list)
{
    constexpr int PPB = 4; // points per workgroup: one a wave
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const unsigned count = __builtin_amdgcn_readfirstlane(*list.count);
    if (count == 0)
        return; // (workgroup-uniform) the common case: a launch and one load
    // (round 4) the preparation of a lot -- ln x, the normaliser's two logs, the copy number's weight -- was most of this
    // kernel: the device library's log (72 issue slots) three times and its pow (210) once per component.  The logs go
    // through the fast_log table (absolute error 2e-16, what the recurrence kernels' anchors are made with), the weight
    // by squaring.
    __shared__ __attribute__((aligned(16))) double log_tab[kLogTableDoubles];
    load_log_table(log_tab);
    __syncthreads();
    const int S = m.n_err;
    const int OT = kWave / S; // copy numbers prepared per lot of 64 components
    const int s = lane % S;
    const int og = lane / S;
    const bool lane_in_tile = og < OT;
    const double comb_s = m.comb[s];
    for (unsigned at0 = blockIdx.x * PPB; at0 < count; at0 += gridDim.x * PPB) { // workgroup-uniform
        const unsigned at = at0 + wave_in_block;
        if (at >= count)
            continue; // (wave-uniform; nothing below synchronises the workgroup)
        const int64_t pt = list.index[at];
        const unsigned long long word = list.word[at];
        double par[kMaxParams];
        int T;
        fetch_point<P>(src, pt, par, T);
        clamp_point<P>(m, par);
        const bool units16 = sub_units16(word);
        const int64_t row_first = units16 ? (int64_t)sub_first(word) * 16 : (int64_t)sub_first(word);
        const int64_t row_last = units16 ? (int64_t)sub_last(word) * 16 + 15 : (int64_t)sub_last(word);
        // (the products the recurrence kernels form, point_fetch.h error_class_rate_mul: a few 1e-16 relative from the
        // pow-made rates of K-direct -- far below the grain of the subnormal terms this kernel exists for -- and 40
        // instructions a point instead of the two pows' 420)
        const double lam = error_class_rate_mul(m, par[0], par[1], s, S);
        const int o_hi = T;
        double value = ll[pt];
        for (int64_t chunk = row_first; chunk <= row_last; chunk += kWave) { // wave-uniform
            const int64_t row = chunk + lane;
            const int bin = (row <= row_last && row < (int64_t)tv.n_tiles * kTileBins) ? tv.row_bin[row] : -1;
            const double h = bin >= 0 ? m.bins.cnt[bin] : 0.0;
            const bool counted = bin >= 0 && h != 0.0;
            const double key = counted ? m.bins.key[bin] : 0.0;
            const double nlg = counted ? -m.bins.lgam[bin] : 0.0;
            double pj = 0.0; // of this lane's row
            const uint64_t cm = __ballot(counted);
            if (cm) {
                // the chunk's smallest and largest counted key (rows ascend with the keys)
                const int l_lo = __builtin_ctzll(cm), l_hi = 63 - __builtin_clzll(cm);
                const double k_lo = wave_bcast(key, l_lo), g_lo = wave_bcast(nlg, l_lo);
                const double k_hi = wave_bcast(key, l_hi), g_hi = wave_bcast(nlg, l_hi);
                // lots of OT copy numbers
                for (int o0 = 1; o0 < o_hi; o0 += OT) {
                    // ---- lane-parallel preparation of up to OT * S mixture components (mix_lot.h) ----
                    const int o = o0 + og;
                    const bool live = lane_in_tile && o < o_hi;
                    const double x = (double)o * lam;
                    {
                        // A whole lot out of reach of the chunk (the usual case) is not prepared at all: the same
                        // test as below in single precision, with the normaliser's floor  D(x) >= x - 19  for
                        // x >= 1 (point_fetch.h: x + ln(1 - e^-xr), xr > 1e-8) and room for the float error of
                        // key * ln x (<= 0.02 at the key cap).
                        const float lxf = __logf((float)x);
                        const float reach = fmaxf(fmaf((float)k_lo, lxf, (float)g_lo), fmaf((float)k_hi, lxf, (float)g_hi));
                        const bool far = x >= 1.0 && (x < k_lo - 1.0 || x > k_hi + 1.0) &&
                                         (double)reach - (x - 19.0) < -745.5;
                        if (!__any(live && !far))
                            continue; // wave-uniform
                    }
                    MixLot c;
                    prepare_mix_lot<P>(TableMath{log_tab}, par, comb_s, x, live, o, og * S, S, c);
                    // Which components reach any row of the chunk at all?  exp(arg) rounds to 0 below ln 2^-1075
                    // = -745.13, and arg is concave in the key with its top within 1 of x: outside [k_lo - 1,
                    // k_hi + 1] it is monotone over the chunk's keys and the nearer end bounds it.  (Most copy
                    // numbers, for the keys of a deep tail: their terms are exactly 0 in the reference too.)
                    const bool inside = x >= k_lo - 1.0 && x <= k_hi + 1.0;
                    const double top = fmax(fma(k_lo, c.lx, c.nd + g_lo), fma(k_hi, c.lx, c.nd + g_hi));
                    const uint64_t keep = __ballot(c.a != 0.0 && (inside || top >= -745.2));
                    // ---- every lane accumulates the kept ones for its own row ----
                    // inner = the classes of one copy number in ascending order, pj += b_o * inner per copy number that
                    // has any (covest/models.py:237) -- the TERMS four at a time (round 5): an exp is a chain of forty-five
                    // dependent instructions, and one wave a SIMD (a launch of this kernel is one trip of every wave) does
                    // not hide one behind another unless they are written side by side.  The sums are the same sums: a
                    // batch's terms are added one by one, in order, to the copy number they belong to.
                    {
                        uint64_t km = keep;
                        int cur_end = 0; // one past the last lane of the copy number `inner` belongs to (0: none yet)
                        double inner = 0.0;
                        while (km) { // wave-uniform
                            int idx[4];
                            int n = 0;
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                idx[u] = km ? __builtin_ctzll(km) : idx[0]; // (a short batch repeats its first term and drops it)
                                n += km ? 1 : 0;
                                km &= km - 1; // (0 stays 0)
                            }
                            double t[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                t[u] = wave_bcast(c.a, idx[u]) * exp(fma(key, wave_bcast(c.lx, idx[u]), wave_bcast(c.nd, idx[u]) + nlg));
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                if (u >= n)
                                    break;
                                if (idx[u] >= cur_end) { // the first kept class of another copy number
                                    if (cur_end > 0)
                                        pj += wave_bcast(c.b, cur_end - S) * inner;
                                    inner = 0.0;
                                    while (idx[u] >= cur_end)
                                        cur_end += S;
                                }
                                inner += t[u];
                            }
                        }
                        if (cur_end > 0)
                            pj += wave_bcast(c.b, cur_end - S) * inner;
                    }
                }
            }
            const bool fix = counted && pj < list.p_clamp;
            const double contrib = fix ? h * ((pj <= 0.0 ? -INFINITY : log(pj)) - list.log_p_clamp) : 0.0;
            uint64_t todo = __ballot(fix);
            while (todo) { // ascending rows
                const int kk = __builtin_ctzll(todo);
                todo &= todo - 1;
                value += wave_bcast(contrib, kk);
            }
        }
        if (lane == 0)
            ll[pt] = value;
    }
}

// The same hand-back for the BASIC model, several points a wave (round 4).  A basic-model point has ONE copy number: its
// S mixture components are prepared by S lanes, and ll_fix_list_kernel<2> above left the other 64 - S idle through
// the whole preparation (exp_neg_rn, a division, three logs) and then used a dozen of its 64 lanes for the point's
// dozen rows -- 1 900 instructions a point, 28 us of C2's 238 us step.  Here a wave takes G = 64 / S queued points at
// once: lane (g, s) prepares component s of point g, then stands for row s of a pass of S rows of point g, the
// components reaching it through the lanes' crossbar (the group's own, in ascending s).  The arithmetic of a row is the
// one above to the letter -- the terms a_s exp(key ln x_s - D_s - ln key!) added in ascending s (a component that is out
// of reach adds an exact 0: the kernel above skips it, which is the same), b_o = 1, the contributions of a point's rows
// in ascending order.
// Round 5.  C2 hands 7 266 of its 10^6 points back: 908 waves, fewer than the chip has SIMDs, so the launch lasts as
// long as ONE wave's chain of dependent loads and calls -- 16.8 us of a 188 us step.  What shortened it: the class count
// as a compile-time 8 (SC), the loops over the classes unrolled so that a row's eight exps and their crossbar reads
// interleave instead of following one another -- 16.5 -> 14.8 us (profiles/r05_c2_kstat_fix_classes_unrolled.txt).
// What did not, and stays because it is less code in flight: the class's rate by multiplication
// (error_class_rate_mul: the very products K-basic itself forms, point_fetch.h) instead of two calls of the device
// library's pow; a queue entry's loads -- the entry, the point's axis values and value, the rows' bins of the first
// pass -- issued together with the log table's, before its barrier, and the rows of the next pass during this one
// (16.93 -> 16.85 us).  Measured and not kept: a wave a point with lane (row, component) holding ONE term -- an exp a lane
// and pass instead of S -- is eight times the waves, each repeating the preparation: 36.5 us,
// profiles/r05_c2_kstat_fix_wave_per_point_not_kept.txt.
template <int SC> // the class count as a constant: every loop over the classes unrolled, a row's exps interleaved
__global__ __launch_bounds__(256) void ll_fix_basic_packed_kernel(const DevModel m, const int32_t n_tiles, const int32_t n_items,
                                                                  const double *__restrict__ tile_dbl,
                                                                  const int32_t *__restrict__ tile_int, const PointSource src,
                                                                  double *__restrict__ ll, const SubList list)
{
    const unsigned count = __builtin_amdgcn_readfirstlane(*list.count);
    if (count == 0)
        return; // (workgroup-uniform) the common case: a launch and one load
    __shared__ __attribute__((aligned(16))) double log_tab[kLogTableDoubles];
    load_log_table(log_tab);
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    const int lane = threadIdx.x & (kWave - 1);
    constexpr int S = SC;             // m.n_err: 8, 16, 24 or 32 (padded: comb = 0 beyond the model's classes)
    constexpr int G = kWave / S;      // points a wave takes at once
    const int g = lane / S, s = lane - g * S;
    const bool in_group = g < G;
    const int first_lane = (in_group ? g : 0) * S; // the group's lane 0 (idle lanes shadow group 0 and store nothing)
    const double comb_s = m.comb[s];
    const int64_t n_rows_table = (int64_t)tv.n_tiles * kTileBins;
    const unsigned wave_global = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const unsigned n_waves = gridDim.x * (blockDim.x / kWave);
    // A queue entry and what hangs on it by loads alone: the point, its value, this lane's row of the first pass
    // {h_j, key, -ln key!} (h = 0: no such row, or no count)
    bool have = false;
    int64_t pt = 0, row_first = 0, row_last = -1;
    double par[kMaxParams] = {0, 0, 0, 0, 0};
    int T = 0;
    double value = 0.0, h_n = 0.0, key_n = 0.0, nlg_n = 0.0;
    auto fetch_row = [&](int64_t r0, double &h, double &key, double &nlg) {
        const int64_t row = row_first + r0 + s;
        const int bin = (have && row <= row_last && row < n_rows_table) ? tv.row_bin[row] : -1;
        h = bin >= 0 ? m.bins.cnt[bin] : 0.0;
        key = (bin >= 0 && h != 0.0) ? m.bins.key[bin] : 0.0;
        nlg = (bin >= 0 && h != 0.0) ? -m.bins.lgam[bin] : 0.0;
    };
    auto fetch_entry = [&](unsigned base) {
        const unsigned at = base + (unsigned)(in_group ? g : 0);
        have = in_group && at < count;
        pt = list.index[have ? at : base];
        const unsigned long long word = have ? list.word[at] : 0ull;
        const bool units16 = sub_units16(word);
        row_first = units16 ? (int64_t)sub_first(word) * 16 : (int64_t)sub_first(word);
        row_last = units16 ? (int64_t)sub_last(word) * 16 + 15 : (int64_t)sub_last(word);
        fetch_row(0, h_n, key_n, nlg_n);
        fetch_point<2>(src, pt, par, T);
        value = have ? ll[pt] : 0.0;
    };
    const unsigned base0 = wave_global * (unsigned)G;
    if (base0 < count) // (wave-uniform) the first entry's loads and the table's are in flight together
        fetch_entry(base0);
    __syncthreads(); // the table is readable
    for (unsigned base = base0; base < count; base += n_waves * (unsigned)G) { // wave-uniform
        if (base != base0)
            fetch_entry(base);
        clamp_point<2>(m, par);
        // ---- component s of point g, with the rate K-basic had (ll_basic.hip): one copy number, o = 1 ----
        const double x = error_class_rate_mul(m, par[0], par[1], s, S);
        MixLot c;
        prepare_mix_lot<2>(TableMath{log_tab}, par, comb_s, x, have && T > 1, 1, first_lane, S, c);
        // ---- the point's rows, S at a time ----
        const int64_t my_rows = have ? row_last - row_first + 1 : 0;
        int64_t most = my_rows;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            most = max(most, __shfl_xor(most, off, kWave)); // wave-uniform trip count
        for (int64_t r0 = 0; r0 < most; r0 += S) {
            const double h = h_n, key = key_n, nlg = nlg_n;
            if (r0 + S < most)
                fetch_row(r0 + S, h_n, key_n, nlg_n);
            const bool counted = h != 0.0;
            double pj = 0.0;
#pragma unroll
            for (int t = 0; t < S; ++t) { // error classes, ascending
                const double a_t = __shfl(c.a, first_lane + t, kWave);
                const double lx_t = __shfl(c.lx, first_lane + t, kWave);
                const double nd_t = __shfl(c.nd, first_lane + t, kWave);
                const double term = a_t * exp(fma(key, lx_t, nd_t + nlg));
                pj += (a_t != 0.0) ? term : 0.0; // (a component without weight is left out above: it adds nothing here)
            }
            const bool fix = counted && pj < list.p_clamp;
            const double contrib = fix ? h * ((pj <= 0.0 ? -INFINITY : log(pj)) - list.log_p_clamp) : 0.0;
#pragma unroll
            for (int t = 0; t < S; ++t) { // ascending rows of the group's point
                const double c_t = __shfl(contrib, first_lane + t, kWave);
                const bool f_t = __shfl((int)fix, first_lane + t, kWave) != 0;
                if (f_t)
                    value += c_t;
            }
        }
        if (have && s == 0)
            ll[pt] = value;
    }
}

} // namespace

// the instantiations of this file's dispatcher, by name (the launch record, covest_compiled_variants)
// (the `,1` of fix_list is historical -- the waves a point took, a template argument until this file was split
// off -- and stays because the tests and tools/compare_point_libs.py match on the names)
const char *const kFixVariantNames[kFixVariants] = {"fix_basic_packed<8>",  "fix_basic_packed<16>", "fix_basic_packed<24>",
                                                    "fix_basic_packed<32>", "fix_list<2,1>",        "fix_list<5,1>"};

hipError_t launch_ll_fix_list(const DevModel &m, const TileView &tv, const PointSource &src, double *ll,
                              const SubList &list, hipStream_t stream, int64_t n_points)
{
    // enough workgroups to spread a few thousand queued points over the chip -- four points a workgroup, no more of them
    // than the launch before can have queued points for; an empty queue is the common case
    const dim3 grid((unsigned)std::min<int64_t>(2048, std::max<int64_t>(64, n_points > 0 ? (n_points + 3) / 4 : 2048))), block(256);
    // (the packed kernel: 64 / S points a wave; no more workgroups than the launch before can have queued points for -- an
    // optimize_grid search launches this hundreds of times on an empty queue)
    const int packed_blocks = (int)std::min<int64_t>(512, std::max<int64_t>(16, n_points > 0 ? (n_points + 31) / 32 : 512));
    if (m.kind == 0 && m.n_err <= 32 && m.n_err % 8 == 0) {
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(packed_blocks), block, 0, stream, m, tv.n_tiles, tv.n_items, tv.dbl_base, tv.int_base, src,
                               ll, list);
        };
        record_launch(kFixVariantNames[m.n_err == 8 ? 0 : m.n_err == 16 ? 1 : m.n_err == 24 ? 2 : 3]); // (the switch below)
        switch (m.n_err) {
        case 8: go(ll_fix_basic_packed_kernel<8>); break;
        case 16: go(ll_fix_basic_packed_kernel<16>); break;
        case 24: go(ll_fix_basic_packed_kernel<24>); break;
        default: go(ll_fix_basic_packed_kernel<32>); break;
        }
    } else if (m.kind == 0) {
        record_launch(kFixVariantNames[4]);
        hipLaunchKernelGGL(ll_fix_list_kernel<2>, grid, block, 0, stream, m, tv.n_tiles, tv.n_items, tv.dbl_base,
                           tv.int_base, src, ll, list);
    } else {
        record_launch(kFixVariantNames[5]);
        hipLaunchKernelGGL(ll_fix_list_kernel<5>, grid, block, 0, stream, m, tv.n_tiles, tv.n_items, tv.dbl_base,
                           tv.int_base, src, ll, list);
    }
    return hipGetLastError();
}

} // namespace covest
