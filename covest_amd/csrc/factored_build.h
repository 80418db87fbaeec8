// factored_build.h -- K-factored, PHASE A (ll_factored.hip): G'[key][o] of one item of the walk into an LDS buffer,
// lane = copy number, by the error-class streams of streams.h.
//   reads   the item's tile records and scales (TileView), the lane's streams
//   writes  32 rows of the lane's column of the buffer; (SPO) the lane's S[o]; the streams, advanced past the item
// SPO: returns sum_b u_b 2^SC of this lane's copy number over the tile's 32 keys (u_b: the true terms' sum at key
// b, streams.h) WITHOUT the keys' 32 scales: with  W_b = (u_0 + .. + u_b) / scal_b,  scal_(b-1) / scal_b = k0 + b
// (tiles.h) gives
//     W_b = W_(b-1) (k0 + b) + g_b,          g_b = the streams' sum at key b, what goes to LDS anyway,
// a fused multiply-add and an add a key on a counter that holds the key as a double (exact: keys <= 16384), and the
// tile's sum is W_31 scal_31 = W_31 renorm 2^-SC.  W stays inside the range the streams' own terms are scaled for
// (partial sums <= 2.5: at most 2.5 x 2^540 x 1e140).  No scalar is fetched in the walk (the tile's 32 scales
// through scalar registers cost the TAIL variants 45 more spilled scalars and an exposed scalar-cache latency a
// half).  Tiles with a FILLER key (a gap of the histogram: its scale is 0, it must add nothing) and short tiles
// take the key-by-key path of build_tile with the scales.
#pragma once
#include "factored_diag.h"
#include "fastmath.h"
#include "streams.h"
#include "tiles.h"
#include "wave.h"

namespace covest {

// this lane's column of G: column tid of a row of ld doubles, if the row has one (waves past the row build nothing,
// lanes past it hold no copy number: nothing of theirs is ever read)
struct BuildLane {
    int tid, ld;
    bool in_row;
    __device__ __forceinline__ double *column(double *dst) const { return dst + (in_row ? tid : 0); }
};

// THE WALK: the 32 keys of a full tile with the streams 0 .. N-1 (the others are zero in every lane of the wave).  One
// region under the row mask, straight-line inside.
//   STORE   the sums go to LDS as they stand (no scale, see ll_factored.hip), walked row by row from `row` (one vector
//           add a store, no scalar multiply by the row's number); else the tile is a count-less one (tail != 0 only):
//           sum_j G[o][j] over its keys stays in a register -- 32 terms of one sign added plainly, the compensated
//           accumulator of phase C gets their contraction -- and is returned instead of 32 stores
//   SPO     the W recurrence of the header on top of either: returns the tile's share of S[o]
// Neither (TAIL && !SPO, a point list on a model with a tail): the rows ARE scaled, a sum over keys needs every key's
// own scale, `scal`.
template <int N, bool SPO, bool STORE>
__device__ __forceinline__ double walk_tile(StreamSet<8> &st, bool in_row, double *row, int ld, const double *scal, double k0,
                                            double renorm)
{
    if (STORE && !in_row)
        return 0.0; // (lanes past the row hold no copy number: nothing of theirs is ever read)
    // squared rates (the streams advance two keys per step, streams.h step2): N multiplies per tile
    // rather than 16 registers held through phases B and C -- the empty asm keeps the compiler from
    // hoisting them back out of the tile loop (it would spill them).  (Written out here: as a function of its own the
    // block changes which product of a key's sum the compiler fuses, in the walks of the grids with a tail.)
    double xx[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        double xs = st.x[s];
        if (s < N) {
            asm volatile("" : "+v"(xs));
            xx[s] = xs * xs;
        } else {
            xx[s] = 0.0;
        }
    }
    double sum = 0.0;
    if (!SPO && !STORE) {
        // two halves of 16 keys, each half's scales fetched into scalar registers up front (one s_load_dwordx16 pair,
        // as K-basic does): fetched pair by pair right before their use, every second key waited for the scalar cache
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double sc[16];
#pragma unroll
            for (int b = 0; b < 16; ++b)
                sc[b] = scal[16 * half + b];
            asm volatile("" ::: "memory"); // (keeps the loads above the half's arithmetic)
#pragma unroll
            for (int b = 0; b < 16; b += 2) {
                double g1, g2;
                st.template step2n<N>(xx, g1, g2);
                sum = fma(g1, sc[b], sum);
                sum = fma(g2, sc[b + 1], sum);
            }
        }
        st.template leave_tile_n<N>(renorm);
        return sum * (1.0 / kBasicScale); // (tv.scal carries 2^kBasicShift, tiles.h)
    }
    double kk = k0; // the key of row b
#pragma unroll
    for (int b = 0; b < kTileBins; b += 2) {
        double g1, g2;
        st.template step2n<N>(xx, g1, g2);
        if (STORE) {
            row[0] = g1;
            row[ld] = g2;
            row += 2 * ld;
        }
        if (SPO) {
            sum = fma(sum, kk, g1);
            kk += 1.0;
            sum = fma(sum, kk, g2);
            kk += 1.0;
        }
    }
    if (SPO)
        sum *= renorm;
    st.template leave_tile_n<N>(renorm);
    return sum;
}

// One tile: entered (streams.h: which streams are live), then walked by the variant of the walk for the live streams,
// or key by key.  STORE: into `dst` (returns, SPO, the tile's share of S[o]); else a count-less tile, returns its sum.
template <bool SPO, bool STORE>
__device__ __forceinline__ double build_tile(const TileView &tv, const FactoredPlan &plan, StreamSet<8> &st, const BuildLane &ln,
                                             Stamps &stamps, int t, bool seg_start, double *dst)
{
    if (STORE && COVEST_SKIP_PHASE(plan, 1))
        return 0.0;
    const TileRec rc = tv.rec[t]; // (the tile's constants: one scalar load of one cache line, tiles.h)
    const double k0 = rc.k0;
    const int nb = rc.nb;
    // n_live: streams above it are zero in every lane of this wave (streams.h) -- most of them, for most tiles.
    // (Measured and not kept, round 5: the entry compiled for one and for two classes as well and picked by `gone` --
    // C3 0.671 against 0.661 ms, the trimmed histogram with a tail 0.395 against 0.396:
    // profiles/r05_c3_ab_entry_by_live_classes_not_kept.txt.  The gone classes' tests are scalar and cost little;
    // three copies of the entry cost the instruction cache more.)
    // (SPO, a count-less tile: it only enters S[o] -- streams.h enter_sum_tile: a stream is on where it matters to a sum)
    const int n_live = (SPO && !STORE) ? st.enter_sum_tile(k0 - 1.0, k0 + (double)(nb - 1), rc.lgam_prev, rc.lgam_last, rc.run_start != 0 || seg_start)
                                       : st.enter_tile(k0 - 1.0, k0 + (double)(nb - 1), rc.lgam_prev, rc.lgam_last, rc.run_start != 0 || seg_start);
    if (STORE)
        stamps.lap(Stamps::kEnter); // (diagnostic builds: entering the tile apart from walking it)
    double *colp = STORE ? ln.column(dst) : nullptr;
    const double *scal = tv.scal + (int64_t)t * kTileBins;
    // the common case: straight-line code (the count-less tiles of a histogram's tail are full ones: the live streams only)
    if (nb == kTileBins && !(SPO && rc.has_filler != 0)) {
        if (n_live > (STORE ? 4 : 2))
            return walk_tile<8, SPO, STORE>(st, ln.in_row, colp, ln.ld, scal, k0, rc.renorm);
        if (STORE && n_live > 2)
            return walk_tile<4, SPO, STORE>(st, ln.in_row, colp, ln.ld, scal, k0, rc.renorm);
        if (n_live == 2)
            return walk_tile<2, SPO, STORE>(st, ln.in_row, colp, ln.ld, scal, k0, rc.renorm);
        if (n_live == 1)
            return walk_tile<1, SPO, STORE>(st, ln.in_row, colp, ln.ld, scal, k0, rc.renorm);
        if (STORE && ln.in_row) { // nothing is on: G = 0 for this wave's copy numbers
            stamps.count_zero_tile();
#pragma unroll
            for (int b = 0; b < kTileBins; ++b)
                colp[b * ln.ld] = 0.0;
        }
        return 0.0;
    }
    double sum = 0.0;
    for (int b = 0; b < (STORE ? kTileBins : nb); ++b) { // (rows past the tile's keys: 0 -- they carry no count and no scale)
        const double g = b < nb ? st.step() : 0.0;
        if ((SPO || !STORE) && b < nb)
            sum = fma(g, scal[b], sum);
        if (STORE && ln.in_row)
            colp[b * ln.ld] = g;
    }
    st.leave_tile(rc.renorm);
    // (tv.scal carries 2^(kBasicShift - SC); S[o] is kept times 2^SC: exact)
    return SPO ? sum * 0x1p476 : sum * (1.0 / kBasicScale);
}

// (SPO) The whole item -- up to 32 tiles, 1024 keys -- at a glance first: a stream's log-term is concave in the
// key, so where the item does not hold its mode its largest value over the item is at an end.  If that is
// below what a sum can hold (streams.h kSumWindowLn) for every stream of every lane of this wave, nothing
// of the item reaches S[o]: it is skipped for the price of two multiply-adds a stream, where entering
// each of its tiles in turn costs a thousand cycles a tile -- the long count-less stretch of a 10 000-key
// histogram is mostly such items (a wave's copy numbers have their mass within a few hundred keys).
// Wave-uniform.
__device__ __forceinline__ bool sum_item_matters(const TileView &tv, const StreamSet<8> &st, int first, int n)
{
    const int tl = first + n - 1;
    const TileRec ra = tv.rec[first], rb = tv.rec[tl];
    const double ka = ra.k0 - 1.0, kb = rb.k0 + (double)(rb.nb - 1);
    const double lga = ra.lgam_prev, lgb = rb.lgam_last;
    bool matters = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if ((st.gone >> s) & 1u)
            continue; // (wave-uniform)
        const double lx = st.an.lx(s), c = st.an.c(s);
        const double top = fmax(fma(ka, lx, c - lga), fma(kb, lx, c - lgb));
        matters = matters || !(top < StreamSet<8>::kSumWindowLn) || (st.x[s] >= ka - 1.0 && st.x[s] <= kb + 1.0);
    }
    return __any(matters);
}

// One item into `dst`: a plain tile, or (TAIL) the per-tile sums of up to 32 count-less tiles as its rows.
// SKIP (a plain grid), `skip`: the item's column limit (ll_factored.hip col_hi, band.h) lies below every copy number of
// this wave -- wave-uniform.  A tile that holds a count is then neither entered nor walked: the wave's columns of the
// buffer get zeros (readers without a band, and the clamped steps beyond a band's edge, read them with a weight) --
// once a buffer, `zeroed` bit buf_bit: they stay zero through a run of skipped items --, the streams are switched off
// and anchored afresh at the next tile the wave walks (resync: the run-start path), and `gone` is left alone (a stream
// that has gone stays gone at every later key).  A sum item is walked as ever: it is judged by what a sum can hold.
template <bool TAIL, bool SPO, bool SKIP>
__device__ __forceinline__ void build_item(const TileView &tv, const FactoredPlan &plan, StreamSet<8> &st, CompSum &so,
                                           bool &resync, unsigned &zeroed, int tid, int ld, bool in_row, Stamps &stamps, int it,
                                           bool seg_start, bool skip, int buf_bit, double *dst)
{
    const BuildLane ln = {tid, ld, in_row};
    const int first = TAIL ? __builtin_amdgcn_readfirstlane(tv.item_first[it]) : it;
    if (TAIL && tv.item_sum[it] != 0) {
        if (COVEST_SKIP_PHASE(plan, 1))
            return;
        const int n = __builtin_amdgcn_readfirstlane(tv.item_ntiles[it]);
        if (SPO) { // the tiles without a count only enter S[o]: nothing is stored, nothing contracted
            // The streams are anchored afresh at the next tile that is walked (resync), as at the start of a run.
            if (!seg_start && !sum_item_matters(tv, st, first, n)) {
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    st.v[s] = 0.0;
                resync = true;
                return;
            }
            for (int r = 0; r < n; ++r) {
                // (every stream of this wave's copy numbers has GONE -- off in all lanes, outside the window, past its
                // mode, streams.h: exact zeros from here on.  The far end of a long histogram: a wave of small copy
                // numbers is done with H10k_rep's 10 000 keys after the first two thousand)
                if (st.gone == 0xFFu && !(seg_start && r == 0))
                    break;
                so.add(build_tile<SPO, false>(tv, plan, st, ln, stamps, first + r, (seg_start && r == 0) || resync, nullptr));
                resync = false;
            }
            return;
        }
        double *colp = ln.column(dst);
        for (int r = 0; r < n; ++r) {
            const double gsum = build_tile<SPO, false>(tv, plan, st, ln, stamps, first + r, seg_start && r == 0, nullptr);
            if (ln.in_row)
                colp[r * ln.ld] = gsum;
        }
        for (int r = n; r < kTileBins; ++r)
            if (ln.in_row)
                colp[r * ln.ld] = 0.0;
    } else {
        if (SKIP && skip) { // (wave-uniform)
            if (!((zeroed >> buf_bit) & 1u)) {
                zeroed |= 1u << buf_bit;
                if (ln.in_row) {
                    double *colp = ln.column(dst);
#pragma unroll
                    for (int b = 0; b < kTileBins; ++b)
                        colp[b * ln.ld] = 0.0;
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
                st.v[s] = 0.0;
            resync = true;
            stamps.count_skipped_item();
            return;
        }
        if (SKIP)
            zeroed &= ~(1u << buf_bit);
        const double tsum = build_tile<SPO, true>(tv, plan, st, ln, stamps, first, seg_start || ((SPO || SKIP) && resync), dst);
        resync = false;
        if (SPO)
            so.add(tsum);
    }
}

} // namespace covest
