// band.h -- the BAND of a (contraction unit, key tile) of K-factored (ll_factored.hip): the MFMA steps (4 copy
// numbers each) outside of which the terms of  P_j = sum_o b_o G[o][j]  add up to less than 2^-64 of P_j, for every
// weight vector (column) of the unit and every key of the tile.  Plain C++, compiled for the host (tests/band_check.cpp)
// and for the device (the kernel's prologue); the logarithm and the reciprocal come from the caller (libm on the host;
// the kernel's table logarithm and the hardware's reciprocal on the device), see "roundings" below.
//
// The unit belongs to a q-tile whose 16 columns have ONE q (tiles.h, shared steps):  b_o = beta_col (1-q)^(o-3) for
// o >= 3, so the ratio of two terms of a column does not depend on the column.  With
//     term_s(o, j) = b_o comb_s e^(-o l_s) (o l_s)^j / (j! N(o)),    N(o) = sum_s comb_s (1 - e^(-o l_s))
// (covest/models.py:220-240: a_os TP(o l_s, j), the (1 - e^..) of the mixture weight and of the truncated Poisson
// cancel) and a REFERENCE copy number o* in 3 .. o_ref_max, below every column's cut-off, P_j >= term_0(o*, j): the
// terms are not negative.  For o > o*:  N(o) >= N(o*)  (N rises), so
//     ln term_0(o, j) / term_0(o*, j) <= -(o - o*) L + j ln(o / o*),   L = l_0 - ln(1-q)                          (1)
//     ln term_s(o, j) / term_0(o*, j) <= ln(comb_s / comb_0) + o* l_0 + (o - o*) ln(1-q) + j ln(o_top l_s / (o* l_0))  (2)
// ((2) drops e^(-o l_s) <= 1 and takes o <= o_top, the unit's largest copy number).  (1) is concave in o and rises with
// j: its root beyond the mode at the tile's LAST key is bracketed from outside by Newton steps -- the tangent of a
// concave function lies above it, so every iterate is at or beyond the root -- and rounded outward.  (2) is linear in
// j: it is tested at both ends of the tile, at the edge found from (1); the classes s >= 1 are thereby PROVABLY
// negligible beyond the edge, or the band is the full range (early tiles: their rates are 150 times smaller, but at
// low keys that is not enough).  At most 2^12 terms are dropped (512 copy numbers, 8 classes), each below
// e^-kBandLn = 2^-80.8 of P_j: less than 2^-68 together.
//
// Roundings: the edge from (1) is rounded up and moved out by one more copy number.  That covers a logarithm good to
// 1e-12 absolute and a reciprocal good to 1e-9 relative (the keys are below 2^14, the copy numbers below 2^10); (2) is
// only compared with a bound that has 2^4 to spare.
//
// The lower edge is not cut: step_lo is 0 (step 0, o = 1 .. 4 with the weights that are not geometric, is always taken).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef COVEST_HD
#ifdef __HIPCC__
#define COVEST_HD __host__ __device__
#else
#define COVEST_HD
#endif
#endif

namespace covest {

constexpr double kBandLn = 56.0;   // a dropped term is below e^-56 of the column's reference term
constexpr int kBandClasses = 8;    // error classes of a PLAIN grid (one lane per copy number)
constexpr int kBandNewton = 2;     // tangent steps towards the upper root (each one valid, each one tighter: from
                                   //   2 mode + 8 two of them end within three copy numbers of the root)

constexpr int kBandMinShared = 8; // a unit with fewer shared steps keeps its full range (the planner's "too short to gain":
                                  //   its band would cost the prologue more than it can save)

struct Band {
    int step_lo, step_hi; // MFMA steps [step_lo, step_hi) are needed
};

// What a key tile contributes, whatever the unit: its keys (rows past the last key may be counted in: a wider range is
// safe) and the classes' part of (2) at either end,  max over s >= 1 of  ln(comb_s / comb_0) + j ln(l_s / l_0).
struct BandTile {
    double key_first, key_last, cls_first, cls_last;
};

// ln_rate[s] = ln l_s (-inf: no rate), ln_comb[s] = ln comb_s (-inf: a padding class, it weighs nothing)
COVEST_HD inline BandTile band_tile(const double *ln_rate, const double *ln_comb, double key_first, double key_last)
{
    BandTile t = {key_first, key_last, -INFINITY, -INFINITY};
    for (int s = 1; s < kBandClasses; ++s) {
        const double lc = ln_comb[s] - ln_comb[0], lr = ln_rate[s] - ln_rate[0];
        if (!(lc > -INFINITY))
            continue;
        const double a = lc + key_first * lr, b = lc + key_last * lr;
        t.cls_first = a > t.cls_first ? a : t.cls_first;
        t.cls_last = b > t.cls_last ? b : t.cls_last;
    }
    return t;
}

// The host's arithmetic: libm's logarithm, a true division.
struct BandMathHost {
    double ln(double x) const { return log(x); }
    double rcp(double x) const { return 1.0 / x; }
};

// rate0 = l_0 (its logarithm must be finite: band_tile subtracts it); ln_1mq = ln(1 - q) of the unit's q-tile (<= 0);
// o_ref_max: a copy number >= 3 below the unit's SMALLEST cut-off (4 + 4 unit_nsh: the shared steps lie below it);
// n_steps: the unit's MFMA steps, shared ones included (its largest copy number is 4 n_steps).
// Returns {0, n_steps} wherever the bound cannot be proved.
template <class Math>
COVEST_HD inline Band band_of_unit(const Math &mth, double rate0, double ln_1mq, int o_ref_max, int n_steps, const BandTile &t)
{
    const Band full = {0, n_steps};
    const double mu = -ln_1mq, L = rate0 + mu;
    // (every test is written so that a NaN fails it)
    if (!(rate0 > 0.0) || !(mu >= 0.0) || !(L < 1e300) || !(t.key_first >= 1.0) || !(t.key_last >= t.key_first) ||
        !(t.key_last < 16384.0) || o_ref_max < 3 || n_steps < 2)
        return full;
    const double mode = t.key_last * mth.rcp(L);
    double o_ref = floor(mode);
    o_ref = o_ref < 3.0 ? 3.0 : o_ref;
    o_ref = o_ref > (double)o_ref_max ? (double)o_ref_max : o_ref;
    const double inv_ref = mth.rcp(o_ref);
    // (1): g(o) = -(o - o*) L + j ln(o / o*) + kBandLn, its root beyond the mode
    double a = 2.0 * mode + 8.0; // (beyond the mode: g' < 0 there)
    for (int it = 0; it < kBandNewton; ++it) {
        const double g = -(a - o_ref) * L + t.key_last * mth.ln(a * inv_ref) + kBandLn;
        const double dg = -L + t.key_last * mth.rcp(a);
        if (!(dg < 0.0))
            return full;
        a -= g * mth.rcp(dg);
        if (!(a > mode))
            return full; // (cannot happen with exact arithmetic: the iterates stay beyond the root)
    }
    const double o_edge = ceil(a) + 1.0; // outward, and one more for the roundings
    if (!(o_edge < 4.0 * (double)n_steps))
        return full;
    const int step_hi = ((int)o_edge + 2) >> 2; // steps >= step_hi hold copy numbers >= 1 + 4 step_hi >= o_edge only
    if (step_hi < 1 || step_hi >= n_steps)
        return full;
    // (2) at the copy numbers actually dropped, o >= 1 + 4 step_hi, for both ends of the tile
    const double o_drop = 1.0 + 4.0 * (double)step_hi, o_top = 4.0 * (double)n_steps;
    const double base = o_ref * rate0 - (o_drop - o_ref) * mu + kBandLn, ln_o = mth.ln(o_top * inv_ref);
    if (!(base + t.key_first * ln_o + t.cls_first <= 0.0) || !(base + t.key_last * ln_o + t.cls_last <= 0.0))
        return full;
    return Band{0, step_hi};
}

// THE COLUMN LIMIT (ll_factored.hip col_hi).  The steps below a band's upper edge hold the copy numbers
// 1 .. 4 step_hi: the largest one the unit reads with a weight that matters in the tile.  The maximum of it over the units of a
// workgroup -- and, for the units without a band, of their largest copy number -- is a limit above which NO unit needs a
// column of G in that tile, and a builder wave whose 64 copy numbers all lie above it need not build them: the columns
// hold zeros instead.  What a unit then loses are terms the proof above already drops, or terms of the steps that the
// clamped step loops run beyond the band's edge (factored_contract.h): both below 2^-68 of P_j together, for every key
// of the tile and every column of the unit.  WITH A TAIL the same columns are missing from S[o] = sum_j G[o][j]
// (ll_factored.hip SPO), whose contraction is sp = sum_j P_j: the bound holds key by key, so the share lost from sp is
// below 2^-68 sp as well.
COVEST_HD inline int band_top_column(const Band &b) { return 4 * b.step_hi; }

// What the planner knows of the limit (plan_factored.cpp; tiles.h FactoredPlan::col_floor, band_extra), for the slots
// of ONE workgroup, [n_waves][slots_per_wave]: tile (-1: none), shared steps, "continues the slot before" per slot,
// top[tile] = the largest copy number a unit of the q-tile reads.  Waves n_build .. n_waves - 1 build nothing: they
// make the bands of their own long units (kBandMinShared shared steps or more, in one piece) and of up to n_extra_max
// long units of the builders, one per q-tile none of them holds -- their slots go to extra[] (-1: none).  Every other
// unit keeps its full range: returns the largest copy number such a unit reads, at least floor_min.  Not `plain`, or no
// wave that builds nothing: no unit has a band.
inline int column_limit_of_block(const int32_t *tile, const int32_t *nsh, const int32_t *cont, const int32_t *top, int n_waves,
                                 int slots_per_wave, int n_build, bool plain, int floor_min, int32_t *extra, int n_extra_max)
{
    const bool bands = plain && n_build < n_waves;
    int floor = floor_min, n_made = 0, n_extra = 0;
    int32_t made[64]; // q-tiles with a band
    for (int j = 0; j < n_extra_max; ++j)
        extra[j] = -1;
    for (int round = 0; round < 2; ++round) // the waves that build nothing first: what they hold they make anyway
        for (int w = round == 0 ? n_build : 0; w < (round == 0 ? n_waves : (n_build < n_waves ? n_build : n_waves)); ++w)
            for (int k = 0; k < slots_per_wave; ++k) {
                const int at = w * slots_per_wave + k;
                if (tile[at] < 0)
                    continue;
                bool has_band = false;
                if (bands && nsh[at] >= kBandMinShared && !cont[at] && !(k + 1 < slots_per_wave && tile[at + 1] == tile[at] && cont[at + 1])) {
                    bool known = false;
                    for (int i = 0; i < n_made; ++i)
                        known = known || made[i] == tile[at];
                    if (round == 0 || known) {
                        has_band = true;
                    } else if (n_extra < n_extra_max) {
                        extra[n_extra++] = at;
                        has_band = true;
                    }
                    if (has_band && !known && n_made < 64)
                        made[n_made++] = tile[at];
                    else if (has_band && !known)
                        has_band = round == 0; // (the list is full: a builder's unit keeps its full range)
                }
                if (!has_band)
                    floor = floor > top[tile[at]] ? floor : top[tile[at]];
            }
    return floor;
}

// The upper edges (step_hi) of a wave's six slots as the kernel keeps them: a byte a slot in two registers, 255: not
// banded (the full range; an edge of 255 steps or more is as good as none: a unit has 128 steps at most).  In the
// kernel lane t holds the bytes of item t of the walk: set per lane in the prologue, one lane read a register and item.
struct BandBytes {
    static constexpr int kSlots = 6, kNone = 255;
    unsigned w0 = ~0u, w1 = ~0u; // slots 0 .. 3, slots 4 and 5
    COVEST_HD void set(int k, int step_hi)
    {
        const unsigned hi = (unsigned)(step_hi < kNone ? step_hi : kNone);
        if (k < 4)
            w0 = (w0 & ~(255u << (8 * k))) | (hi << (8 * k));
        else
            w1 = (w1 & ~(255u << (8 * (k - 4)))) | (hi << (8 * (k - 4)));
    }
    COVEST_HD int get(int k) const { return (int)(((k < 4 ? w0 >> (8 * k) : w1 >> (8 * (k - 4)))) & 255u); }
};

} // namespace covest
