// unit_deal.h -- the cost model by which K-factored's planner deals (q-tile, half) units to the waves of a workgroup
// (plan_factored.cpp place_units; tiles.h): what a builder wave is charged for phase A, and the deal itself -- longest
// unit first into the lightest SIMD.  Plain C++ for the host, with no other header of the library, so that a check
// program runs the planner's own code (tests/deals_check.cpp, tests/test_deals_host.py).
#pragma once
#include <algorithm>
#include <cstdlib>

namespace covest {

constexpr int kBuildShareWaves = 8;
// Per cent of the build charge that builder wave w is charged in a plain part with one workgroup a (c, e) pair: since the
// upper builder waves skip the items above the column limit (band.h) they build 83 / 52 / 35 / 26 % of C3's items, and a
// wave charged for items it skips waits at their barriers.  Found by a search over 840 profiles and confirmed by bench.py
// against the commit before (profiles/deals_charge_sweep.txt, deals_ab.txt).
constexpr int kBuildShare[kBuildShareWaves] = {100, 75, 40, 40, 40, 40, 40, 40};

// Where the shares apply -- the shapes they were measured on; everything else keeps one charge and the tables it had:
// a plain part (list mode 0, one pass, no chunk) of a grid with one workgroup a pair, whose upper builder waves skip items ...
inline bool wave_shares_apply(bool one_block_a_pair, int list_mode, int n_pass, int o_base)
{
    return one_block_a_pair && list_mode == 0 && n_pass == 1 && o_base == 0;
}
// ... and a histogram that is not at low keys alone: the few items of such a one are all early ones, which every
// builder builds (the falling shares cost c3t 7 us a step)
inline int wave_share(bool low_keys, int w) { return low_keys ? 100 : kBuildShare[std::min(std::max(w, 0), kBuildShareWaves - 1)]; }

// (the assignment fixes the order of a point's sums: the shipped library takes the constants of tiles.h and of this file,
// only a diagnostic build -- tiles.h -- or a TUNING build of plan_factored.cpp alone, -DCOVEST_TUNE linked against the
// shipped kernels (tools/build_tune.sh), lets the environment override them: charges_from_env, and nowhere else)
struct Charges {
    int unit_overhead, build_cost, shared_div, last_builder_extra;
    int min_shared; // fewer shared steps than this are left to the MFMA steps
    int build_share[kBuildShareWaves]; // per cent of build_cost a builder wave is charged where the shares apply
#if defined(COVEST_DIAG) || defined(COVEST_TUNE)
    int wave_build[kBuildShareWaves]; // COVEST_FACTORED_BUILD_COST_WAVES: a charge per builder wave (-1: by build_share)
#endif
    // wave w's charge for phase A; shares: wave_shares_apply of the part
    int build_of(int w, bool shares) const
    {
        w = std::min(std::max(w, 0), kBuildShareWaves - 1);
        if (!shares)
            return build_cost;
#if defined(COVEST_DIAG) || defined(COVEST_TUNE)
        if (wave_build[w] >= 0)
            return wave_build[w];
#endif
        return (build_cost * build_share[w] + 50) / 100;
    }
};

#if defined(COVEST_DIAG) || defined(COVEST_TUNE)
// "27,22,14,9,7" -> out[0 ..]; the entries the list does not reach, or that are no numbers, stay
inline void env_int_list(const char *name, int *out, int n)
{
    const char *v = std::getenv(name);
    for (int w = 0; v && w < n && *v; ++w) {
        char *end = nullptr;
        const long c = std::strtol(v, &end, 10);
        if (end == v)
            break;
        out[w] = (int)std::min(1000000l, std::max(0l, c));
        v = *end == ',' ? end + 1 : end;
    }
}
inline void charges_from_env(Charges &ch)
{
    if (const char *v = std::getenv("COVEST_FACTORED_UNIT_OVERHEAD"))
        ch.unit_overhead = std::atoi(v);
    if (const char *v = std::getenv("COVEST_FACTORED_BUILD_COST"))
        ch.build_cost = std::atoi(v);
    if (const char *v = std::getenv("COVEST_FACTORED_SHARED_DIV"))
        ch.shared_div = std::max(1, std::atoi(v));
    if (const char *v = std::getenv("COVEST_FACTORED_LAST_BUILDER_EXTRA"))
        ch.last_builder_extra = std::atoi(v);
    if (const char *v = std::getenv("COVEST_FACTORED_MIN_SHARED"))
        ch.min_shared = std::atoi(v);
    // a charge per builder wave where the shares apply, absolute or in per cent of build_cost
    std::fill(ch.wave_build, ch.wave_build + kBuildShareWaves, -1);
    env_int_list("COVEST_FACTORED_BUILD_COST_WAVES", ch.wave_build, kBuildShareWaves);
    env_int_list("COVEST_FACTORED_BUILD_SHARE_WAVES", ch.build_share, kBuildShareWaves);
}
#endif

// The deal: units by falling cost (cost[0 .. n_units), sorted by the caller), each into the lightest SIMD (waves w and
// w + 4 share one) that still has room, then into the lighter of that SIMD's waves with room; wave_of[i]: unit i's wave.
// builders_charged: G is double-buffered, so the builders -- the waves below n_columns / 64 -- fill the next key tile
// while the others contract, and start with the charge of phase A.  False: a unit found no wave with room.
constexpr int kDealMaxWaves = 16;
inline bool deal_units(const int *cost, int n_units, int n_waves, int n_columns, bool builders_charged, int units_per_wave,
                       const Charges &ch, bool shares, int *wave_of)
{
    if (n_waves < 1 || n_waves > kDealMaxWaves)
        return false;
    const int n_bins = std::min(4, n_waves);
    long bin_load[4] = {0, 0, 0, 0}, wave_load[kDealMaxWaves] = {};
    int n_held[kDealMaxWaves] = {};
    if (builders_charged)
        for (int w = 0; w < n_waves && w * 64 < n_columns; ++w) {
            // (the builder of the TOP copy numbers is the wave every interval waits for -- the stamps of round 3:
            // its streams stay live over the widest range of keys, and it shares its SIMD with another builder)
            const int c = ch.build_of(w, shares) + (((w + 1) * 64 >= n_columns && w >= n_bins) ? ch.last_builder_extra : 0);
            bin_load[w % n_bins] += c;
            wave_load[w] += c;
        }
    for (int i = 0; i < n_units; ++i) {
        int best = -1;
        for (int w = 0; w < n_waves; ++w) {
            if (n_held[w] >= units_per_wave)
                continue;
            if (best < 0) {
                best = w;
                continue;
            }
            const long lb = bin_load[w % n_bins], bb = bin_load[best % n_bins];
            if (lb < bb || (lb == bb && wave_load[w] < wave_load[best]))
                best = w;
        }
        if (best < 0)
            return false;
        wave_of[i] = best;
        n_held[best] += 1;
        bin_load[best % n_bins] += cost[i];
        wave_load[best] += cost[i];
    }
    return true;
}

} // namespace covest
