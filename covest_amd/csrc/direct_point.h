// direct_point.h -- the log-likelihood of ONE grid point computed by ONE wave64, the body of
// K-direct (ll_direct.hip); and, with the same arithmetic, the strict evaluation of single keys for
// the points a recurrence kernel hands back (strict_pj_wave here; the kernels of ll_fix.hip).  The preparation of a lot
// of mixture components, which all of them share, is mix_lot.h; the hand-back's protocol is handback.h.
//
// Every lane owns histogram bins, the (copy number o, error class s) mixture components are
// prepared lane-parallel and broadcast through the scalar unit, every pmf term costs one fp64
// exp, and the per-bin log terms are reduced with wavefront shuffles.  The terms are formed and
// rounded one by one, in the reference's order -- which is what makes this the strict kernel
// where p_j is a subnormal double.
//
// Reference restated (paths relative to the reference checkout):
//   BasicModel.compute_probabilities    covest/models.py:81-98
//   RepeatsModel.compute_probabilities  covest/models.py:211-242
//   BasicModel.compute_loglikelihood    covest/models.py:100-107
//   truncated_poisson                   c_src/covest_poissonmodule.c:7-35
#pragma once
#include <hip/hip_runtime.h>

#include "device_model.h"
#include "mix_lot.h"
#include "point_fetch.h"
#include "tiles.h"
#include "wave.h"

namespace covest {

constexpr int kDirectBinsPerLane = 4; // bins held in registers per lane per pass

// p_j of ONE bin at one point, by the whole wave, with K-direct's arithmetic: the same expressions, the same
// order of the two sums (error classes inside, copy numbers outside: covest/models.py:92-97, :235-241), every
// term rounded to a double on its own.  All lanes call it with the same arguments and get the same value.
// par: the point's parameters AFTER clamp_point; key / neg_lgam: the bin's j and -lgamma(j + 1).
template <int P>
__device__ __forceinline__ double strict_pj_wave(const DevModel &m, const double *par, int T, double key, double neg_lgam)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int S = m.n_err;
    const int OT = kWave / S;
    const int s = lane % S;
    const int og = lane / S;
    const bool lane_in_tile = og < OT;
    const double lam = error_class_rate(m, par[0], par[1], s);
    const double comb_s = m.comb[s];
    double p = 0.0;
    for (int o0 = 1; o0 < T; o0 += OT) {
        const int o = o0 + og;
        const bool live = lane_in_tile && o < T;
        MixLot c;
        prepare_mix_lot<P>(LibmMath{}, par, comb_s, (double)o * lam, live, o, og * S, S, c);
        const double term = c.a != 0.0 ? c.a * exp(fma(key, c.lx, c.nd + neg_lgam)) : 0.0;
        const int n_o = min(OT, T - o0);
        for (int g = 0; g < n_o; ++g) { // wave-uniform; copy numbers in ascending order
            double inner = 0.0;
            for (int t = 0; t < S; ++t)
                inner += __shfl(term, g * S + t, kWave);
            p += __shfl(c.b, g * S, kWave) * inner;
        }
    }
    return p;
}

// ln(LDBL_MAX) of the x87 long double the reference's product lives in (c_src/covest_poissonmodule.c:19-24)
constexpr double kLnLdblMax = 11356.523406294143949492;

// All 64 lanes of a wave call this with the same point; every lane returns the point's LL.
// REF_OVF (COVEST_KERNEL_DIRECT_REF): the reference's OVERFLOW reproduced.  truncated_poisson forms the whole product
// prod_{i <= j} (x / i) in long double before any scaling (c_src/covest_poissonmodule.c:22-24) and returns +inf once the
// running product passes LDBL_MAX -- it grows until i = floor(x), so the term of (x, j) is +inf iff
// m ln x - ln m! > ln LDBL_MAX for m = min(j, floor(x)).  Then p_j = +inf, log p_j = +inf, and the likelihood is +inf,
// or NaN where another counted key has p_j = 0 (inf - inf); sp_j = min(1, fsum(...)) = 1 and the tail term is dropped
// (covest/models.py:103-105).  optimize_grid WOULD select such a point (covest/grid.py:65-70: -(+inf) < anything).
template <int P, bool WRITE_P, bool REF_OVF = false>
__device__ __forceinline__ double direct_point_ll(const DevModel &m, const PointSource &src, int64_t pt,
                                                  double *__restrict__ out_p)
{
    constexpr int kBinsPerLane = kDirectBinsPerLane;
    const int lane = threadIdx.x & (kWave - 1);
    double par[kMaxParams];
    int T;
    fetch_point<P>(src, pt, par, T);
    clamp_point<P>(m, par);

    const int S = m.n_err;
    const int OT = kWave / S; // copy-number classes prepared per tile
    const int s = lane % S;
    const int og = lane / S;
    const bool lane_in_tile = og < OT;
    const double lam = error_class_rate(m, par[0], par[1], s);
    const double comb_s = m.comb[s];

    double acc_ll = 0.0;
    CompSum acc_sp = {0.0, 0.0};
    const int64_t n_bins = m.bins.n;
    bool saw_special = false; // REF_OVF: a p_j that is +inf (or NaN) -- sp_j is then not < 1

    for (int64_t base = 0; base < n_bins; base += (int64_t)kWave * kBinsPerLane) {
        double key[kBinsPerLane], nlg[kBinsPerLane], p[kBinsPerLane], inner[kBinsPerLane];
#pragma unroll
        for (int b = 0; b < kBinsPerLane; ++b) {
            const int64_t idx = base + (int64_t)b * kWave + lane;
            const bool ok = idx < n_bins;
            key[b] = ok ? m.bins.key[idx] : 0.0;
            nlg[b] = ok ? -m.bins.lgam[idx] : 0.0;
            p[b] = 0.0;
            inner[b] = 0.0;
        }

        for (int o0 = 1; o0 < T; o0 += OT) {
            // ---- lane-parallel preparation of up to OT*S mixture components ----
            const int o = o0 + og;
            const bool live = lane_in_tile && o < T;
            const double x = (double)o * lam;
            MixLot c;
            prepare_mix_lot<P>(LibmMath{}, par, comb_s, x, live, o, og * S, S, c);
            // REF_OVF: can this component's product overflow at all (its largest value, at i = floor(x)), and from
            // which key on is that value reached
            double fx = INFINITY;
            if (REF_OVF && live && x >= 1.0) {
                const double top = floor(x);
                if (fma(top, c.lx, -lgamma(top + 1.0)) > kLnLdblMax)
                    fx = top;
            }

            // ---- every lane accumulates all components for its own bins ----
            const int n_comp = min(OT, T - o0) * S;
            for (int i = 0; i < n_comp; ++i) {
                const double a_i = wave_bcast(c.a, i);
                if (a_i != 0.0) { // wave-uniform; NaN falls through and poisons p_j as in the reference
                    const double l_i = wave_bcast(c.lx, i);
                    const double d_i = wave_bcast(c.nd, i);
                    const double fx_i = REF_OVF ? wave_bcast(fx, i) : INFINITY;
                    if (REF_OVF && fx_i < INFINITY) { // (wave-uniform, rare) this component overflows somewhere
#pragma unroll
                        for (int b = 0; b < kBinsPerLane; ++b) {
                            // the running product grows up to i = floor(x): past LDBL_MAX at this key?
                            const bool ovf = key[b] >= fx_i || fma(key[b], l_i, nlg[b]) > kLnLdblMax;
                            inner[b] += a_i * (ovf ? INFINITY : exp(fma(key[b], l_i, d_i + nlg[b])));
                        }
                    } else {
#pragma unroll
                        for (int b = 0; b < kBinsPerLane; ++b)
                            inner[b] += a_i * exp(fma(key[b], l_i, d_i + nlg[b]));
                    }
                }
                if ((i + 1) % S == 0) { // end of one copy-number class: p_j += b_o * inner  models.py:237
                    const double b_i = wave_bcast(c.b, i);
#pragma unroll
                    for (int b = 0; b < kBinsPerLane; ++b) {
                        p[b] += b_i * inner[b];
                        inner[b] = 0.0;
                    }
                }
            }
        }

        // ---- bin epilogue: sp_j contribution and h_j * safe_log(p_j)  models.py:103-106 ----
#pragma unroll
        for (int b = 0; b < kBinsPerLane; ++b) {
            const int64_t idx = base + (int64_t)b * kWave + lane;
            if (idx < n_bins) {
                const double h = m.bins.cnt[idx];
                if (REF_OVF && !(p[b] < INFINITY))
                    saw_special = true; // (+inf or NaN: kept out of the compensated sum, whose error terms it would poison)
                else
                    acc_sp.add(p[b]);
                if (h != 0.0)
                    acc_ll += h * ((p[b] <= 0.0) ? -INFINITY : log(p[b]));
                if (WRITE_P)
                    out_p[idx] = p[b];
            }
        }
    }

    acc_ll = wave_sum(acc_ll);
    double tail_term = 0.0;
    if (m.tail != 0.0) { // tail == 0: the term is 0 * finite = 0 in the reference
        double sp = wave_comp_sum(acc_sp);
        if (!(sp < 1.0))
            sp = 1.0; // min(1, fsum(...)), NaN -> 1
        if (sp < 1.0)
            tail_term = m.tail * log(1.0 - sp);
        if (REF_OVF && __any(saw_special))
            tail_term = 0.0; // min(1, fsum(...)) of a sum with +inf (or NaN) in it is 1: covest/models.py:103-104
    }
    return acc_ll + tail_term;
}

} // namespace covest
