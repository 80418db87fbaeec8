// mix_lot.h -- the lane-parallel preparation of ONE LOT of mixture components (copy number o, error class s), the core
// of the term-by-term ("strict") evaluation: K-direct's body and strict_pj_wave (direct_point.h) and the two hand-back
// kernels (ll_fix.hip) all call prepare_mix_lot, so the reference's rule is restated here and nowhere else.  (The
// derivative kernel, ll_deriv.hip, forms the same values interleaved with their derivatives and keeps its own copy.)
//
// Reference restated (paths relative to the reference checkout):
//   BasicModel.compute_probabilities    covest/models.py:85-97    (one copy number: o = 1, b_o = 1)
//   RepeatsModel.compute_probabilities  covest/models.py:221-241
#pragma once
#include <hip/hip_runtime.h>

#include "fastmath.h"
#include "point_fetch.h"
#include "wave.h"

namespace covest {

// The two ways the callers take a component's logs and a copy number's weight.
// K-direct and strict_pj_wave: the device library's log and pow, the arithmetic the tests hold against the reference.
struct LibmMath {
    __device__ __forceinline__ double log_x(double x) const { return log(x); }
    __device__ __forceinline__ double log_norm(double x, double lx) const { return log_trunc_norm(x, lx); }
    __device__ __forceinline__ double weight(double q1, double q2, double q, int o) const { return copy_number_weight(q1, q2, q, o); }
};
// The hand-back kernels: the logs through the LDS copy of the fast_log table (absolute error 2e-16, what the recurrence
// kernels' anchors are made with) and the weight by squaring (point_fetch.h) -- their terms are rounded onto the
// 4.9e-324 grid, far above either difference.
struct TableMath {
    const double *tab; // load_log_table's
    __device__ __forceinline__ double log_x(double x) const { return fast_log(x, tab); }
    __device__ __forceinline__ double log_norm(double x, double lx) const { return log_trunc_norm(x, lx, tab); }
    __device__ __forceinline__ double weight(double q1, double q2, double q, int o) const { return copy_number_weight_by_squaring(q1, q2, q, o); }
};

// This lane's component of a lot: its term at key j is  a * exp(j * lx + nd - ln j!),  and p_j += b * (the terms of the
// copy number's classes, ascending).
struct MixLot {
    double a;  // a_os, 0 for a lane that is not live
    double b;  // b_o (1 in the basic model)
    double lx; // ln x
    double nd; // -D(x), the log of the truncated Poisson's normaliser; -inf where x = 0: the term is a * 0
};

// All 64 lanes call this together.  par: the point's parameters AFTER clamp_point; comb_s: m.comb of the lane's class;
// x = o * l_s of the lane's component; live: the lane holds a component of the point at all; the S lanes from
// first_lane on hold the classes of the lane's copy number o, ascending.
// (The lot is an out-parameter on purpose: returned by value, the same statements compile to other code in every caller.)
template <int P, class Math>
__device__ __forceinline__ void prepare_mix_lot(const Math &math, const double *par, double comb_s, double x, bool live,
                                                int o, int first_lane, int S, MixLot &c)
{
    const double n_os = comb_s * (1.0 - exp_neg_rn(x)); // exp(o * -l_s[s]): NOT expm1, as the reference  models.py:87,221
    double tot = 0.0;                                   // naive sum in s order                            models.py:88,225
    for (int t = 0; t < S; ++t)
        tot += __shfl(n_os, first_lane + t, kWave);
    if (tot == 0.0)
        tot = 1.0;                                      // fix_zero
    c.a = n_os / tot;
    c.b = (P == 5) ? math.weight(par[2], par[3], par[4], o) : 1.0;
    c.lx = 0.0;
    c.nd = -INFINITY; // exp(key * 0 - inf) = 0: the component contributes a_os * 0
    if (live && x > 0.0) {
        c.lx = math.log_x(x);                           // x = o * l_s[s]                                  models.py:93,238
        c.nd = -math.log_norm(x, c.lx);
    }
    if (!live)
        c.a = 0.0;
}

} // namespace covest
