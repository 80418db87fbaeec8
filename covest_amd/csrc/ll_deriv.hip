// ll_deriv.hip -- the derivative kernels, for gfx950.  ORDER 1 is K-grad: the log-likelihood of a point list AND its
// analytic gradient.  ORDER 2 is K-hess: those two AND the Hessian in closed form.  ORDER kDerivOpg (3; a mode, not a
// third derivative) is K-opg: K-grad's walk, unchanged, AND the outer product of the per-k-mer scores,
//     B_kl = sum_{h_j != 0} h_j r_k(j) r_l(j) + [tail != 0, sp < 1] tail S_k S_l / (1 - sp)^2,   r_k = d_k p_j / p_j,
// S_k = sum_j d_k p_j: the meat of the sandwich covariance.  One source, templated on the model
// (P parameters) and on the order; everything second-order sits behind `if constexpr (ORDER == 2)`, everything of the
// outer product behind `if constexpr (ORDER == kDerivOpg)`.
//
// The function differentiated is what the kernels evaluate, piece by piece, at the point after fit_to_bounds
// (clamp_point), with threshold_o held fixed, the reference's two roundings kept in the weights and given no derivative
// (DESIGN.md sections 6e, 6f have the formulas).  The model is a finite sum of exponentials: beside the exp every pmf
// term pays for anyway, a first derivative in c or in e costs two fused multiply-adds,
//     d/dtheta [a_os TP(x, j)] = TP(x, j) (alpha + j beta),
// with alpha = da_os - a_os L'(x) o dlambda_s and beta = a_os o dlambda_s / x wave-uniform per component, and a second
// derivative for theta, theta' in {c, e} three,
//     d d' [a_os TP(x, j)] = TP(x, j) (alpha2 + j beta2 + j^2 gamma2)
// (hess_coef below).  The derivatives in q1, q2, q touch the copy-number weights b_o only: d q_k is the class's plain
// inner sum weighted by db_o / dq_k, (theta, q_k) the class's inner sum of d theta weighted by db_o / dq_k, (q_k, q_l)
// the plain inner sum weighted by d2 b_o / dq_k dq_l.
//
// The scheme is K-direct's (direct_point.h): components prepared lane-parallel and broadcast through the scalar unit,
// one exp per (component, key), every lane owning keys; the value uses the same expressions.  But ONE WORKGROUP PER
// (point, key segment) instead of one wave per point: keys are independent up to the final sums, so a segment of
// kDerivSegKeys keys -- one key a lane, four waves -- leaves compensated partial sums, and ll_deriv_finish_kernel adds a
// point's segments in ascending order, applies the tail terms and (ORDER 2, K-opg) mirrors the upper triangle.  The segment
// size and every order of summation are a function of the model alone: a point's numbers do not depend on what else is
// in the call.  The first-order arithmetic is the same expressions in both orders, so the two return the same value and
// the same gradient.
//
// Where a key's p_j is a subnormal double nothing is handed back: the terms are formed one by one as K-direct forms them.
#include <hip/hip_runtime.h>
#include <tuple>

#include "direct_point.h"
#include "grad_common.h"
#include "kernels.h"

namespace covest {

namespace {

constexpr int kDerivWaves = 4;
constexpr int kDerivSegKeys = kDerivWaves * kWave; // one key a lane
constexpr int64_t kDerivPointsPerLaunch = 16384;   // (gridDim.y)

// The sums a segment leaves, each as a (hi, lo) pair, NP the parameter pairs (k <= l, row by row) of ORDER 2, none of
// the others; NB the same pairs of K-opg, none of the others:
//   0 sum h log p (finite terms), 1 sum p,
//   kG + k   sum h d_k p / p,            kD + k   sum d_k p,
//   kH + kl  sum h (d_k d_l p / p - d_k p d_l p / p^2),      kDD + kl  sum d_k d_l p,
//   kB + kl  sum h (d_k p / p)(d_l p / p);
// behind them ONE double: the sum of the terms h log p that are not finite (-inf where p_j = 0, NaN), kept out of the
// compensated sums they would poison.
template <int P, int ORDER> struct DerivLayout {
    static_assert(ORDER == 1 || ORDER == 2 || ORDER == kDerivOpg, "K-grad, K-hess or K-opg");
    static constexpr int kPairs = ORDER == 2 ? P * (P + 1) / 2 : 0;
    static constexpr int kOuter = ORDER == kDerivOpg ? P * (P + 1) / 2 : 0;
    static constexpr int kG = 2, kD = 2 + P, kH = 2 + 2 * P, kDD = 2 + 2 * P + kPairs, kB = 2 + 2 * P + 2 * kPairs;
    static constexpr int kSums = 2 + 2 * P + 2 * kPairs + kOuter;
    static constexpr int kStride = 2 * kSums + 1;
    static_assert(kSums + 1 <= kWave, "the finishing kernel adds one quantity a thread");
};

__host__ __device__ constexpr int pair_index(int P, int k, int l) { return k * P - k * (k - 1) / 2 + (l - k); } // k <= l

// The component's second-order coefficients in the key for the parameters theta, theta': a = a_os with first derivatives
// da, dap and second derivative d2a; x = o lambda_s with dx, dxp, d2x; l1 = L'(x), l2 = L''(x), ix = 1 / x.
__device__ __forceinline__ void hess_coef(double a, double da, double dap, double d2a, double dx, double dxp, double d2x,
                                          double ix, double l1, double l2, double &al, double &be, double &ga)
{
    const double xx = dx * dxp;
    const double cross = da * dxp + dap * dx;
    ga = a * xx * ix * ix;
    be = (cross + a * d2x - 2.0 * a * l1 * xx) * ix - ga;
    al = d2a - l1 * cross - a * l1 * d2x + a * xx * (l1 * l1 - l2);
}

// TABLE (orders 1 and 2; DESIGN.md sections 6u, 6x) is the same walk with its per-key quantities stored on the way, before
// the counts enter: Extra is then (double *rows, int32_t *dead) -- into row RT pt of `rows` (n_bins doubles a row; RT = P + 1
// at order 1, 1 + P + P (P + 1) / 2 at order 2) goes log p_j, behind it the P rows d_k p_j / p_j, at order 2 behind those
// the rows c_kl(j) = d_k d_l p_j / p_j - (d_k p_j / p_j)(d_l p_j / p_j), k <= l row by row, and dead[pt] (zeroed by the
// launcher) counts the keys with p_j <= 0.  It is launched on the batch's all-keys view with zero counts and tail 1, so that
// the segment sums are those of the pure tail term and ll_deriv_finish_kernel<P, ORDER> returns the tail coefficients.  The
// stores sit in the key epilogue behind `if constexpr`; without TABLE the pack is empty and the six instantiations compile
// to the instructions they had, and the order-1 table's to those it had.
template <int P, int ORDER, bool TABLE = false, class... Extra>
__global__ __launch_bounds__(kDerivWaves *kWave) void ll_deriv_kernel(const DevModel m, const PointSource src,
                                                                      double *__restrict__ partial, Extra... extra)
{
    static_assert(!TABLE || ORDER == 1 || ORDER == 2, "the table is first or second order");
    static_assert(sizeof...(Extra) == (TABLE ? 2 : 0), "TABLE takes (double *rows, int32_t *dead)");
    double *rows = nullptr;
    int32_t *dead = nullptr;
    if constexpr (TABLE) {
        const std::tuple<Extra...> table(extra...);
        rows = std::get<0>(table);
        dead = std::get<1>(table);
    }
    using L = DerivLayout<P, ORDER>;
    constexpr int NQ = L::kSums, STRIDE = L::kStride, NP = L::kPairs;
    constexpr int NP1 = NP > 0 ? NP : 1; // (an array's length)
    __shared__ double red[kDerivWaves][STRIDE];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t pt = blockIdx.y;
    const int64_t n_bins = m.bins.n;
    const int64_t idx = (int64_t)blockIdx.x * kDerivSegKeys + (int64_t)wave * kWave + lane;
    const bool ok = idx < n_bins;

    double val[NQ]; // this lane's key's term of every sum
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        val[q] = 0.0;
    double special = 0.0;

    if ((int64_t)blockIdx.x * kDerivSegKeys + (int64_t)wave * kWave < n_bins) { // (wave-uniform) the wave has keys
        double par[kMaxParams];
        int T;
        fetch_point<P>(src, pt, par, T);
        bool moved[P]; // (TABLE) the clamp moved the parameter: its score row is 0, K-grad's rule (its c_kl rows: K-hess's)
        if constexpr (TABLE) {
            double raw[P];
#pragma unroll
            for (int d = 0; d < P; ++d)
                raw[d] = par[d];
            clamp_point<P>(m, par);
#pragma unroll
            for (int d = 0; d < P; ++d)
                moved[d] = par[d] != raw[d];
        } else {
            clamp_point<P>(m, par);
        }

        const int S = m.n_err;
        const int OT = kWave / S; // copy-number classes prepared per tile
        const int s = lane % S;
        const int og = lane / S;
        const bool lane_in_tile = og < OT;
        const double c = par[0], err = par[1];
        const double lam = error_class_rate(m, c, err, s);
        const double comb_s = m.comb[s];
        // lambda_s = ck 3^-s e^s (1 - e)^(k - s), ck = c (r - k + 1) / r.  d lambda_s / dc = lambda_s / c;
        // d lambda_s / de = ck 3^-s [s e^(s-1) (1-e)^(k-s) - (k-s) e^s (1-e)^(k-s-1)], and so on: a term with a zero
        // coefficient dropped (pow(0, 0) = 1), so that e = 0 and c = 0 need no division
        const double dlam_c = c != 0.0 ? lam / c : error_class_rate(m, 1.0, err, s);
        const double ck = c * (double)(m.r - m.k + 1) / (double)m.r;
        const int ks = m.k - s;
        double de = 0.0;
        if (s > 0)
            de = (double)s * pow(err, (double)(s - 1)) * pow(1.0 - err, (double)ks);
        if (ks > 0)
            de -= (double)ks * pow(err, (double)s) * pow(1.0 - err, (double)(ks - 1));
        const double dlam_e = ck * m.pow3neg[s] * de;
        double d2lam_ce = 0.0, d2lam_ee = 0.0; // (d2 lambda / dc2 = 0)
        if constexpr (ORDER == 2) {
            const double ck1 = (double)(m.r - m.k + 1) / (double)m.r;
            const double sd = (double)s, ksd = (double)ks;
            double d2e = 0.0;
            if (s > 1)
                d2e = sd * (sd - 1.0) * pow(err, sd - 2.0) * pow(1.0 - err, ksd);
            if (s > 0 && ks > 0)
                d2e -= 2.0 * sd * ksd * pow(err, sd - 1.0) * pow(1.0 - err, ksd - 1.0);
            if (ks > 1)
                d2e += ksd * (ksd - 1.0) * pow(err, sd) * pow(1.0 - err, ksd - 2.0);
            d2lam_ce = ck1 * m.pow3neg[s] * de; // (d lambda / de) / c
            d2lam_ee = ck * m.pow3neg[s] * d2e;
        }

        const double key = ok ? m.bins.key[idx] : 0.0;
        const double nlg = ok ? -m.bins.lgam[idx] : 0.0;
        double p = 0.0, p1[P], p2[NP1];
#pragma unroll
        for (int d = 0; d < P; ++d)
            p1[d] = 0.0;
#pragma unroll
        for (int q = 0; q < NP1; ++q)
            p2[q] = 0.0;
        double inner = 0.0, inner_c = 0.0, inner_e = 0.0, inner_cc = 0.0, inner_ce = 0.0, inner_ee = 0.0;

        for (int o0 = 1; o0 < T; o0 += OT) {
            // ---- lane-parallel preparation of up to OT*S mixture components (as prepare_mix_lot, mix_lot.h, with the
            // derivatives of tot summed in the same shuffle loop) ----
            const int o = o0 + og;
            const bool live = lane_in_tile && o < T;
            const double od = (double)o;
            const double x = od * lam;
            const double ex = exp_neg_rn(x);
            const double n_os = comb_s * (1.0 - ex);
            const double dn_c = comb_s * ex * od * dlam_c;
            const double dn_e = comb_s * ex * od * dlam_e;
            // second order: its own names for o dlambda, o d2lambda and comb e^-x (first order keeps K-grad's association)
            const double dx_c = od * dlam_c, dx_e = od * dlam_e;
            double d2x_ce = 0.0, d2x_ee = 0.0, d2n_cc = 0.0, d2n_ce = 0.0, d2n_ee = 0.0;
            if constexpr (ORDER == 2) {
                const double cex = comb_s * ex;
                d2x_ce = od * d2lam_ce;
                d2x_ee = od * d2lam_ee;
                d2n_cc = -cex * dx_c * dx_c; // comb e^-x (d d'x - dx d'x)
                d2n_ce = cex * (d2x_ce - dx_c * dx_e);
                d2n_ee = cex * (d2x_ee - dx_e * dx_e);
            }
            double tot = 0.0, dtot_c = 0.0, dtot_e = 0.0, d2tot_cc = 0.0, d2tot_ce = 0.0, d2tot_ee = 0.0;
            for (int t = 0; t < S; ++t) {
                tot += __shfl(n_os, og * S + t, kWave);
                dtot_c += __shfl(dn_c, og * S + t, kWave);
                dtot_e += __shfl(dn_e, og * S + t, kWave);
                if constexpr (ORDER == 2) {
                    d2tot_cc += __shfl(d2n_cc, og * S + t, kWave);
                    d2tot_ce += __shfl(d2n_ce, og * S + t, kWave);
                    d2tot_ee += __shfl(d2n_ee, og * S + t, kWave);
                }
            }
            const bool replaced = tot == 0.0; // fix_zero: a_os is the constant 0 there
            if (replaced)
                tot = 1.0;
            double a_os = n_os / tot;
            const double da_c = replaced ? 0.0 : (dn_c - a_os * dtot_c) / tot;
            const double da_e = replaced ? 0.0 : (dn_e - a_os * dtot_e) / tot;
            double d2a_cc = 0.0, d2a_ce = 0.0, d2a_ee = 0.0;
            if constexpr (ORDER == 2) {
                if (!replaced) {
                    d2a_cc = (d2n_cc - 2.0 * da_c * dtot_c - a_os * d2tot_cc) / tot;
                    d2a_ce = (d2n_ce - da_c * dtot_e - da_e * dtot_c - a_os * d2tot_ce) / tot;
                    d2a_ee = (d2n_ee - 2.0 * da_e * dtot_e - a_os * d2tot_ee) / tot;
                }
            }
            // b_o and its derivatives: first in q1, q2, q; second q1q2, q1q, q2q, qq (q1q1 = q2q2 = 0)
            double b_o = 1.0, db_q1 = 0.0, db_q2 = 0.0, db_q = 0.0, d2b_12 = 0.0, d2b_1q = 0.0, d2b_2q = 0.0, d2b_qq = 0.0;
            if (P == 5) {
                const double q1 = par[2], q2 = par[3], q = par[4];
                b_o = copy_number_weight(q1, q2, q, o);
                if (o == 1) {
                    db_q1 = 1.0;
                } else if (o == 2) {
                    db_q1 = -q2;
                    db_q2 = 1.0 - q1;
                    d2b_12 = -1.0;
                } else {
                    // g = q (1 - q)^(o - 3) and g', g'', a term with a zero coefficient dropped
                    const double n3 = (double)(o - 3);
                    const double w = pow(1.0 - q, n3);
                    const double w1 = o > 3 ? pow(1.0 - q, (double)(o - 4)) : 0.0;
                    const double g1 = o == 3 ? 1.0 : w - n3 * q * w1;
                    db_q1 = -(1.0 - q2) * q * w;
                    db_q2 = -(1.0 - q1) * q * w;
                    db_q = (1.0 - q1) * (1.0 - q2) * g1;
                    if constexpr (ORDER == 2) {
                        double g2 = 0.0;
                        if (o > 3)
                            g2 = -2.0 * n3 * w1;
                        if (o > 4)
                            g2 += n3 * (n3 - 1.0) * q * pow(1.0 - q, n3 - 2.0);
                        d2b_12 = q * w;
                        d2b_1q = -(1.0 - q2) * g1;
                        d2b_2q = -(1.0 - q1) * g1;
                        d2b_qq = (1.0 - q1) * (1.0 - q2) * g2;
                    }
                }
            }
            double lx = 0.0, nd = -INFINITY;
            double al_c = 0.0, be_c = 0.0, al_e = 0.0, be_e = 0.0;
            double al_cc = 0.0, be_cc = 0.0, ga_cc = 0.0, al_ce = 0.0, be_ce = 0.0, ga_ce = 0.0, al_ee = 0.0, be_ee = 0.0,
                   ga_ee = 0.0;
            if (live && x > 0.0) {
                lx = log(x);
                nd = -log_trunc_norm(x, lx);
                double dl, l2 = 0.0; // L'(x), L''(x)
                if constexpr (ORDER == 2)
                    trunc_norm_dlog2(x, dl, l2);
                else
                    dl = trunc_norm_dlog(x);
                al_c = da_c - a_os * dl * od * dlam_c;
                be_c = c != 0.0 ? a_os / c : a_os * od * dlam_c / x;
                al_e = da_e - a_os * dl * od * dlam_e;
                be_e = a_os * od * dlam_e / x;
                if constexpr (ORDER == 2) {
                    const double ix = 1.0 / x;
                    hess_coef(a_os, da_c, da_c, d2a_cc, dx_c, dx_c, 0.0, ix, dl, l2, al_cc, be_cc, ga_cc);
                    hess_coef(a_os, da_c, da_e, d2a_ce, dx_c, dx_e, d2x_ce, ix, dl, l2, al_ce, be_ce, ga_ce);
                    hess_coef(a_os, da_e, da_e, d2a_ee, dx_e, dx_e, d2x_ee, ix, dl, l2, al_ee, be_ee, ga_ee);
                }
            }
            if (!live)
                a_os = 0.0;
            // a component that weighs nothing and none of whose coefficients moves is skipped (NaN falls through, as in
            // K-direct)
            bool idle = a_os == 0.0 && al_c == 0.0 && al_e == 0.0;
            if constexpr (ORDER == 2)
                idle = idle && al_cc == 0.0 && be_cc == 0.0 && ga_cc == 0.0 && al_ce == 0.0 && be_ce == 0.0 && ga_ce == 0.0 &&
                       al_ee == 0.0 && be_ee == 0.0 && ga_ee == 0.0;
            const int use = (live && !idle) ? 1 : 0;

            // ---- every lane accumulates all components for its own key ----
            const int n_comp = min(OT, T - o0) * S;
            for (int i = 0; i < n_comp; ++i) {
                if (__builtin_amdgcn_readlane(use, i)) { // wave-uniform
                    const double a_i = wave_bcast(a_os, i);
                    const double l_i = wave_bcast(lx, i);
                    const double d_i = wave_bcast(nd, i);
                    const double t = exp(fma(key, l_i, d_i + nlg));
                    inner += a_i * t;
                    inner_c = fma(t, fma(key, wave_bcast(be_c, i), wave_bcast(al_c, i)), inner_c);
                    inner_e = fma(t, fma(key, wave_bcast(be_e, i), wave_bcast(al_e, i)), inner_e);
                    if constexpr (ORDER == 2) {
                        inner_cc = fma(t, fma(key, fma(key, wave_bcast(ga_cc, i), wave_bcast(be_cc, i)), wave_bcast(al_cc, i)),
                                       inner_cc);
                        inner_ce = fma(t, fma(key, fma(key, wave_bcast(ga_ce, i), wave_bcast(be_ce, i)), wave_bcast(al_ce, i)),
                                       inner_ce);
                        inner_ee = fma(t, fma(key, fma(key, wave_bcast(ga_ee, i), wave_bcast(be_ee, i)), wave_bcast(al_ee, i)),
                                       inner_ee);
                    }
                }
                if ((i + 1) % S == 0) { // end of one copy-number class
                    const double b_i = wave_bcast(b_o, i);
                    p += b_i * inner;
                    p1[0] += b_i * inner_c;
                    p1[1] += b_i * inner_e;
                    if constexpr (ORDER == 2) {
                        p2[pair_index(P, 0, 0)] += b_i * inner_cc;
                        p2[pair_index(P, 0, 1)] += b_i * inner_ce;
                        p2[pair_index(P, 1, 1)] += b_i * inner_ee;
                    }
                    if constexpr (P == 5) {
                        const double d1 = wave_bcast(db_q1, i), d2 = wave_bcast(db_q2, i), d3 = wave_bcast(db_q, i);
                        p1[2] += d1 * inner;
                        p1[3] += d2 * inner;
                        p1[4] += d3 * inner;
                        if constexpr (ORDER == 2) {
                            p2[pair_index(P, 0, 2)] += d1 * inner_c;
                            p2[pair_index(P, 0, 3)] += d2 * inner_c;
                            p2[pair_index(P, 0, 4)] += d3 * inner_c;
                            p2[pair_index(P, 1, 2)] += d1 * inner_e;
                            p2[pair_index(P, 1, 3)] += d2 * inner_e;
                            p2[pair_index(P, 1, 4)] += d3 * inner_e;
                            p2[pair_index(P, 2, 3)] += wave_bcast(d2b_12, i) * inner;
                            p2[pair_index(P, 2, 4)] += wave_bcast(d2b_1q, i) * inner;
                            p2[pair_index(P, 3, 4)] += wave_bcast(d2b_2q, i) * inner;
                            p2[pair_index(P, 4, 4)] += wave_bcast(d2b_qq, i) * inner;
                        }
                    }
                    inner = inner_c = inner_e = inner_cc = inner_ce = inner_ee = 0.0;
                }
            }
        }

        // ---- key epilogue: this key's term of every sum ----
        if (ok) {
            const double h = m.bins.cnt[idx];
            val[1] = p;
#pragma unroll
            for (int d = 0; d < P; ++d)
                val[L::kD + d] = p1[d];
#pragma unroll
            for (int q = 0; q < NP; ++q)
                val[L::kDD + q] = p2[q];
            if constexpr (TABLE) {
                // the batch table's conventions (ll_batch.hip): +0.0 is a dead key's and nothing else's, p = 1 is -0.0,
                // NaN stays NaN; a dead key's scores are +0.0, so that a histogram that does not count it adds 0
                double *row = rows + (int64_t)pt * (P + 1 + NP) * n_bins + idx; // (P + 1 + NP rows a point)
                const bool is_dead = p <= 0.0;
                double l = 0.0;
                if (!is_dead) {
                    l = log(p);
                    if (l == 0.0)
                        l = -0.0;
                }
                row[0] = l;
#pragma unroll
                for (int d = 0; d < P; ++d)
                    row[(int64_t)(1 + d) * n_bins] = (is_dead || moved[d]) ? 0.0 : p1[d] / p;
                if constexpr (ORDER == 2) {
                    double r1[P]; // d_k p / p, as the sums below form it
#pragma unroll
                    for (int d = 0; d < P; ++d)
                        r1[d] = p1[d] / p;
#pragma unroll
                    for (int k = 0; k < P; ++k)
#pragma unroll
                        for (int l = k; l < P; ++l) {
                            const int q = pair_index(P, k, l);
                            row[(int64_t)(1 + P + q) * n_bins] = (is_dead || moved[k] || moved[l]) ? 0.0 : p2[q] / p - r1[k] * r1[l];
                        }
                }
                if (is_dead)
                    atomicAdd(dead + pt, 1);
            }
            if (h != 0.0) {
                const double term = h * ((p <= 0.0) ? -INFINITY : log(p));
                if (term - term == 0.0) // finite
                    val[0] = term;
                else
                    special = term;
#pragma unroll
                for (int d = 0; d < P; ++d)
                    val[L::kG + d] = h * p1[d] / p;
                if constexpr (ORDER == 2) {
                    double r1[P]; // d_k p / p
#pragma unroll
                    for (int d = 0; d < P; ++d)
                        r1[d] = p1[d] / p;
#pragma unroll
                    for (int k = 0; k < P; ++k)
#pragma unroll
                        for (int l = k; l < P; ++l)
                            val[L::kH + pair_index(P, k, l)] = h * (p2[pair_index(P, k, l)] / p - r1[k] * r1[l]);
                }
                if constexpr (ORDER == kDerivOpg) {
                    double r1[P]; // the score's factors d_k p / p
#pragma unroll
                    for (int d = 0; d < P; ++d)
                        r1[d] = p1[d] / p;
#pragma unroll
                    for (int k = 0; k < P; ++k)
#pragma unroll
                        for (int l = k; l < P; ++l)
                            val[L::kB + pair_index(P, k, l)] = h * r1[k] * r1[l];
                }
            }
        }
    }

    // ---- the workgroup's sums: lanes by butterfly, waves in ascending order ----
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const CompSum r = wave_comp_reduce(CompSum{val[q], 0.0});
        if (lane == 0) {
            red[wave][2 * q] = r.hi;
            red[wave][2 * q + 1] = r.lo;
        }
    }
    special = wave_sum(special);
    if (lane == 0)
        red[wave][2 * NQ] = special;
    __syncthreads();
    if (threadIdx.x <= NQ) {
        double *out = partial + ((int64_t)pt * gridDim.x + blockIdx.x) * STRIDE;
        const int q = threadIdx.x;
        if (q < NQ) {
            CompSum r = {0.0, 0.0};
            for (int w = 0; w < kDerivWaves; ++w)
                comp_merge(r, red[w][2 * q], red[w][2 * q + 1]);
            out[2 * q] = r.hi;
            out[2 * q + 1] = r.lo;
        } else {
            double r = 0.0;
            for (int w = 0; w < kDerivWaves; ++w)
                r += red[w][2 * NQ];
            out[2 * NQ] = r;
        }
    }
}

// One workgroup a point: thread q adds quantity q over the point's segments in ascending order.  Then, with
// on = [tail != 0 and sp < 1]:  LL = sum h log p + on tail log(1 - sp);  threads 0 .. P - 1 form
// d_k LL = sum h d_k p / p - on tail (sum d_k p) / (1 - sp), and (ORDER 2) threads 0 .. NP - 1 one pair (k <= l) each,
// d_k d_l LL = sum h (d_k d_l p / p - d_k p d_l p / p^2) - on tail [sum d_k d_l p / (1 - sp) + (sum d_k p)(sum d_l p) / (1 - sp)^2],
// written to H[k][l] and H[l][k] (out_hess is not read for ORDER 1).  K-opg has the same threads form
// B_kl = sum h (d_k p / p)(d_l p / p) + on tail (sum d_k p)(sum d_l p) / (1 - sp)^2 and write it where ORDER 2 writes H.
// A component, a row and a column whose parameter the clamp moved are 0; where LL is not finite every entry is NaN.
template <int P, int ORDER>
__global__ __launch_bounds__(kWave) void ll_deriv_finish_kernel(const DevModel m, const PointSource src, int n_seg,
                                                                const double *__restrict__ partial, double *__restrict__ out_ll,
                                                                double *__restrict__ out_grad, double *__restrict__ out_hess)
{
    using L = DerivLayout<P, ORDER>;
    constexpr int NQ = L::kSums, STRIDE = L::kStride;
    constexpr int NT = ORDER == 2 ? L::kPairs : ORDER == kDerivOpg ? L::kOuter : P; // threads with an entry to write
    __shared__ double tot[NQ + 1];
    const int64_t pt = blockIdx.x;
    const int q = threadIdx.x;
    const double *base = partial + pt * (int64_t)n_seg * STRIDE;
    if (q < NQ) {
        CompSum r = {0.0, 0.0};
        for (int sg = 0; sg < n_seg; ++sg)
            comp_merge(r, base[(int64_t)sg * STRIDE + 2 * q], base[(int64_t)sg * STRIDE + 2 * q + 1]);
        tot[q] = r.hi + r.lo;
    } else if (q == NQ) {
        double r = 0.0;
        for (int sg = 0; sg < n_seg; ++sg)
            r += base[(int64_t)sg * STRIDE + 2 * NQ];
        tot[NQ] = r;
    }
    __syncthreads();
    if (q < NT) {
        double raw[kMaxParams], par[kMaxParams];
        int T;
        fetch_point<P>(src, pt, raw, T);
#pragma unroll
        for (int d = 0; d < P; ++d)
            par[d] = raw[d];
        clamp_point<P>(m, par);
        int k = 0, l = 0; // (ORDER 2, K-opg) the pair this thread owns
        bool moved_k = false, moved_l = false, moved_q = false;
#pragma unroll
        for (int a = 0; a < P; ++a) {
            if (a == q)
                moved_q = par[a] != raw[a];
            if constexpr (ORDER != 1) {
#pragma unroll
                for (int b = a; b < P; ++b)
                    if (pair_index(P, a, b) == q) {
                        k = a, l = b;
                        moved_k = par[a] != raw[a];
                        moved_l = par[b] != raw[b];
                    }
            }
        }
        double ll = tot[0] + tot[NQ];
        double g = q < P ? tot[L::kG + q] : 0.0;
        double hkl = 0.0;
        if constexpr (ORDER == 2)
            hkl = tot[L::kH + q];
        if constexpr (ORDER == kDerivOpg)
            hkl = tot[L::kB + q];
        if (m.tail != 0.0) { // tail * log(1 - min(1, sp)), covest/models.py:103-105
            double sp = tot[1];
            if (!(sp < 1.0))
                sp = 1.0;
            if (sp < 1.0) {
                ll += m.tail * log(1.0 - sp);
                if (q < P)
                    g -= m.tail * tot[L::kD + q] / (1.0 - sp);
                if constexpr (ORDER == 2) {
                    const double inv = 1.0 / (1.0 - sp);
                    hkl -= m.tail * (tot[L::kDD + q] * inv + tot[L::kD + k] * tot[L::kD + l] * inv * inv);
                }
                if constexpr (ORDER == kDerivOpg) { // the tail as one more class: score -S_k / (1 - sp), tail times
                    const double inv = 1.0 / (1.0 - sp);
                    hkl += m.tail * (tot[L::kD + k] * tot[L::kD + l] * inv * inv);
                }
            }
        }
        if (moved_q)
            g = 0.0;
        if (moved_k || moved_l)
            hkl = 0.0;
        if (!(ll - ll == 0.0)) {
            g = NAN;
            hkl = NAN;
        }
        if constexpr (ORDER != 1) {
            out_hess[(pt * P + k) * P + l] = hkl;
            out_hess[(pt * P + l) * P + k] = hkl;
        }
        if (q < P)
            out_grad[pt * P + q] = g;
        if (q == 0)
            out_ll[pt] = ll;
    }
}

template <int P, int ORDER>
void launch_part(const DevModel &m, const PointSource &part, int n_seg, int64_t cnt, double *partial, double *out_ll,
                 double *out_grad, double *out_hess, double *rows, int32_t *dead, hipStream_t stream)
{
    if (rows) {
        if constexpr (ORDER == 1 || ORDER == 2)
            hipLaunchKernelGGL((ll_deriv_kernel<P, ORDER, true, double *, int32_t *>), dim3((unsigned)n_seg, (unsigned)cnt), dim3(kDerivWaves * kWave), 0,
                               stream, m, part, partial, rows, dead);
    } else {
        hipLaunchKernelGGL((ll_deriv_kernel<P, ORDER>), dim3((unsigned)n_seg, (unsigned)cnt), dim3(kDerivWaves * kWave), 0,
                           stream, m, part, partial);
    }
    hipLaunchKernelGGL((ll_deriv_finish_kernel<P, ORDER>), dim3((unsigned)cnt), dim3(kWave), 0, stream, m, part, n_seg, partial,
                       out_ll, out_grad, out_hess);
}

} // namespace

// the instantiations of launch_ll_deriv's dispatch, by name (the launch record, covest_compiled_variants): 3 * (P == 5) +
// (order 1, 2, kDerivOpg -> 0, 1, 2); the finishing kernel's six share one name
const char *const kDerivVariantNames[kDerivVariants] = {"ll_deriv<2,grad>", "ll_deriv<2,hess>", "ll_deriv<2,opg>", "ll_deriv<5,grad>",
                                                        "ll_deriv<5,hess>", "ll_deriv<5,opg>", "ll_deriv_finish"};

int ll_deriv_segments(const DevModel &m)
{
    const int64_t n = (m.bins.n + kDerivSegKeys - 1) / kDerivSegKeys;
    return n < 1 ? 1 : (int)n;
}

size_t ll_deriv_partial_bytes(const DevModel &m, int order, int64_t n)
{
    const int64_t pts = n < kDerivPointsPerLaunch ? n : kDerivPointsPerLaunch;
    const int stride = m.kind == 0 ? (order == 2           ? DerivLayout<2, 2>::kStride
                                      : order == kDerivOpg ? DerivLayout<2, kDerivOpg>::kStride
                                                           : DerivLayout<2, 1>::kStride)
                                   : (order == 2           ? DerivLayout<5, 2>::kStride
                                      : order == kDerivOpg ? DerivLayout<5, kDerivOpg>::kStride
                                                           : DerivLayout<5, 1>::kStride);
    return (size_t)pts * (size_t)ll_deriv_segments(m) * (size_t)stride * sizeof(double);
}

namespace {

// the launches of a point list, cut at kDerivPointsPerLaunch points; rows != nullptr: the table-writing walk (order 1 or 2)
hipError_t deriv_launches(const DevModel &m, int order, const PointSource &src, int64_t n, double *partial, double *out_ll,
                          double *out_grad, double *out_hess, double *rows, int32_t *dead, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    if (src.is_grid || (order != 1 && order != 2 && order != kDerivOpg) || (rows && (order == kDerivOpg || !dead)))
        return hipErrorInvalidValue;
    const int n_seg = ll_deriv_segments(m);
    const int P = m.kind == 0 ? 2 : 5;
    const int64_t table_rows = order == 2 ? 1 + P + P * (P + 1) / 2 : P + 1; // (rows a point of the table-writing walk)
    const auto launch = P == 2 ? (order == 1 ? launch_part<2, 1> : order == 2 ? launch_part<2, 2> : launch_part<2, kDerivOpg>)
                               : (order == 1 ? launch_part<5, 1> : order == 2 ? launch_part<5, 2> : launch_part<5, kDerivOpg>);
    for (int64_t first = 0; first < n; first += kDerivPointsPerLaunch) {
        const int64_t cnt = n - first < kDerivPointsPerLaunch ? n - first : kDerivPointsPerLaunch;
        launch(m, points_from(src, first, P), n_seg, cnt, partial, out_ll + first, out_grad + first * P,
               order != 1 ? out_hess + first * P * P : nullptr, rows ? rows + first * table_rows * m.bins.n : nullptr,
               rows ? dead + first : nullptr, stream);
        if (!rows) // (the table-writing walk is the batch's: not a variant of the launch record)
            record_launch(kDerivVariantNames[(P == 5 ? 3 : 0) + (order == 1 ? 0 : order == 2 ? 1 : 2)]);
        record_launch(kDerivVariantNames[kDerivVariants - 1]);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_ll_deriv(const DevModel &m, int order, const PointSource &src, int64_t n, double *partial, double *out_ll,
                           double *out_grad, double *out_hess, hipStream_t stream)
{
    return deriv_launches(m, order, src, n, partial, out_ll, out_grad, out_hess, nullptr, nullptr, stream);
}

hipError_t launch_ll_deriv_table(const DevModel &m, int order, const PointSource &src, int64_t n, double *partial, double *rows,
                                 int32_t *dead, double *out_ll, double *out_grad, double *out_hess, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    const hipError_t err = hipMemsetAsync(dead, 0, (size_t)n * sizeof(int32_t), stream);
    if (err != hipSuccess)
        return err;
    return deriv_launches(m, order, src, n, partial, out_ll, out_grad, out_hess, rows, dead, stream);
}

} // namespace covest
