// ll_grad.hip -- K-grad: the log-likelihood of a point list AND its analytic gradient, for gfx950.
//
// The gradient is of what the kernels evaluate, piece by piece, at the point after fit_to_bounds (clamp_point), with
// threshold_o held fixed (DESIGN.md section 6e has the formulas).  The model is a finite sum of exponentials: beside
// the exp every pmf term pays for anyway, the derivative in c and in e costs two fused multiply-adds each,
//     d/dtheta [a_os TP(x, j)] = TP(x, j) (alpha + j beta),
// with alpha = da_os - a_os L'(x) o dlambda_s and beta = a_os o dlambda_s / x wave-uniform per component, and the
// derivatives in q1, q2, q are the copy-number classes' inner sums weighted by db_o/dq instead of b_o.
//
// The scheme is K-direct's (direct_point.h): components prepared lane-parallel and broadcast through the scalar unit,
// one exp per (component, key), every lane owning keys; the value uses the same expressions.  But ONE WORKGROUP PER
// (point, key segment) instead of one wave per point: keys are independent up to the final sums, so a segment of
// kGradSegKeys keys -- one key a lane, four waves -- leaves compensated partial sums, and ll_grad_finish_kernel adds a
// point's segments in ascending order and applies the tail term.  The segment size and every order of summation are a
// function of the model alone: a point's numbers do not depend on what else is in the call.
//
// Where a key's p_j is a subnormal double nothing is handed back: the terms are formed one by one as K-direct forms them.
#include <hip/hip_runtime.h>

#include "direct_point.h"
#include "grad_common.h"
#include "kernels.h"

namespace covest {

namespace {

constexpr int kGradWaves = 4;
constexpr int kGradSegKeys = kGradWaves * kWave; // one key a lane
constexpr int64_t kGradPointsPerLaunch = 16384;  // (gridDim.y)

// The sums a segment leaves, each as a (hi, lo) pair: 0 sum h log p (finite terms), 1 sum p, 2 .. 2 + P - 1
// sum h dp/p per parameter, 2 + P .. 2 + 2P - 1 sum dp per parameter; behind them ONE double: the sum of the terms
// h log p that are not finite (-inf where p_j = 0, NaN), kept out of the compensated sums they would poison.
template <int P> struct GradLayout {
    static constexpr int kSums = 2 + 2 * P;
    static constexpr int kStride = 2 * kSums + 1;
};

template <int P>
__global__ __launch_bounds__(kGradWaves *kWave) void ll_grad_kernel(const DevModel m, const PointSource src,
                                                                    double *__restrict__ partial)
{
    constexpr int NQ = GradLayout<P>::kSums, STRIDE = GradLayout<P>::kStride;
    __shared__ double red[kGradWaves][STRIDE];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t pt = blockIdx.y;
    const int64_t n_bins = m.bins.n;
    const int64_t idx = (int64_t)blockIdx.x * kGradSegKeys + (int64_t)wave * kWave + lane;
    const bool ok = idx < n_bins;

    CompSum sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        sum[q] = {0.0, 0.0};
    double special = 0.0;

    if ((int64_t)blockIdx.x * kGradSegKeys + (int64_t)wave * kWave < n_bins) { // (wave-uniform) the wave has keys
        double par[kMaxParams];
        int T;
        fetch_point<P>(src, pt, par, T);
        clamp_point<P>(m, par);

        const int S = m.n_err;
        const int OT = kWave / S; // copy-number classes prepared per tile
        const int s = lane % S;
        const int og = lane / S;
        const bool lane_in_tile = og < OT;
        const double c = par[0], err = par[1];
        const double lam = error_class_rate(m, c, err, s);
        const double comb_s = m.comb[s];
        // d lambda_s / dc = lambda_s / c;  d lambda_s / de = ck 3^-s [s e^(s-1) (1-e)^(k-s) - (k-s) e^s (1-e)^(k-s-1)],
        // a term with a zero coefficient dropped (pow(0, 0) = 1): e = 0 needs no division
        const double dlam_c = c != 0.0 ? lam / c : error_class_rate(m, 1.0, err, s);
        const double ck = c * (double)(m.r - m.k + 1) / (double)m.r;
        const int ks = m.k - s;
        double de = 0.0;
        if (s > 0)
            de = (double)s * pow(err, (double)(s - 1)) * pow(1.0 - err, (double)ks);
        if (ks > 0)
            de -= (double)ks * pow(err, (double)s) * pow(1.0 - err, (double)(ks - 1));
        const double dlam_e = ck * m.pow3neg[s] * de;

        const double key = ok ? m.bins.key[idx] : 0.0;
        const double nlg = ok ? -m.bins.lgam[idx] : 0.0;
        double p = 0.0, p_c = 0.0, p_e = 0.0, p_q1 = 0.0, p_q2 = 0.0, p_q = 0.0;
        double inner = 0.0, inner_c = 0.0, inner_e = 0.0;

        for (int o0 = 1; o0 < T; o0 += OT) {
            // ---- lane-parallel preparation of up to OT*S mixture components (as direct_point_ll) ----
            const int o = o0 + og;
            const bool live = lane_in_tile && o < T;
            const double od = (double)o;
            const double x = od * lam;
            const double ex = exp_neg_rn(x);
            const double n_os = comb_s * (1.0 - ex);
            const double dn_c = comb_s * ex * od * dlam_c;
            const double dn_e = comb_s * ex * od * dlam_e;
            double tot = 0.0, dtot_c = 0.0, dtot_e = 0.0;
            for (int t = 0; t < S; ++t) {
                tot += __shfl(n_os, og * S + t, kWave);
                dtot_c += __shfl(dn_c, og * S + t, kWave);
                dtot_e += __shfl(dn_e, og * S + t, kWave);
            }
            const bool replaced = tot == 0.0; // fix_zero: a_os is the constant 0 there
            if (replaced)
                tot = 1.0;
            double a_os = n_os / tot;
            const double da_c = replaced ? 0.0 : (dn_c - a_os * dtot_c) / tot;
            const double da_e = replaced ? 0.0 : (dn_e - a_os * dtot_e) / tot;
            double b_o = 1.0, db_q1 = 0.0, db_q2 = 0.0, db_q = 0.0;
            if (P == 5) {
                const double q1 = par[2], q2 = par[3], q = par[4];
                b_o = copy_number_weight(q1, q2, q, o);
                if (o == 1) {
                    db_q1 = 1.0;
                } else if (o == 2) {
                    db_q1 = -q2;
                    db_q2 = 1.0 - q1;
                } else {
                    const double w = pow(1.0 - q, (double)(o - 3));
                    db_q1 = -(1.0 - q2) * q * w;
                    db_q2 = -(1.0 - q1) * q * w;
                    db_q = (1.0 - q1) * (1.0 - q2) * (o == 3 ? 1.0 : w - (double)(o - 3) * q * pow(1.0 - q, (double)(o - 4)));
                }
            }
            double lx = 0.0, nd = -INFINITY;
            double al_c = 0.0, be_c = 0.0, al_e = 0.0, be_e = 0.0;
            if (live && x > 0.0) {
                lx = log(x);
                nd = -log_trunc_norm(x, lx);
                const double dl = trunc_norm_dlog(x);
                al_c = da_c - a_os * dl * od * dlam_c;
                be_c = c != 0.0 ? a_os / c : a_os * od * dlam_c / x;
                al_e = da_e - a_os * dl * od * dlam_e;
                be_e = a_os * od * dlam_e / x;
            }
            if (!live)
                a_os = 0.0;
            // a component that weighs nothing and whose weight does not move is skipped (NaN falls through, as in K-direct)
            const int use = (live && !(a_os == 0.0 && al_c == 0.0 && al_e == 0.0)) ? 1 : 0;

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
                }
                if ((i + 1) % S == 0) { // end of one copy-number class
                    const double b_i = wave_bcast(b_o, i);
                    p += b_i * inner;
                    p_c += b_i * inner_c;
                    p_e += b_i * inner_e;
                    if (P == 5) {
                        p_q1 += wave_bcast(db_q1, i) * inner;
                        p_q2 += wave_bcast(db_q2, i) * inner;
                        p_q += wave_bcast(db_q, i) * inner;
                    }
                    inner = inner_c = inner_e = 0.0;
                }
            }
        }

        // ---- key epilogue ----
        if (ok) {
            const double dp[5] = {p_c, p_e, p_q1, p_q2, p_q};
            const double h = m.bins.cnt[idx];
            sum[1].add(p);
#pragma unroll
            for (int d = 0; d < P; ++d)
                sum[2 + P + d].add(dp[d]);
            if (h != 0.0) {
                const double term = h * ((p <= 0.0) ? -INFINITY : log(p));
                if (term - term == 0.0) // finite
                    sum[0].add(term);
                else
                    special += term;
#pragma unroll
                for (int d = 0; d < P; ++d)
                    sum[2 + d].add(h * dp[d] / p);
            }
        }
    }

    // ---- the workgroup's sums: lanes by butterfly, waves in ascending order ----
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const CompSum r = wave_comp_reduce(sum[q]);
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
            for (int w = 0; w < kGradWaves; ++w)
                comp_merge(r, red[w][2 * q], red[w][2 * q + 1]);
            out[2 * q] = r.hi;
            out[2 * q + 1] = r.lo;
        } else {
            double r = 0.0;
            for (int w = 0; w < kGradWaves; ++w)
                r += red[w][2 * NQ];
            out[2 * NQ] = r;
        }
    }
}

// One workgroup a point: thread q adds quantity q over the point's segments in ascending order; threads 0 .. P - 1 then
// form LL = sum h log p + tail log(1 - sp) and dLL = sum h dp/p - [tail != 0 and sp < 1] tail (sum dp) / (1 - sp).
// A component whose parameter the clamp moved is 0; where LL is not finite every component is NaN.
template <int P>
__global__ __launch_bounds__(kWave) void ll_grad_finish_kernel(const DevModel m, const PointSource src, int n_seg,
                                                               const double *__restrict__ partial, double *__restrict__ out_ll,
                                                               double *__restrict__ out_grad)
{
    constexpr int NQ = GradLayout<P>::kSums, STRIDE = GradLayout<P>::kStride;
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
    if (q < P) {
        double raw[kMaxParams], par[kMaxParams];
        int T;
        fetch_point<P>(src, pt, raw, T);
#pragma unroll
        for (int d = 0; d < P; ++d)
            par[d] = raw[d];
        clamp_point<P>(m, par);
        double ll = tot[0] + tot[NQ];
        double g = tot[2 + q];
        if (m.tail != 0.0) { // tail * log(1 - min(1, sp)), covest/models.py:103-105
            double sp = tot[1];
            if (!(sp < 1.0))
                sp = 1.0;
            if (sp < 1.0) {
                ll += m.tail * log(1.0 - sp);
                g -= m.tail * tot[2 + P + q] / (1.0 - sp);
            }
        }
        bool moved = false;
#pragma unroll
        for (int d = 0; d < P; ++d)
            if (d == q)
                moved = par[d] != raw[d];
        if (moved)
            g = 0.0;
        if (!(ll - ll == 0.0))
            g = NAN;
        out_grad[pt * P + q] = g;
        if (q == 0)
            out_ll[pt] = ll;
    }
}

} // namespace

int ll_grad_segments(const DevModel &m)
{
    const int64_t n = (m.bins.n + kGradSegKeys - 1) / kGradSegKeys;
    return n < 1 ? 1 : (int)n;
}

size_t ll_grad_partial_bytes(const DevModel &m, int64_t n)
{
    const int64_t pts = n < kGradPointsPerLaunch ? n : kGradPointsPerLaunch;
    const int stride = m.kind == 0 ? GradLayout<2>::kStride : GradLayout<5>::kStride;
    return (size_t)pts * (size_t)ll_grad_segments(m) * (size_t)stride * sizeof(double);
}

hipError_t launch_ll_grad(const DevModel &m, const PointSource &src, int64_t n, double *partial, double *out_ll,
                          double *out_grad, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    if (src.is_grid)
        return hipErrorInvalidValue;
    const int n_seg = ll_grad_segments(m);
    const int P = m.kind == 0 ? 2 : 5;
    for (int64_t first = 0; first < n; first += kGradPointsPerLaunch) {
        const int64_t cnt = n - first < kGradPointsPerLaunch ? n - first : kGradPointsPerLaunch;
        PointSource part = src;
        part.params = src.params + first * P;
        part.t_list = src.t_list ? src.t_list + first : nullptr;
        const dim3 grid((unsigned)n_seg, (unsigned)cnt), block(kGradWaves * kWave);
        if (P == 2) {
            hipLaunchKernelGGL((ll_grad_kernel<2>), grid, block, 0, stream, m, part, partial);
            hipLaunchKernelGGL((ll_grad_finish_kernel<2>), dim3((unsigned)cnt), dim3(kWave), 0, stream, m, part, n_seg, partial,
                               out_ll + first, out_grad + first * P);
        } else {
            hipLaunchKernelGGL((ll_grad_kernel<5>), grid, block, 0, stream, m, part, partial);
            hipLaunchKernelGGL((ll_grad_finish_kernel<5>), dim3((unsigned)cnt), dim3(kWave), 0, stream, m, part, n_seg, partial,
                               out_ll + first, out_grad + first * P);
        }
    }
    return hipGetLastError();
}

} // namespace covest
