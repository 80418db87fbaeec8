// fastmath.h -- fp64 log for the per-bin term h_j * log(p_j) of the fast kernels.
//
// The device library's log costs ~72 FMA-issue slots on gfx950 (tools/
// microbench_f64.hip) -- it became the dominant cost once a pmf term is down to 2
// instructions.  The log-likelihood needs log(p_j) to an ABSOLUTE accuracy of a few
// 1e-16 (it is summed with weights h_j into a total whose terms all have the same
// sign), so: exponent/mantissa split (v_frexp_*), a 256-entry table {1/c, log c'}
// in LDS (4 KB) indexed by the top 8 mantissa bits, r = fma(m, 1/c, -1) with |r| <= 2^-9,
// and log1p(r) to r^5 (a 64-entry table needs r^7: two more FMAs per log).  ~16 instructions.
// Error, for every finite x > 0 with binary exponent e (derived in tests/math_reference.py, held on the device by
// tests/test_gpu_math.py, which also holds every bit to a restatement in exact arithmetic):
//     |fast_log(x) - log x| <= 2^-54 / 6 + 2^-52 |log x| + |fl(ln 2) - ln 2| |e| + 2^-53
// -- the truncation r^6 / 6, the two roundings at the result's magnitude, the constant's own error (2.3e-17) once per
// unit of the exponent, the table entry's rounding: 1.2e-16 near x = 1, 3.5e-16 at x = 0.5, 2.2e-16 |log x| + 2.3e-17 |e|
// where |log x| is large (1.3e-13 at x = 2^-1000, 1.9e-16 of the value).  The "absolute 2e-16" this header used to
// state holds for |log x| <= 0.4 only.  Measured worst share of that bar: 0.82 (profiles/math_primitives.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "log_table.h"

namespace covest {

constexpr int kLogTableDoubles = 2 << kLogTableBits;

// Copy the table into this workgroup's LDS (call from all threads, then barrier).
__device__ __forceinline__ void load_log_table(double *tab_lds)
{
    for (int i = threadIdx.x; i < kLogTableDoubles; i += blockDim.x)
        tab_lds[i] = kLogTable[i];
}

// d = a * b + c with the coefficient c in an SGPR pair, as the three-address VOP3 instruction.
// Left to itself the compiler keeps the Horner coefficients in VGPRs, picks the two-address
// v_fmac_f64 and copies the coefficient into the destination first -- 7 extra full-rate slots
// per log (16% of K-basic).  A scalar operand costs nothing and frees the VGPRs.
__device__ __forceinline__ double fma_vvs(double a, double b, double c)
{
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}

// d = a * b + c as the three-address instruction with every operand in vector registers: where d is a LOOP-CARRIED value
// and c a freshly loaded one the compiler takes v_fmac_f64 into c's register and copies the result back (a v_mov_b64, one
// full-rate slot, per Horner step of K-factored's shared steps).
__device__ __forceinline__ double fma_vvv(double a, double b, double c)
{
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// exp(x) 2^sc: the device library's algorithm (ocml expD: x = n ln 2 + t by Cody-Waite, a degree-11 polynomial in t,
// |t| <= 0.347, ldexp) with its OWN coefficients, written so that none of them lives in a vector register.  Inlined from
// the library the eleven coefficients are loop invariants that the compiler parks in 22 VGPRs for the whole key walk of
// a recurrence kernel (and copies into the v_fmac destination before every use, a full-rate v_mov_b64 each): a sixth
// of K-basic's register file -- round 5, found in the ISA of ll_basic_kernel<true>, which spilled 266 registers.  Here
// every coefficient is a scalar operand of a three-address v_fma_f64 (the scalar unit re-creates it with two s_mov).
// The power of two is applied by the final v_ldexp_f64 -- exactly, one rounding in all, where the result is a normal
// double -- so a caller that wants exp(x) 2^540 (streams.h) no longer adds ln 2^540 to the argument or scales twice.
// x = -inf gives +0 and NaN propagates.  For |x| <= 1e15 a result beyond the doubles' range is +inf, one below it +0
// (with that sign), and a subnormal one is rounded once more by v_ldexp_f64 onto the 4.9e-324 grid: up to there the
// remainder t = x - dn ln 2 stays within ln 2 / 2 + 2.3e-16 |x| <= 0.58, where the polynomial is positive, and the
// ldexp decides alone.  The library's range guards are NOT here, so beyond that t is no longer small and the
// polynomial's sign and size decide: exp_scaled(-1e20) = -0.0 (a zero of the wrong sign), exp_scaled(1e300) = -inf,
// exp_scaled(-1e300) = +inf, exp_scaled(+inf) = NaN -- pinned by tests/test_gpu_math.py, bit-equal to the restatement
// in tests/math_reference.py.  What callers can reach: exp_scaled(a0, kScaleBits) is used only for a log-term inside
// the window, -760 < a0, and a0 is the log of a mixture term, far below 709.78 - 374.3 (streams.h enter_tile_n; the
// lanes whose result is discarded may pass anything, -inf included); exp_fast(-xr) of log_trunc_norm has xr in [1, 200];
// exp_neg_rn(x) has x = o lambda_s with o <= 16384 and lambda_s <= the coverage, which the basic model bounds by
// max_cov and the repeats model by nothing (clamp_point) -- but the normaliser the same x goes through is defined up
// to x = 200 x 2^53 = 1.8e18 only (log_trunc_norm; covest_truncated_poisson accepts any rate), and the reference does
// not return beyond 2^61.  Between 1e15 and 1.8e18 the one deviation is the -0.0 above, and exp_neg_rn's callers form
// 1.0 - exp_neg_rn(x) or products with it, which cannot see the sign of a zero.  So nothing here is guarded: the two
// selects would cost every anchor of every recurrence kernel two compares for arguments no defined result depends on.
// Accuracy inside the range: 0.78 ulp at sc = 0 and 0.71 ulp at sc = kScaleBits over the inputs of tests/test_gpu_math.py,
// the device library's own exp 0.78 and 0.71 ulp on the same inputs (profiles/math_primitives.txt).
__device__ __forceinline__ double exp_scaled(double x, int sc)
{

    const double dn = __builtin_rint(x * 0x1.71547652b82fep+0);
    double t = fma(-dn, 0x1.62e42fefa39efp-1, x);
    t = fma(-dn, 0x1.abc9e3b39803fp-56, t);
    // (the first Horner step as two instructions with one scalar operand each -- gfx950's VOP3 reads ONE scalar pair --
    // behind asm: left to the compiler the pair is contracted into a v_fmac whose addend is hoisted into a VGPR pair)
    double p;
    asm("v_mul_f64 %0, %1, %2" : "=v"(p) : "v"(t), "s"(0x1.ade156a5dcb37p-26));
    asm("v_add_f64 %0, %1, %2" : "=v"(p) : "v"(p), "s"(0x1.28af3fca7ab0cp-22));
    p = fma_vvs(t, p, 0x1.71dee623fde64p-19);
    p = fma_vvs(t, p, 0x1.a01997c89e6b0p-16);
    p = fma_vvs(t, p, 0x1.a01a014761f6ep-13);
    p = fma_vvs(t, p, 0x1.6c16c1852b7b0p-10);
    p = fma_vvs(t, p, 0x1.1111111122322p-7);
    p = fma_vvs(t, p, 0x1.55555555502a1p-5);
    p = fma_vvs(t, p, 0x1.5555555555511p-3);
    p = fma_vvs(t, p, 0x1.000000000000bp-1);
    p = fma(t, p, 1.0);
    p = fma(t, p, 1.0);
    // (keeps n + sc inside the ints; |dn| beyond 4096 means |x| beyond 2839, where p 2^(+-4096 + sc) is 0 or +-inf
    // for any finite p != 0 -- the SIGN is p's, see above)
    const int n = (int)fmin(fmax(dn, -4096.0), 4096.0);
    const double z = ldexp(p, n + sc);
    return x == -INFINITY ? 0.0 : z;
}

__device__ __forceinline__ double exp_fast(double x) { return exp_scaled(x, 0); }

// log(x) for finite x > 0 (subnormals included).  NaN propagates.  x == 0 gives a finite
// value (callers handle p_j <= 0 themselves).
__device__ __forceinline__ double fast_log(double x, const double *tab_lds)
{
    const double m = __builtin_amdgcn_frexp_mant(x); // [0.5, 1)
    const int e = __builtin_amdgcn_frexp_exp(x);
    // byte offset of the 16-byte entry: the top kLogTableBits mantissa bits
    const unsigned off = __builtin_amdgcn_ubfe((unsigned)__double2hiint(m), 20 - kLogTableBits, kLogTableBits) << 4;
    const double2 ent = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(tab_lds) + off);
    const double r = fma(m, ent.x, -1.0); // |r| <= 2^-(kLogTableBits + 1)
    double q;
    if (kLogTableBits >= 8) { // |r| <= 2^-9: log1p(r) to r^5, truncation r^6/6 < 2^-56
        q = fma_vvs(r, 0.2, -0.25);
    } else { // |r| <= 2^-7: to r^7, truncation r^8/8 < 2^-59
        q = fma_vvs(r, 1.0 / 7.0, -1.0 / 6.0);
        q = fma_vvs(r, q, 0.2);
        q = fma_vvs(r, q, -0.25);
    }
    q = fma_vvs(r, q, 1.0 / 3.0);
    q = fma(r, q, -0.5);
    const double lp = fma(r * r, q, r); // log1p(r)
    return fma((double)e, 0.693147180559945309417232121458, ent.y) + lp;
}

// The raw instruction: llvm's fmax quiets its operands first (a v_max_f64 x, x, x each) -- two extra full-rate
// slots per log for a NaN nobody feeds it (a NaN parameter poisons the result by other means).
__device__ __forceinline__ double max_raw(double a, double b)
{
    double d;
    asm("v_max_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// N logs at once, written stage by stage so that the N table reads are in flight together and the N dependent
// chains interleave: one log after the other exposes the LDS latency and the latency of every FMA of its chain,
// which two waves per SIMD do not hide (ll_factored.hip).
template <int N>
__device__ __forceinline__ void fast_log_n(const double (&x)[N], double (&out)[N], const double *tab_lds)
{
    double m[N], r[N], q[N], lp[N];
    int e[N];
    double2 ent[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        m[k] = __builtin_amdgcn_frexp_mant(x[k]);
        e[k] = __builtin_amdgcn_frexp_exp(x[k]);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned off = __builtin_amdgcn_ubfe((unsigned)__double2hiint(m[k]), 20 - kLogTableBits, kLogTableBits) << 4;
        ent[k] = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(tab_lds) + off);
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        r[k] = fma(m[k], ent[k].x, -1.0);
    static_assert(kLogTableBits >= 8, "log1p to r^5 needs |r| <= 2^-9");
#pragma unroll
    for (int k = 0; k < N; ++k)
        q[k] = fma_vvs(r[k], 0.2, -0.25);
#pragma unroll
    for (int k = 0; k < N; ++k)
        q[k] = fma_vvs(r[k], q[k], 1.0 / 3.0);
#pragma unroll
    for (int k = 0; k < N; ++k)
        q[k] = fma(r[k], q[k], -0.5);
#pragma unroll
    for (int k = 0; k < N; ++k)
        lp[k] = fma(r[k] * r[k], q[k], r[k]);
#pragma unroll
    for (int k = 0; k < N; ++k)
        out[k] = fma((double)e[k], 0.693147180559945309417232121458, ent[k].y) + lp[k];
}

// N logs of POSITIVE doubles scaled by 2^SC, log(x 2^-SC): fast_log_n with the 2^-SC folded into the exponent
// arithmetic -- the exponent comes off the bits with a shift and an add (two half-rate integer instructions, the
// price of v_frexp_exp_i32_f64 alone), so the scale costs nothing; x must be a NORMAL double (the callers clamp).
// (Taking the mantissa off the bits too -- and, or -- was tried: the compiler copies the low word into a fresh
// register pair for it, v_frexp_mant_f64 is cheaper.)  DEG: log1p(r) to r^DEG, |r| <= 2^-9.  The error is fast_log's
// bound with log(x 2^-SC) for log x, the exponent e that multiplies ln 2 here, and the truncation T_DEG for 2^-54 / 6:
// 5 -> T_5 = 2^-54 / 6 = 9.3e-18 (as fast_log); 4 -> T_4 = 2^-45 / 5 + T_5 = 5.69e-15, zero-mean over the mantissa (odd
// in r) -- one FMA less per log (no kernel instantiates it; the test does); 3 (round 5, dense grids: ll_factored.hip)
// -> another FMA less: r - (1/2 + d) r^2 + r^3 / 3 with d = 0.2071 x 2^-18 chosen so that d r^2 - r^4 / 4
// equioscillates over |r| <= 2^-9 -- T_3 = (1/4 - 0.2071) 2^-36 + 2^-45 / 5 + T_5 = 6.30e-13 (the restatement in exact
// arithmetic reaches 6.25e-13 on [0.5, 1); 3.6e-12 for the plain Taylor cubic), against sums whose terms are
// |log p_j| >= 1 and a parity bar of 1e-9.  Measured worst shares of these bars: 0.87 (5), 0.85 (4), 0.97 (3).
// RAW (DEG 3 only): the exponent is not un-biased -- the result is log(x 2^-SC) + (1022 + SC) ln 2, one integer
// subtract less per log, with the same bound (e is then the biased exponent, up to 2046).  The caller takes the
// constant kLogRawBias<SC> off once per SUM (h_j kLogRawBias summed over the counted keys is a constant of the
// histogram); that double is off the real (1022 + SC) ln 2 by its own rounding and 1562 times fl(ln 2)'s error:
// 6.97e-14 at SC = 540 (bound 1.5e-13), the same for every key, so 7e-14 relative to a sum of |log p_j| >= 1.
template <int SC>
constexpr double kLogRawBias = (double)(1022 + SC) * 0.693147180559945309417232121458;
template <int N, int DEG, int SC, bool RAW = false>
__device__ __forceinline__ void fast_log_bits_n(const double (&x)[N], double (&out)[N], const double *tab_lds)
{
    static_assert(kLogTableBits == 8, "table offset below takes the top 8 mantissa bits");
    static_assert(DEG == 3 || DEG == 4 || DEG == 5, "log1p degree");
    double m[N], r[N], q[N], lp[N];
    int e[N];
    double2 ent[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int hi = __double2hiint(x[k]);
        e[k] = RAW ? (hi >> 20) : (hi >> 20) - (1022 + SC);
        m[k] = __builtin_amdgcn_frexp_mant(x[k]); // [0.5, 1): the mantissa bits are x's own
        const unsigned off = ((unsigned)hi >> 8) & 0xFF0u;
        ent[k] = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(tab_lds) + off);
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        r[k] = fma(m[k], ent[k].x, -1.0);
    if (DEG == 5) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = fma_vvs(r[k], 0.2, -0.25);
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = fma_vvs(r[k], q[k], 1.0 / 3.0);
    } else if (DEG == 4) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = fma_vvs(r[k], -0.25, 1.0 / 3.0);
    }
    if (DEG == 3) {
#pragma unroll
        for (int k = 0; k < N; ++k) // (1/3 in a vector register pair, as -1/4 was for degree 4: VOP3 reads ONE scalar pair)
            q[k] = fma_vvs(r[k], 1.0 / 3.0, -(0.5 + 0.20710678118654752 * 0x1p-18));
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            q[k] = fma(r[k], q[k], -0.5);
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        lp[k] = fma(r[k] * r[k], q[k], r[k]);
#pragma unroll
    for (int k = 0; k < N; ++k)
        out[k] = fma((double)e[k], 0.693147180559945309417232121458, ent[k].y) + lp[k];
}

} // namespace covest
