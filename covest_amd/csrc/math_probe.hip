// math_probe.hip -- covest_math_probe of the C ABI: a DIAGNOSTIC that evaluates the scalar primitives every likelihood
// kernel stands on (fastmath.h, point_fetch.h, grad_common.h), one element a thread, so that a test can hold each of
// them to a bit-exact restatement and to a 50-digit value (tests/test_gpu_math.py, tests/math_reference.py).  The
// functions are called from the headers as they stand -- nothing is restated here -- and the table reaches them as it
// reaches the kernels: load_log_table into LDS, then a barrier.  One launch of 256-thread workgroups a call.  The launch
// is entered neither in the launch records nor in covest_compiled_variants.
#include "host.h"

#include "fastmath.h"
#include "grad_common.h"
#include "point_fetch.h"
#include "tiles.h"

namespace covest {

namespace {

// the values of `fn` (include/covest_amd.h; named once more in covest_amd/_capi.py MATH_PROBE_FN)
enum ProbeFn : int32_t {
    kProbeExpFast = 0,
    kProbeExpScaled,
    kProbeExpLibrary,
    kProbeExpNegRn,
    kProbeFastLog,
    kProbeFastLogN4,
    kProbeLogBits1Deg5Basic,
    kProbeLogBits4Deg5Scale,
    kProbeLogBits4Deg3ScaleRaw,
    kProbeLogBits4Deg4Scale,
    kProbeLogTruncNorm,
    kProbeLogTruncNormTable,
    kProbeTruncNormDlog,
    kProbeTruncNormDlog2First,
    kProbeTruncNormDlog2Second,
    kProbeRatePow,
    kProbeRateMul8,
    kProbeRateMul16,
    kProbeRates8,
    kProbeRates16,
    kProbeWeightPow,
    kProbeWeightSquaring,
    kProbeFnCount
};

constexpr int64_t kProbeMaxN = 65536;
constexpr int kProbeGroup = 4; // elements a thread takes in the four-at-a-time functions; the staged arrays are padded to it

bool four_at_a_time(int32_t fn)
{
    return fn == kProbeFastLogN4 || fn == kProbeLogBits4Deg5Scale || fn == kProbeLogBits4Deg3ScaleRaw ||
           fn == kProbeLogBits4Deg4Scale;
}

template <int S>
__device__ __forceinline__ double rates_class(const DevModel &m, double c, double err, int s)
{
    double lam[S];
    error_class_rates<S>(m, c, err, lam);
    double v = lam[0];
#pragma unroll
    for (int t = 1; t < S; ++t)
        v = t == s ? lam[t] : v;
    return v;
}

// m: only k, r and pow3neg are read.  np: n rounded up to a multiple of kProbeGroup, the length of every staged array.
__global__ __launch_bounds__(256) void math_probe_kernel(const DevModel m, const int32_t fn, const int32_t n, const int32_t np,
                                                         const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ z, const int32_t *__restrict__ iarg,
                                                         double *__restrict__ out)
{
    __shared__ double log_tab[kLogTableDoubles];
    load_log_table(log_tab);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (fn == kProbeFastLogN4 || fn == kProbeLogBits4Deg5Scale || fn == kProbeLogBits4Deg3ScaleRaw ||
        fn == kProbeLogBits4Deg4Scale) {
        const int first = i * kProbeGroup; // a thread takes four consecutive inputs
        if (first >= np)
            return;
        const double in4[kProbeGroup] = {x[first], x[first + 1], x[first + 2], x[first + 3]};
        double lg4[kProbeGroup];
        if (fn == kProbeFastLogN4)
            fast_log_n<4>(in4, lg4, log_tab);
        else if (fn == kProbeLogBits4Deg5Scale)
            fast_log_bits_n<4, 5, kScaleBits, false>(in4, lg4, log_tab);
        else if (fn == kProbeLogBits4Deg3ScaleRaw)
            fast_log_bits_n<4, 3, kScaleBits, true>(in4, lg4, log_tab);
        else
            fast_log_bits_n<4, 4, kScaleBits, false>(in4, lg4, log_tab);
#pragma unroll
        for (int k = 0; k < kProbeGroup; ++k)
            out[first + k] = lg4[k];
        return;
    }
    if (i >= n)
        return;
    const double a = x[i], b = y[i], c = z[i];
    const int ia = iarg[i];
    double v = 0.0;
    switch (fn) {
    case kProbeExpFast:
        v = exp_fast(a);
        break;
    case kProbeExpScaled:
        v = exp_scaled(a, ia);
        break;
    case kProbeExpLibrary:
        v = exp(a);
        break;
    case kProbeExpNegRn:
        v = exp_neg_rn(a);
        break;
    case kProbeFastLog:
        v = fast_log(a, log_tab);
        break;
    case kProbeLogBits1Deg5Basic: {
        const double in1[1] = {a};
        double lg1[1];
        fast_log_bits_n<1, 5, kBasicShift>(in1, lg1, log_tab);
        v = lg1[0];
        break;
    }
    case kProbeLogTruncNorm:
        v = log_trunc_norm(a, b);
        break;
    case kProbeLogTruncNormTable:
        v = log_trunc_norm(a, b, log_tab);
        break;
    case kProbeTruncNormDlog:
        v = trunc_norm_dlog(a);
        break;
    case kProbeTruncNormDlog2First:
    case kProbeTruncNormDlog2Second: {
        double d1, d2;
        trunc_norm_dlog2(a, d1, d2);
        v = fn == kProbeTruncNormDlog2First ? d1 : d2;
        break;
    }
    case kProbeRatePow:
        v = error_class_rate(m, a, b, ia);
        break;
    case kProbeRateMul8:
        v = error_class_rate_mul(m, a, b, ia, 8);
        break;
    case kProbeRateMul16:
        v = error_class_rate_mul(m, a, b, ia, 16);
        break;
    case kProbeRates8:
        v = rates_class<8>(m, a, b, ia);
        break;
    case kProbeRates16:
        v = rates_class<16>(m, a, b, ia);
        break;
    case kProbeWeightPow:
        v = copy_number_weight(a, b, c, ia);
        break;
    case kProbeWeightSquaring:
        v = copy_number_weight_by_squaring(a, b, c, ia);
        break;
    default:
        break;
    }
    out[i] = v;
}

// what `fn` reads beside x
struct ProbeNeeds {
    bool y, z, iarg, model;
    int classes; // rates: iarg is a class in [0, classes)
};

ProbeNeeds needs_of(int32_t fn)
{
    switch (fn) {
    case kProbeExpScaled:
        return {false, false, true, false, 0};
    case kProbeLogTruncNorm:
    case kProbeLogTruncNormTable:
        return {true, false, false, false, 0};
    case kProbeRatePow:
        return {true, false, true, true, kMaxErr};
    case kProbeRateMul8:
    case kProbeRates8:
        return {true, false, true, true, 8};
    case kProbeRateMul16:
    case kProbeRates16:
        return {true, false, true, true, 16};
    case kProbeWeightPow:
    case kProbeWeightSquaring:
        return {true, true, true, false, 0};
    default:
        return {false, false, false, false, 0};
    }
}

} // namespace

} // namespace covest

extern "C" {

int covest_math_probe(int32_t device, int32_t fn, int64_t n, const double *x, const double *y, const double *z,
                      const int32_t *iarg, int32_t k, int32_t r, double *out)
{
    if (fn < 0 || fn >= kProbeFnCount)
        return fail(COVEST_E_INVALID, "covest_math_probe: unknown function");
    if (n < 0 || n > kProbeMaxN)
        return fail(COVEST_E_INVALID, "covest_math_probe: n must be in 0..65536");
    const ProbeNeeds needs = needs_of(fn);
    if (n > 0 && (!x || !out || (needs.y && !y) || (needs.z && !z) || (needs.iarg && !iarg)))
        return fail(COVEST_E_INVALID, "covest_math_probe: a null array this function reads or writes");
    if (needs.model && (k < 1 || k >= kMaxErr || r < k))
        return fail(COVEST_E_INVALID, "covest_math_probe: k must be in 1..63 and r >= k");
    for (int64_t i = 0; i < n && needs.iarg; ++i) {
        const int32_t v = iarg[i];
        const bool ok = needs.model            ? v >= 0 && v < needs.classes
                        : fn == kProbeExpScaled ? v >= -2048 && v <= 2048
                                                : v >= 1 && v <= kMaxFastKey; // a copy number
        if (!ok)
            return fail(COVEST_E_INVALID, "covest_math_probe: iarg outside the function's range "
                                          "(class: 0..S-1; scale: -2048..2048; copy number: 1..16384)");
    }
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_math_probe");
    COVEST_TRY(call.status());

    DevModel dm{};
    dm.k = k, dm.r = r;
    for (int s = 0; s < kMaxErr; ++s)
        dm.pow3neg[s] = std::pow(3.0, (double)-s); // as covest_model_create forms it (abi_model.cpp)

    // staged: x | y | z (np doubles each) | iarg (np ints); padded with harmless values up to a multiple of four
    const int64_t np = (n + kProbeGroup - 1) / kProbeGroup * kProbeGroup;
    const size_t in_bytes = (size_t)np * (3 * sizeof(double) + sizeof(int32_t)), out_bytes = (size_t)np * sizeof(double);
    DevBuf d_in, d_out;
    HIP_TRY(d_in.reserve(in_bytes));
    HIP_TRY(d_out.reserve(out_bytes));
    {
        SharedStage &ss = shared_stage();
        std::lock_guard<std::mutex> hold(ss.mu);
        HIP_TRY(ss.buf.reserve(in_bytes));
        double *sx = ss.buf.as<double>(), *sy = sx + np, *sz = sy + np;
        int32_t *si = reinterpret_cast<int32_t *>(sz + np);
        for (int64_t i = 0; i < np; ++i) {
            const bool in = i < n;
            sx[i] = in ? x[i] : 1.0;
            sy[i] = in && y ? y[i] : 0.0;
            sz[i] = in && z ? z[i] : 0.0;
            si[i] = in && iarg ? iarg[i] : 0;
        }
        HIP_TRY(hipMemcpy(d_in.ptr, ss.buf.ptr, in_bytes, hipMemcpyHostToDevice));
    }
    const double *dx = d_in.as<double>(), *dy = dx + np, *dz = dy + np;
    const int32_t *di = reinterpret_cast<const int32_t *>(dz + np);
    const int64_t threads = four_at_a_time(fn) ? np / kProbeGroup : n;
    const dim3 block(256), grid((unsigned)((threads + 255) / 256));
    hipLaunchKernelGGL(math_probe_kernel, grid, block, 0, nullptr, dm, fn, (int32_t)n, (int32_t)np, dx, dy, dz, di,
                       d_out.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.ptr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
