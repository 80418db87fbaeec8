// abi_tp.cpp -- covest_truncated_poisson and covest_truncated_poisson_table of the C ABI over tp_eval.hip: the
// counterpart of the reference's importable extension, covest_poisson.truncated_poisson (c_src/covest_poissonmodule.c:7-35).
// No model handle: the calls stage what they send in the process's page-locked block (host.h SharedStage).
#include "host.h"

using namespace covest;

namespace {

constexpr int64_t kTpMaxKey = (int64_t)1 << 22; // the ln j! table's reach (host_common.cpp)

// rate | key | ln key! | ln m!, m = min(key, floor(rate)): the four input arrays of tp_pairs_kernel, n doubles each
void stage_pairs(double *dst, int64_t n, const double *l, const int64_t *j)
{
    for (int64_t i = 0; i < n; ++i) {
        const double x = l[i];
        const int64_t m = x >= 1.0 ? (int64_t)std::min((double)j[i], std::floor(x)) : 0; // (NaN: 0; never read)
        dst[i] = x;
        dst[n + i] = (double)j[i];
        dst[2 * n + i] = lgamma_at(j[i]);
        dst[3 * n + i] = lgamma_at(m);
    }
}

// The tile table of the recurrence over a key list: a throw-away model handle whose bins are the keys, each with a
// count (so that every tile is a plain item) and its position in the list as its index -- build_tiles as it stands.
int tiles_over_keys(covest_model &tmp, int64_t n_j, const int64_t *keys)
{
    std::vector<HostBin> bins((size_t)n_j);
    for (int64_t b = 0; b < n_j; ++b)
        bins[(size_t)b] = HostBin{(int)keys[b], 1.0, (int32_t)b};
    lgamma_ensure(keys[n_j - 1]);
    const int rc = build_tiles(&tmp, std::move(bins));
    if (rc != COVEST_OK)
        return rc;
    if (!tmp.has_tiles)
        return fail(COVEST_E_INVALID, "covest_truncated_poisson_table: no tile table over these keys");
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_truncated_poisson(int32_t device, int64_t n, const double *l, const int64_t *j, int32_t mode, double *out)
{
    if (n < 0 || (n > 0 && (!l || !j || !out)))
        return fail(COVEST_E_INVALID, "covest_truncated_poisson: bad argument");
    if (mode != kTpValue && mode != kTpReference && mode != kTpLog)
        return fail(COVEST_E_INVALID, "covest_truncated_poisson: unknown mode");
    if (n > kTpMaxPairs)
        return fail(COVEST_E_INVALID, "covest_truncated_poisson: more than 2^30 pairs in one call");
    int64_t j_max = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (j[i] < 1 || j[i] > kTpMaxKey)
            return fail(COVEST_E_INVALID, "covest_truncated_poisson: j must be in 1..4194304");
        j_max = std::max(j_max, j[i]);
    }
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_truncated_poisson");
    COVEST_TRY(call.status());
    lgamma_ensure(j_max); // as a model does for its keys: one lock for the whole call

    const size_t in_bytes = (size_t)n * 4 * sizeof(double), out_bytes = (size_t)n * sizeof(double);
    SharedStage &ss = shared_stage();
    if (n <= kInPlaceMaxPoints) {
        // a short list moves nothing through the copy engine: read, and its values written, in place in the mapped block
        std::lock_guard<std::mutex> hold(ss.mu);
        HIP_TRY(ss.buf.reserve(in_bytes + out_bytes));
        double *in = ss.buf.as<double>(), *res = in + 4 * n;
        stage_pairs(in, n, l, j);
        HIP_TRY(launch_tp_pairs(mode, n, in, res, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        std::memcpy(out, res, out_bytes);
        return COVEST_OK;
    }
    DevBuf d_in, d_out; // (released after the staging lock: another handle's upload does not wait for the kernel)
    HIP_TRY(d_in.reserve(in_bytes));
    HIP_TRY(d_out.reserve(out_bytes));
    {
        std::lock_guard<std::mutex> hold(ss.mu);
        HIP_TRY(ss.buf.reserve(in_bytes));
        stage_pairs(ss.buf.as<double>(), n, l, j);
        HIP_TRY(hipMemcpy(d_in.ptr, ss.buf.ptr, in_bytes, hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_tp_pairs(mode, n, d_in.as<double>(), d_out.as<double>(), nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, out_bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_truncated_poisson_table(int32_t device, int64_t n_l, const double *l, int64_t n_j, const int64_t *j, double *out)
{
    if (n_l < 0 || n_j < 0 || (n_l > 0 && !l) || (n_j > 0 && !j) || (n_l > 0 && n_j > 0 && !out))
        return fail(COVEST_E_INVALID, "covest_truncated_poisson_table: bad argument");
    for (int64_t b = 0; b < n_j; ++b)
        if (j[b] < 1 || j[b] > kMaxFastKey || (b > 0 && j[b] <= j[b - 1]))
            return fail(COVEST_E_INVALID, "covest_truncated_poisson_table: keys must be strictly ascending integers in 1..16384");
    if (n_l > ((int64_t)1 << 30))
        return fail(COVEST_E_INVALID, "covest_truncated_poisson_table: more than 2^30 rates in one call");
    if (n_l == 0 || n_j == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_truncated_poisson_table");
    COVEST_TRY(call.status());

    covest_model tmp; // (owns the tile table's device buffer; goes with the call)
    tmp.device = call.device();
    COVEST_TRY(tiles_over_keys(tmp, n_j, j));
    const size_t l_bytes = (size_t)n_l * sizeof(double), out_bytes = (size_t)n_l * (size_t)n_j * sizeof(double);
    DevBuf d_l, d_out;
    HIP_TRY(d_l.reserve(l_bytes));
    HIP_TRY(d_out.reserve(out_bytes));
    {
        SharedStage &ss = shared_stage();
        std::lock_guard<std::mutex> hold(ss.mu);
        HIP_TRY(ss.buf.reserve(l_bytes));
        std::memcpy(ss.buf.ptr, l, l_bytes);
        HIP_TRY(hipMemcpy(d_l.ptr, ss.buf.ptr, l_bytes, hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_tp_table(tmp.tv, n_l, d_l.as<double>(), n_j, d_out.as<double>(), nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, out_bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
