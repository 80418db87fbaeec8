// abi_posterior.cpp -- covest_posterior_classes of the C ABI over posterior.hip: per key of the model, the log of p_j and
// the posterior shares of the error classes and the copy numbers.  On the pattern of
// covest_probabilities (abi_model.cpp): the model's lock and device, the all-keys view, thresholds by the host rule, NaN
// bounds where the point is taken as given.  Neither launch is entered in the model's launch record.
#include "host.h"
#include "posterior.h"

using namespace covest;

namespace {

constexpr size_t kPostChunkBytes = (size_t)64 << 20; // a chunk's table and its results on the device
constexpr int64_t kPostChunkPoints = 4096;           // ... and its points at most (a launch's grid y stays below 65536)

// rows x live doubles from `src` into rows of row_len at `dst`; what lies behind the live columns is 0, or NaN in the
// row of a key that has no posterior (log_p[row] is -inf or NaN: every share of the row is NaN)
void widen_rows(double *dst, const double *src, const double *log_p, size_t rows, size_t live, size_t row_len)
{
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(dst + r * row_len, src + r * live, live * sizeof(double));
        const bool none = !(log_p[r] > -std::numeric_limits<double>::infinity());
        std::fill(dst + r * row_len + live, dst + (r + 1) * row_len, none ? std::numeric_limits<double>::quiet_NaN() : 0.0);
    }
}

} // namespace

extern "C" {

int covest_posterior_classes_chunked(covest_model *m, int64_t n, const double *params, int32_t clamp, int32_t copy_columns,
                                     int64_t chunk_points, double *out_log_p, double *out_error_share,
                                     double *out_copy_share, double *out_mean_copies)
{
    if (!m)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: model is NULL");
    if (n < 0)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: n is negative");
    if (n > 0 && !params)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: params is NULL");
    if (copy_columns < 1 || copy_columns > kPostMaxCopyColumns)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: copy_columns outside 1..65536");
    if (chunk_points < 0)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: chunk_points is negative");
    if (n > 0 && !out_log_p && !out_error_share && !out_copy_share && !out_mean_copies)
        return fail(COVEST_E_INVALID, "covest_posterior_classes: every output is NULL");
    if (n == 0 || m->n_keys == 0)
        return COVEST_OK;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    COVEST_TRY(dev_guard.status());
    COVEST_TRY(ensure_all_bins(m));

    const int P = m->n_par;
    const size_t S = (size_t)m->dm.n_err, K = (size_t)m->n_keys;
    std::vector<int32_t> t;
    int t_max = 2;
    if (P == 5) {
        if (clamp) {
            t = point_thresholds(m, n, params);
        } else {
            t.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i)
                t[(size_t)i] = threshold_o_host(params[i * 5 + 2], params[i * 5 + 3], params[i * 5 + 4], m->threshold,
                                                m->has_threshold, m->hist_max);
        }
        t_max = *std::max_element(t.begin(), t.end());
    }
    DevModel full = m->dm;
    full.bins = m->all_bins;
    if (!clamp)
        for (int i = 0; i < kMaxParams; ++i)
            full.lo[i] = full.hi[i] = std::numeric_limits<double>::quiet_NaN();

    // the columns the device stores: those beyond every point's T - 1 are 0 and are filled in here
    const size_t live = (size_t)std::max(1, std::min((int)copy_columns, t_max - 1));
    const size_t Cc = (size_t)copy_columns;
    const int64_t stride = (int64_t)std::max(1, t_max - 1) * (int64_t)S;
    const bool want_copy = out_copy_share != nullptr, want_err = out_error_share != nullptr, want_mean = out_mean_copies != nullptr;
    const size_t per_point = (size_t)stride * sizeof(PostComp) +
                             K * sizeof(double) * (1 + (want_mean ? 1 : 0) + (want_err ? S : 0) + (want_copy ? live : 0));
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(kPostChunkPoints, (int64_t)(kPostChunkBytes / per_point)));
    if (chunk_points > 0)
        chunk = std::min(chunk, chunk_points);
    chunk = std::min(chunk, n);

    HIP_TRY(m->ws_params.reserve((size_t)chunk * P * sizeof(double)));
    if (P == 5)
        HIP_TRY(m->ws_t.reserve((size_t)chunk * sizeof(int32_t)));
    HIP_TRY(m->ws_post_table.reserve((size_t)chunk * (size_t)stride * sizeof(PostComp)));
    HIP_TRY(m->ws_post_out.reserve((size_t)chunk * (per_point - (size_t)stride * sizeof(PostComp))));
    std::vector<double> h_log_p, h_copy; // a chunk's, where the caller's arrays cannot take the download as it is
    const bool widen = want_copy && live != Cc;
    if (widen) {
        h_log_p.resize((size_t)chunk * K);
        h_copy.resize((size_t)chunk * K * live);
    }

    for (int64_t first = 0; first < n; first += chunk) {
        const size_t cnt = (size_t)std::min(chunk, n - first);
        HIP_TRY(hipMemcpy(m->ws_params.ptr, params + first * P, cnt * P * sizeof(double), hipMemcpyHostToDevice));
        PointSource src{};
        src.params = m->ws_params.as<double>();
        if (P == 5) {
            HIP_TRY(hipMemcpy(m->ws_t.ptr, t.data() + first, cnt * sizeof(int32_t), hipMemcpyHostToDevice));
            src.t_list = m->ws_t.as<int32_t>();
        }
        PostOut o{};
        double *cursor = m->ws_post_out.as<double>();
        o.log_p = cursor, cursor += cnt * K;
        if (want_mean)
            o.mean = cursor, cursor += cnt * K;
        if (want_err)
            o.err = cursor, cursor += cnt * K * S;
        if (want_copy)
            o.copy = cursor, cursor += cnt * K * live;
        HIP_TRY(launch_posterior_table(full, src, (int64_t)cnt, t_max, stride, m->ws_post_table.as<PostComp>(), nullptr));
        HIP_TRY(launch_posterior_walk(full, src.t_list, (int64_t)cnt, stride, m->ws_post_table.as<PostComp>(), copy_columns,
                                      (int)live, o, nullptr));
        const size_t row0 = (size_t)first * K;
        if (out_log_p)
            HIP_TRY(hipMemcpy(out_log_p + row0, o.log_p, cnt * K * sizeof(double), hipMemcpyDeviceToHost));
        if (want_mean)
            HIP_TRY(hipMemcpy(out_mean_copies + row0, o.mean, cnt * K * sizeof(double), hipMemcpyDeviceToHost));
        if (want_err)
            HIP_TRY(hipMemcpy(out_error_share + row0 * S, o.err, cnt * K * S * sizeof(double), hipMemcpyDeviceToHost));
        if (want_copy && !widen)
            HIP_TRY(hipMemcpy(out_copy_share + row0 * Cc, o.copy, cnt * K * Cc * sizeof(double), hipMemcpyDeviceToHost));
        if (widen) {
            HIP_TRY(hipMemcpy(h_log_p.data(), o.log_p, cnt * K * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(h_copy.data(), o.copy, cnt * K * live * sizeof(double), hipMemcpyDeviceToHost));
            widen_rows(out_copy_share + row0 * Cc, h_copy.data(), h_log_p.data(), cnt * K, live, Cc);
        }
    }
    return COVEST_OK;
}

int covest_posterior_classes(covest_model *m, int64_t n, const double *params, int32_t clamp, int32_t copy_columns,
                             double *out_log_p, double *out_error_share, double *out_copy_share, double *out_mean_copies)
{
    return covest_posterior_classes_chunked(m, n, params, clamp, copy_columns, 0, out_log_p, out_error_share, out_copy_share,
                                            out_mean_copies);
}

} // extern "C"
