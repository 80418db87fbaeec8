// abi_draw.cpp -- covest_draw_thresholds, covest_draw_histograms* of the C ABI over draw_hist.hip: replicate histograms
// drawn from a weight vector, the generator of the parametric bootstrap.  The arithmetic and the
// argument rules are draw_host.h's (plain C++, checked without a device); no handle: the device form launches on the
// caller's stream and returns, the host form owns its device buffers for the call.
#include "host.h"

#include "draw_host.h"

using namespace covest;

static_assert(kDrawHostMaxCells == kDrawMaxCells && COVEST_DRAW_MAX_CELLS == kDrawMaxCells, "one cap on m");

namespace {

int refuse(const char *who, const char *what) { return fail(COVEST_E_INVALID, std::string(who) + ": " + what); }

} // namespace

namespace covest {

// The host side of a draw whose rows STAY on the device (covest_draw_histograms copies them back; covest_batch_draw,
// abi_batch.cpp, turns them into a batch): thresholds of the checked weights, up through the staging block, and the
// launch on the null stream of the current device.  d_out holds n_rep * m int64 afterwards; d_thr must live until the
// kernels are done.
int draw_histograms_resident(const char *who, int64_t m, const double *weights, int64_t n_draws, int64_t first_rep,
                             int64_t n_rep, uint64_t seed, DevBuf &d_thr, DevBuf &d_out)
{
    std::vector<uint64_t> thr((size_t)m);
    draw_thresholds(m, weights, thr.data());
    HIP_TRY(d_thr.reserve(thr.size() * sizeof(uint64_t)));
    HIP_TRY(d_out.reserve((size_t)n_rep * (size_t)m * sizeof(int64_t)));
    COVEST_TRY(stage_upload(d_thr.ptr, thr.data(), thr.size() * sizeof(uint64_t),
                            (std::string(who) + ": upload of the thresholds").c_str()));
    HIP_TRY(launch_draw_hist(d_thr.as<uint64_t>(), m, n_draws, (uint64_t)first_rep, n_rep, seed, d_out.as<int64_t>(), nullptr));
    return COVEST_OK;
}

} // namespace covest

extern "C" {

int covest_draw_thresholds(int64_t m, const double *weights, uint64_t *out)
{
    if (const char *bad = draw_check_weights(m, weights))
        return refuse("covest_draw_thresholds", bad);
    if (!out)
        return refuse("covest_draw_thresholds", "null output");
    draw_thresholds(m, weights, out);
    return COVEST_OK;
}

int covest_draw_histograms_device(int32_t device, int64_t m, const uint64_t *d_thresholds, int64_t n_draws,
                                  int64_t first_rep, int64_t n_rep, uint64_t seed, int64_t *d_out, void *stream)
{
    if (const char *bad = draw_check_call(m, n_draws, first_rep, n_rep))
        return refuse("covest_draw_histograms_device", bad);
    if (n_rep == 0)
        return COVEST_OK;
    if (!d_thresholds || !d_out)
        return refuse("covest_draw_histograms_device", "null buffer");
    DeviceCall call(device, "covest_draw_histograms_device");
    COVEST_TRY(call.status());
    HIP_TRY(launch_draw_hist(d_thresholds, m, n_draws, (uint64_t)first_rep, n_rep, seed, d_out,
                             static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_draw_histograms(int32_t device, int64_t m, const double *weights, int64_t n_draws, int64_t first_rep,
                           int64_t n_rep, uint64_t seed, int64_t *out_counts)
{
    if (const char *bad = draw_check_call(m, n_draws, first_rep, n_rep))
        return refuse("covest_draw_histograms", bad);
    if (const char *bad = draw_check_weights(m, weights))
        return refuse("covest_draw_histograms", bad);
    if (n_rep == 0)
        return COVEST_OK;
    if (!out_counts)
        return refuse("covest_draw_histograms", "null output");
    const size_t cells = (size_t)n_rep * (size_t)m;
    if (n_draws == 0) { // nothing to draw: the rows are zero, and no device is asked for
        std::fill(out_counts, out_counts + cells, (int64_t)0);
        return COVEST_OK;
    }
    DeviceCall call(device, "covest_draw_histograms");
    COVEST_TRY(call.status());
    DevBuf d_thr, d_out; // (go with the call; the copy back has waited for the kernels by then)
    COVEST_TRY(draw_histograms_resident("covest_draw_histograms", m, weights, n_draws, first_rep, n_rep, seed, d_thr, d_out));
    HIP_TRY(hipMemcpy(out_counts, d_out.ptr, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
