// draw_host.h -- the host arithmetic and the argument rules of covest_draw_thresholds and covest_draw_histograms*
// (abi_draw.cpp; the definition is in include/covest_amd.h).  Plain C++ without HIP, so that
// tests/draw_host_check.cpp runs all of it under the sanitizers on a machine without a device.
#pragma once
#include <cmath>
#include <cstdint>

namespace covest {

constexpr int64_t kDrawHostMaxCells = 65536; // COVEST_DRAW_MAX_CELLS; kernels.h kDrawMaxCells (abi_draw.cpp asserts it)

// What is wrong with a weight vector (nullptr: nothing): m >= 1 finite weights >= 0 whose running sum stays finite
// and ends above 0.
inline const char *draw_check_weights(int64_t m, const double *w)
{
    if (m < 1)
        return "m must be at least 1";
    if (!w)
        return "null weights";
    double cdf = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        if (!(w[i] >= 0.0) || std::isinf(w[i])) // (NaN fails the comparison)
            return "a weight is negative, NaN or infinite";
        cdf = i ? cdf + w[i] : w[i];
    }
    if (!(cdf > 0.0) || std::isinf(cdf))
        return "the weights' total is 0 or not finite";
    return nullptr;
}

// ... and with the rest of a call: n >= 0 draws of replicates first_rep .. first_rep + n_rep - 1, every index < 2^32
inline const char *draw_check_call(int64_t m, int64_t n_draws, int64_t first_rep, int64_t n_rep)
{
    if (m < 1)
        return "m must be at least 1";
    if (m > kDrawHostMaxCells)
        return "m is beyond the 65536 cells a call supports";
    if (n_draws < 0)
        return "n_draws must not be negative";
    if (n_rep < 0)
        return "n_rep must not be negative";
    if (first_rep < 0 || first_rep > ((int64_t)1 << 32) || n_rep > ((int64_t)1 << 32) - first_rep)
        return "a replicate index is 2^32 or more";
    return nullptr;
}

// t_i = floor(r_i * 2^63), r_i = cdf_i / total, cdf summed strictly left to right: basic IEEE operations only (the
// product is an exact scaling, and r_i <= 1 so that t_i <= 2^63 fits).  After draw_check_weights.
inline void draw_thresholds(int64_t m, const double *w, uint64_t *out)
{
    double total = w[0];
    for (int64_t i = 1; i < m; ++i)
        total = total + w[i];
    double cdf = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        cdf = i ? cdf + w[i] : w[i];
        const double r = cdf / total;
        out[i] = (uint64_t)(r * 9223372036854775808.0); // (non-negative: the conversion is the floor)
    }
}

} // namespace covest
