// batch_host.h -- the argument rules and the host arithmetic of the covest_batch_* entry points (abi_batch.cpp; DESIGN.md
// section 6r; the definition is in include/covest_amd.h): what a batch accepts, how a point list is cut into table
// chunks against the byte budget, how a launch is cut at 2^23 workgroups, and the exactly rounded sum behind the tail
// cell of a draw.  Plain C++ without HIP, so that tests/batch_host_check.cpp runs all of it under the sanitizers on a
// machine without a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace covest {

constexpr int64_t kBatchHostTableBytes = (int64_t)256 << 20; // kernels.h kBatchTableBytes (abi_batch.cpp asserts it)
constexpr int64_t kBatchHostMaxBlocks = (int64_t)1 << 23;    // workgroups of one launch, as everywhere in the library
constexpr int64_t kBatchHostMaxHist = (int64_t)1 << 20;      // histograms of a batch (kernels.h kBatchMaxHist)

// What is wrong with the histograms of covest_batch_create (nullptr: nothing): n_hist rows of n_keys finite counts >= 0,
// and per row a finite tail >= 0 (tails == nullptr: all 0).
inline const char *batch_check_create(int64_t n_keys, int64_t n_hist, const double *counts, const double *tails)
{
    if (n_keys < 1)
        return "the model has no keys";
    if (n_hist < 0)
        return "n_hist must not be negative";
    if (n_hist > kBatchHostMaxHist)
        return "more than 2^20 histograms";
    if (n_hist > 0 && !counts)
        return "null counts";
    for (int64_t i = 0; i < n_hist * n_keys; ++i)
        if (!(counts[i] >= 0.0) || std::isinf(counts[i])) // (NaN fails the comparison)
            return "a count is negative, NaN or infinite";
    if (tails)
        for (int64_t b = 0; b < n_hist; ++b)
            if (!(tails[b] >= 0.0) || std::isinf(tails[b]))
                return "a tail is negative, NaN or infinite";
    return nullptr;
}

// ... with an evaluation's point list: n >= 0 points, and the buffers when there is anything to do
inline const char *batch_check_points(int64_t n, int64_t n_hist, const void *params, const void *out)
{
    if (n < 0)
        return "n must not be negative";
    if (n > 0 && n_hist > 0 && (!params || !out))
        return "null buffer";
    return nullptr;
}

// ... with two result arrays (the arg-min's value and index; the score table's rows and tail coefficients)
inline const char *batch_check_points(int64_t n, int64_t n_hist, const void *params, const void *out_a, const void *out_b)
{
    return batch_check_points(n, n_hist, params, out_a && out_b ? out_a : nullptr);
}

// ... and with the histogram numbers of a pairs call: each in 0 .. n_hist - 1
inline const char *batch_check_index(int64_t n, const int64_t *index, int64_t n_hist)
{
    if (n > 0 && !index)
        return "null index";
    for (int64_t i = 0; i < n; ++i)
        if (index[i] < 0 || index[i] >= n_hist)
            return "a histogram index is outside 0 .. n_hist - 1";
    return nullptr;
}

// A pairs call: its list (the buffers whenever n > 0: a request names its histogram), then its histogram numbers
inline const char *batch_check_pairs(int64_t n, int64_t n_hist, const int64_t *index, const void *params, const void *out)
{
    if (const char *bad = batch_check_points(n, 1, params, out))
        return bad;
    return batch_check_index(n, index, n_hist);
}

// Rows a point of the table of a model with n_par parameters, by the order of the derivatives asked for: 1 for the values
// (order 0), P + 1 with the gradient (the value row, then a score row a parameter), and
// 1 + P + P (P + 1) / 2 with the Hessian (behind those a curvature row a pair k <= l; section 6x): 6 and 21.
inline int batch_rows_per_point(int n_par, int order)
{
    return order <= 0 ? 1 : order == 1 ? n_par + 1 : 1 + n_par + n_par * (n_par + 1) / 2;
}

// ... and the order a table of `rows` rows a point was built for
inline int batch_table_order(int n_par, int rows) { return rows <= 1 ? 0 : rows == n_par + 1 ? 1 : 2; }

// Points of one table chunk: as many as the budget holds at `rows_per_point` rows of n_keys doubles each (1: the value
// table; P + 1: the gradient's; 1 + P + P (P + 1) / 2: the Hessian's), one at least.
inline int64_t batch_points_per_chunk(int64_t n_keys, int64_t rows_per_point, int64_t budget_bytes)
{
    const int64_t point = (n_keys > 0 ? n_keys : 1) * (rows_per_point > 0 ? rows_per_point : 1) * (int64_t)sizeof(double);
    const int64_t per = budget_bytes / point;
    return per > 0 ? per : 1;
}

inline int64_t batch_chunk_count(int64_t n, int64_t per) { return n <= 0 ? 0 : (n + per - 1) / per; }

// chunk c of a list of n: its first point and how many it has
inline void batch_chunk(int64_t n, int64_t per, int64_t c, int64_t *first, int64_t *count)
{
    *first = c * per;
    *count = n - *first < per ? n - *first : per;
}

// A launch of `total` workgroups in parts of at most `cap`: how many parts, and part k's first workgroup and size.
inline int64_t batch_launch_parts(int64_t total, int64_t cap) { return total <= 0 ? 0 : (total + cap - 1) / cap; }
inline void batch_launch_part(int64_t total, int64_t cap, int64_t k, int64_t *first, int64_t *count)
{
    *first = k * cap;
    *count = total - *first < cap ? total - *first : cap;
}

// The cross contraction's launch grid: tiles of 16 histograms, four of them a workgroup (grid y), against groups of 64
// points (grid x); x is cut so that one launch stays within `cap` workgroups.
inline int64_t batch_cross_groups_y(int64_t n_hist) { return ((n_hist + 15) / 16 + 3) / 4; }
inline int64_t batch_cross_groups_x(int64_t n_points) { return (n_points + 63) / 64; }
inline int64_t batch_cross_x_per_launch(int64_t groups_y, int64_t cap)
{
    const int64_t per = cap / (groups_y > 0 ? groups_y : 1);
    return per > 0 ? per : 1;
}

// The sum of finite doubles, rounded once (Shewchuk's partials with the half-way correction: what Python's math.fsum
// returns, and so the tail cell 1 - fsum(p) that bootstrap.model_cells forms).  Finite inputs whose sum stays finite.
inline double batch_fsum(const double *v, int64_t n)
{
    std::vector<double> part;
    for (int64_t k = 0; k < n; ++k) {
        double x = v[k];
        size_t kept = 0;
        for (size_t p = 0; p < part.size(); ++p) {
            double y = part[p];
            if (std::fabs(x) < std::fabs(y)) {
                const double t = x;
                x = y;
                y = t;
            }
            volatile double hi = x + y; // (volatile: the two roundings must be the doubles', whatever the host's flags)
            volatile double yr = hi - x;
            const double lo = y - yr;
            if (lo != 0.0)
                part[kept++] = lo;
            x = hi;
        }
        part.resize(kept);
        part.push_back(x);
    }
    double hi = 0.0;
    int64_t i = (int64_t)part.size();
    if (i > 0) {
        hi = part[(size_t)--i];
        double lo = 0.0;
        while (i > 0) { // from the top down until the sum is inexact
            const double x = hi, y = part[(size_t)--i];
            volatile double s = x + y;
            volatile double yr = s - x;
            hi = s;
            lo = y - yr;
            if (lo != 0.0)
                break;
        }
        // half-way case: round to even needs the sign of what lies below
        if (i > 0 && ((lo < 0.0 && part[(size_t)i - 1] < 0.0) || (lo > 0.0 && part[(size_t)i - 1] > 0.0))) {
            const double y = lo * 2.0;
            volatile double x = hi + y;
            volatile double yr = x - hi;
            if (y == yr)
                hi = x;
        }
    }
    return hi;
}

// The weights of a draw over a model's cells from its probabilities (bootstrap.model_cells): p_j at every key and, with
// a tail, one more cell max(0, 1 - fsum(p)).  out has room for n_keys + has_tail.
inline void batch_draw_weights(int64_t n_keys, const double *p, bool has_tail, double *out)
{
    for (int64_t j = 0; j < n_keys; ++j)
        out[j] = p[j];
    if (has_tail) {
        const double rest = 1.0 - batch_fsum(p, n_keys);
        out[n_keys] = rest > 0.0 ? rest : 0.0;
    }
}

} // namespace covest
