// posterior.h -- K-post: per key, the posterior shares of the mixture's error classes and copy numbers, in the log
// domain (posterior.hip; covest_posterior_classes, abi_posterior.cpp).
//
// With x_os = o * l_s, a_os and b_o the doubles prepare_mix_lot forms (mix_lot.h: the reference's, covest/models.py:77,
// 87-90, 194-206, 221-233) and D the reference's normaliser (log_trunc_norm, point_fetch.h):
//   ln w_os(j) = ln b_o + ln a_os + j ln x_os - D(x_os) - ln j!     (-inf where a_os b_o = 0 or x_os = 0)
//   ln p_j     = logsumexp over (o, s);  E_s(j) = sum_o w_os / p_j;  C_o(j) = sum_s w_os / p_j;  M(j) = sum_o o C_o(j)
// Two launches a chunk of points, neither entered in the launch records or in covest_compiled_variants.
#pragma once
#include <hip/hip_runtime_api.h>

#include "device_model.h"

namespace covest {

// One component of a point's table: its term at key j is exp(j * lx + w - ln j!).
struct PostComp {
    double w;  // ln b_o + ln a_os - D(x_os); -inf where the component weighs nothing
    double lx; // ln x_os (0 where x_os = 0)
};

constexpr int kPostMaxCopyColumns = 65536; // the cap on copy_columns (include/covest_amd.h)

// Stage 1: table[i * stride + (o - 1) * S + s] for the n points of `src` (a list; threshold_o per point for the repeats
// model, 2 for the basic one), o = 1 .. T_i - 1, s = 0 .. S - 1, S = m.n_err.  One wave per (point, lot of 64 / S copy
// numbers): prepare_mix_lot<P>(LibmMath{}, ...) and two logs a component.  t_max: the largest threshold_o of the list;
// stride >= (t_max - 1) * S.  n <= 65535.
hipError_t launch_posterior_table(const DevModel &m, const PointSource &src, int64_t n, int t_max, int64_t stride,
                                  PostComp *table, hipStream_t stream);

// What stage 2 leaves, point-major; a pointer that is nullptr is not written (log_p always is).
struct PostOut {
    double *log_p;  // [n][n_keys]
    double *err;    // [n][n_keys][S]
    double *copy;   // [n][n_keys][live], live = the row length given to the launch
    double *mean;   // [n][n_keys]
};

// Stage 2: one lane a key of m.bins (the all-keys view), one wave 64 keys of one point.  Three walks over the point's
// table: the maximum; class-major (E_s, and ln p_j from its total); copy-major (the copy columns and M; only where
// out.copy or out.mean is asked for).  Column c < copy_columns - 1 is o = c + 1, column copy_columns - 1 everything from
// o = copy_columns on; live = min(copy_columns, t_max - 1) (at least 1) columns are stored, zero beyond T_i - 1.
// A key at which every component is -inf: ln p_j = -inf, NaN shares and mean.  n <= 65535.
hipError_t launch_posterior_walk(const DevModel &m, const int32_t *t_list, int64_t n, int64_t stride, const PostComp *table,
                                 int copy_columns, int live, const PostOut &out, hipStream_t stream);

} // namespace covest
