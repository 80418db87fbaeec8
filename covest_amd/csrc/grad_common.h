// grad_common.h -- what the derivative kernels (K-grad and K-hess, ll_deriv.hip) need beside the walk: the derivatives of the
// log of the truncated Poisson's normaliser inside each of its pieces.  (The compensated (hi, lo) sums a segment leaves:
// wave.h comp_merge, wave_comp_reduce.)
#pragma once
#include <hip/hip_runtime.h>

#include "point_fetch.h"
#include "wave.h"

namespace covest {

// d/dx of log_trunc_norm (point_fetch.h), inside each of its pieces: 1 / x on the two branches that divide by x itself,
// 1 / (1 - exp(-xr)) of the residual otherwise.  The rint onto the 2^-63 grid is rounding noise and has no derivative.
__device__ __forceinline__ double trunc_norm_dlog(double x)
{
    if (x <= 1e-8)
        return 1.0 / x;
    double xr = x;
    if (x > 200.0) {
        const double n = ceil(x / 200.0) - 1.0;
        xr = fma(-200.0, n, x);
        if (xr > 200.0)
            xr -= 200.0;
        else if (xr <= 0.0)
            xr += 200.0;
        if (xr <= 1e-8)
            return 1.0 / x;
    }
    return -1.0 / expm1(-xr);
}

// The first AND the second derivative, piece by piece as above: L' = 1 / x, L'' = -1 / x^2 on the two branches that
// divide by x itself; L' = 1 / (1 - exp(-xr)), L'' = -exp(-xr) / (1 - exp(-xr))^2 of the residual otherwise.  d1 is
// trunc_norm_dlog(x), the same expressions (bit for bit: tests/test_gpu_math.py, which holds both to the 50-digit
// derivatives inside every piece -- relative errors in profiles/math_primitives.txt, all below 1e-15).
__device__ __forceinline__ void trunc_norm_dlog2(double x, double &d1, double &d2)
{
    double xr = x;
    bool by_x = x <= 1e-8;
    if (!by_x && x > 200.0) {
        const double n = ceil(x / 200.0) - 1.0;
        xr = fma(-200.0, n, x);
        if (xr > 200.0)
            xr -= 200.0;
        else if (xr <= 0.0)
            xr += 200.0;
        by_x = xr <= 1e-8;
    }
    if (by_x) {
        d1 = 1.0 / x;
        d2 = -d1 * d1;
    } else {
        const double em = expm1(-xr); // -(1 - exp(-xr))
        d1 = -1.0 / em;
        // exp(-xr): em + 1 carries an ABSOLUTE 1.1e-16, which is all of exp(-xr) from xr = 37 on (L'' came out as 0 at
        // xr = 199.9, and 2e-12 off at xr = 10: tests/test_gpu_math.py) -- from 1 on the exponential itself
        const double ex = xr >= 1.0 ? exp_fast(-xr) : em + 1.0;
        d2 = -ex * d1 * d1;
    }
}

} // namespace covest
