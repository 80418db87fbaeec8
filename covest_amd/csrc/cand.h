// cand.h -- the candidate of the selection scan of covest/grid.py:65-70 and its comparison, shared by the kernels
// that restate it (argmin.hip over a whole block, axis_min.hip per cell of the kept axes, ll_batch.hip per histogram of a batch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave.h"

namespace covest {

struct Cand {
    double v;
    int64_t i; // INT64_MAX: none yet (v = +inf)
};

__host__ __device__ __forceinline__ Cand better(Cand a, Cand b)
{
    // b replaces a iff b is strictly smaller, or equal with a lower index
    const bool take = (b.v < a.v) || (b.v == a.v && b.i < a.i);
    return take ? b : a;
}

__device__ __forceinline__ Cand wave_best(Cand c)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Cand o;
        o.v = __shfl_xor(c.v, off, kWave);
        o.i = __shfl_xor(c.i, off, kWave);
        c = better(c, o);
    }
    return c;
}

} // namespace covest
