// factored_state.h -- what the stages of K-factored's kernel share (ll_factored.hip; the stages: factored_build.h,
// factored_contract.h, factored_log.h, factored_epilogue.h).  The kernel's state stays in the kernel, as plain locals
// declared where they always were, and a stage takes what it reads and writes by reference -- gathered into structs,
// or handed to a stage without a local lambda in between, the same code is compiled with other registers for the
// streams and other fused products.
#pragma once
#include <hip/hip_runtime.h>

#include "tiles.h"

namespace covest {

typedef double d4 __attribute__((ext_vector_type(4)));

// K-factored's LDS layout (tiles.h) MADE AFRESH from the plan, in the slot's shared steps and behind the walk: `lay`,
// held from the top of the kernel, cost the walk spilled scalars (its n_buf; the choice of the SPO parts' place,
// hoisted into the walk, 25 registers).
template <int NT, bool SPO>
__device__ __forceinline__ FactoredLds fresh_lds(const FactoredPlan &plan, int ld)
{
    return FactoredLds{NT, plan.n_buf, ld, SPO};
}

// The scale of row `row` of the item at position p: the kernel keeps the rows' scales, rows[2][kTileBins], only where
// p_j itself is needed row by row (NEED_SCAL: not PLAIN); else the array is a stub and every index is 0.
template <bool NEED_SCAL, class Rows>
__device__ __forceinline__ const double *row_scale(const Rows &rows, int p, int row)
{
    return &rows[NEED_SCAL ? (p & 1) : 0][NEED_SCAL ? row : 0];
}

} // namespace covest
