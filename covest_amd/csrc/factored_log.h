// factored_log.h -- K-factored, PHASE C (ll_factored.hip): what becomes of a slot's accumulator once an item is
// contracted -- the pieces of phase C that stand on their own.  (The unit's logs themselves, h_j log p_j through
// fast_log_bits_n, stay in the kernel's slot loop: they are the registers' critical stretch.)
#pragma once
#include "factored_launch.h" // kShareScale
#include "fastmath.h"
#include "handback.h"
#include "factored_state.h"

namespace covest {

// A chunk's shares of p_j (list modes 2 and 3, tiles.h) on their way to HBM: this lane's four rows of a slot's
// accumulator, each times its row's scale (scal: the lane's first row's, row_scale) and kShareScale, to dst[0], dst[4],
// dst[8], dst[12] -- stored (the first chunk of a dense grid's long weight vectors; every chunk of a point list, which
// has a row of its own in `partial`) or added to what the chunks before left there.  Each element has one owner.
template <bool NEED_SCAL>
__device__ __forceinline__ void store_shares(double *dst, bool add, const d4 &acc, const double *scal)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double share = acc[r] * (scal[NEED_SCAL ? 4 * r : 0] * kShareScale); // (x 2^128: kShareScale)
        dst[4 * r] = add ? dst[4 * r] + share : share;
    }
}

} // namespace covest
