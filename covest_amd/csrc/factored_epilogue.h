// factored_epilogue.h -- K-factored behind the walk (ll_factored.hip): the unit-table words of the result entries.
#pragma once
#include "tiles.h"

namespace covest {

// The four unit-table words of a result entry (one per (wave, slot, weight vector); `at`: its slot in the unit tables),
// fetched TOGETHER -- behind `||`, word after word, each waited for the one before (round 5).  The kernel asks for them
// either before the per-slot sums, where they pass during the sums and the barrier (kEntriesEarly: with a tail), or
// behind the barrier, entry by entry.
struct ResultEntry {
    int qt, half, cont, pair; // the q-tile (-1: none), the half, a piece behind a first slot, the half-1 partner's slot
};
__device__ __forceinline__ ResultEntry fetch_entry(const FactoredPlan &plan, int at)
{
    return ResultEntry{plan.unit_tile[at], plan.unit_half[at], plan.unit_cont[at], plan.unit_pair[at]};
}

} // namespace covest
