// factored_launch.h -- what K-factored's two kinds of translation unit share: ll_factored.hip, compiled once per
// variant (-DCOVEST_FACTORED_VARIANT=v: the kernel and its launcher), and ll_factored_launch.hip (the finishing kernels
// and the dispatcher).  THE TABLE OF VARIANTS is here: a variant's template arguments, its number (the row) and its name
// in the launch record are written once; the instantiation of a variant's unit, the dispatcher and
// covest_compiled_variants read them from it, covest_amd/build.py its length (kernels.h kFactoredVariants).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "kernels.h"

namespace covest {

// The chunks' shares of p_j (list modes 2 and 3, tiles.h) travel through HBM TIMES 2^128: p_j <= 2.5, so nothing
// overflows, and a p_j below half a grid step -- which the reference's roundings may still keep alive, handback.h
// kZeroSteps -- does not flush to 0 on the way: finish_point decides on the exact value.
constexpr double kShareScale = 0x1p128;

// LDC: the row stride of G as a COMPILE-TIME constant (0: plan.ld) -- kLdWide = 290, the stride of every plain grid whose
// largest threshold_o - 1 lies in 257 .. 288 (C3: 284): the 32 stores of a tile's walk and the fragments' offsets become
// immediates (round 4).
constexpr int kLdWide = 290;

// PLAIN: the shape every dense grid of the reference's own set-up has -- list_mode 0, at most 8 error classes (one
// lane per copy number) -- compiled on its own so that the other modes' code costs it no registers.
struct FactoredVariant {
    int nt;     // threads of a workgroup
    bool tail;  // the model has a tail (sp_j is summed)
    bool plain;
    int ldc;    // 0, or the row stride the variant is compiled for
    const char *name; // in the launch record and covest_compiled_variants
};
// (one translation unit each: the HIP runtime loads a translation unit's code object when one of its kernels is first
// launched, and a process that evaluates a plain dense grid should not pay for the other variants, 75-98 KB of code each)
constexpr FactoredVariant kFactoredVariantTable[] = {
    {256, false, false, 0, "ll_factored<256>"},
    {256, false, true, 0, "ll_factored<256,plain>"},
    {256, true, false, 0, "ll_factored<256,tail>"},
    {256, true, true, 0, "ll_factored<256,tail,plain>"},
    {512, false, false, 0, "ll_factored<512>"},
    {512, false, true, 0, "ll_factored<512,plain>"},
    {512, true, false, 0, "ll_factored<512,tail>"},
    {512, true, true, 0, "ll_factored<512,tail,plain>"},
    {512, false, true, kLdWide, "ll_factored<512,plain,ld290>"},
    {512, true, true, kLdWide, "ll_factored<512,tail,plain,ld290>"},
};
static_assert(sizeof(kFactoredVariantTable) / sizeof(kFactoredVariantTable[0]) == kFactoredVariants,
              "kernels.h kFactoredVariants counts the table's rows (covest_amd/build.py compiles a unit per row)");
static_assert(kLdWide == 290, "the names of the table spell the row stride of kLdWide");

// The variant that runs a workgroup of nt threads at row stride ld: the one compiled for that stride where there is
// one, else the one that reads it from the plan; -1: none.
constexpr int factored_variant_of(int nt, bool tail, bool plain, int ld)
{
    int found = -1;
    for (int v = 0; v < kFactoredVariants; ++v) {
        const FactoredVariant &f = kFactoredVariantTable[v];
        if (f.nt == nt && f.tail == tail && f.plain == plain && (f.ldc == ld || (f.ldc == 0 && found < 0)))
            found = v;
    }
    return found;
}

// HIP wraps a grid of more than 2^32 threads silently: at most 2^22 workgroups per launch ((c, e) rows per launch)
inline int64_t factored_rows_per_launch(const FactoredPlan &plan) { return std::max<int64_t>(1, ((int64_t)1 << 22) / plan.n_qblocks); }

// Variant V of the table: defined and instantiated in ll_factored.hip's unit number V, called by the dispatcher.
template <int V>
hipError_t launch_ll_factored_variant(const DevModel &m, const TileView &tv, const FactoredPlan &plan, double *out_ll,
                                      const SubList &sub_list, hipStream_t stream);

} // namespace covest
