// handback.h -- the hand-back of the recurrence kernels (K-basic, K-factored): the clamp below which a p_j is not theirs to
// decide, the side word that names the rows a point hands back, and the queue of such points that ll_fix.hip drains.
// Host and device code: the launchers size and reset the queue, the kernels push to it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace covest {

// ---- the hand-back of the recurrence kernels: a RANGE of tile rows per point ----
// Where keys with h_j != 0 have a subnormal p_j -- typically a run of a few dozen keys at one end of the counted
// keys -- the reference's value hangs on the rounding of every single term onto the 4.9e-324 grid (DESIGN.md
// section 2), which only the term-by-term evaluation reproduces.  How far the recurrence kernels' own p_j can be
// off there is bounded.  With g = 4.94e-324: the reference rounds each of the S terms of a copy number twice
// (<= g each, weighted by b_o, and the b_o sum to <= 1) and each copy number's share once (g / 2); the recurrence
// kernels round each G[o][j] once and each accumulation step once.  So |p_j - p_j(reference)| <= (S + T) g, which
// moves the log-likelihood by at most h_j (S + T) g / p_j -- and |LL| >= 708 h_j because of that very key.  So above
//     p_clamp = (S + T_max) * 7e-317     (T_max: the largest threshold_o of the launch)
// the recurrence kernels' value is within 1e-10 of the reference's whatever the roundings were, and nothing needs
// doing.  Below it they take log(max(p_j, p_clamp)) (one v_max per log, everywhere), so what such a key
// contributed is KNOWN -- h_j log(p_clamp) -- and they name, in a 64-bit side word per point, the first and last
// tile row (row = 32 * tile + position, tiles.h) at which they met one: single rows (K-basic) or units of 16 rows
// (K-factored: the half tile of a weight vector).  ll_fix_list_kernel (ll_fix.hip) then evaluates the counted rows
// of that range strictly (K-direct's arithmetic) and, where the strict p_j is below p_clamp, replaces the known
// contribution by h_j safe_log(p_j).
constexpr unsigned long long kSubFieldMask = 0xFFFFFull; // 20 bits: rows < 2^20 (16384 keys, one tile each, at worst)
constexpr double kClampPerTerm = 7e-317; // see above
// WHEN IS p_j ZERO IN THE REFERENCE?  (round 4: found by comparing K-basic with K-direct on ALL 10^6 points of C2 -- one
// point, p_j = 0.9987 x 2^-1075, was -inf here and finite there and in the reference.)  The reference rounds every
// term onto the 4.94e-324 grid on its way: the extension's cast to double (c_src/covest_poissonmodule.c:32, ties to even:
// anything above half a grid step survives), then a_os * TP (covest/models.py:93,238: survives if a_os > 1/2), then, repeats
// model, b_o * (sum over s) (:237-241: survives if b_o > 1/2).  So the reference's p_j can be ONE GRID STEP when the exact
// value is as small as 1/4 of a step (basic model) or 1/8 (repeats model) -- and h_j log(4.94e-324) is finite where
// h_j log(0) is -inf.  A recurrence kernel's own product, rounded once, is 0 below 1/2 step: it must not decide.  Below
// kZeroSteps grid steps (EXACT value, tested before the product underflows) a p_j is zero in the reference whatever the
// roundings were; between that and p_clamp the row is handed back to the term-by-term evaluation.
constexpr double kZeroSteps = 0.12;
constexpr double kGridStep = 4.94065645841246544e-324; // 2^-1074
// kZeroSteps grid steps TIMES 2^sh, for values carried with that factor (K-basic's p_j 2^64, the chunks' shares
// 2^128).  Multiplied in THIS order: kZeroSteps * kGridStep alone rounds to 0 (round 4, first cut: every row below
// the clamp went to the strict kernel, 78 instead of 29 us on C2)
constexpr double zero_steps_scaled(double two_to_sh) { return kZeroSteps * (kGridStep * two_to_sh); }

__host__ __device__ inline unsigned long long sub_word(unsigned first, unsigned last, bool units16)
{
    return (1ull << 62) | ((unsigned long long)(units16 ? 1 : 0) << 60) | ((unsigned long long)last << 20) |
           (unsigned long long)first;
}
// The queue of handed-back points of one launch: (local point index, side word) pairs appended with one atomic
// each by the thread that writes the point's value.  Capacity = the number of points, so it cannot overflow.
// ll_fix_list_kernel (ll_fix.hip) drains it, one wave per entry.
struct SubList {
    double p_clamp;           // (S + T_max) * kClampPerTerm of this launch, and its log (libm, host)
    double log_p_clamp;
    unsigned *count;          // device counter; zero before the launch
    int64_t *index;           // [capacity] index into the launch's LL buffer
    unsigned long long *word; // [capacity]
    int64_t index_offset;     // added by the launcher when it cuts a launch into parts
#ifdef COVEST_DIAG
    // DIAGNOSTIC builds only (tiles.h): K-basic writes, INSTEAD of the log-likelihood, 1: the class of the point's
    // route through its closed form (ll_basic.hip kClass*), 2: the smaller of log p_j at the first and at the last
    // counted key the closed form was asked about (NaN where it was not asked).  tools/dump_c2_classes.py uses it to
    // choose WHERE the reference is asked (tests/golden/make_golden.py section c2classes); env COVEST_DIAG_BASIC_CLASS.
    int diag_class;
#endif
#ifdef __HIPCC__
    __device__ __forceinline__ void push(int64_t idx, unsigned long long w) const
    {
        const unsigned at = atomicAdd(count, 1u);
        index[at] = idx;
        word[at] = w;
    }
#endif
};

__host__ __device__ inline unsigned sub_first(unsigned long long w) { return (unsigned)(w & kSubFieldMask); }
__host__ __device__ inline unsigned sub_last(unsigned long long w) { return (unsigned)((w >> 20) & kSubFieldMask); }
__host__ __device__ inline bool sub_units16(unsigned long long w) { return ((w >> 60) & 1) != 0; }

} // namespace covest
