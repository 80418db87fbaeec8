// ll_factored.hip -- K-factored: the fast likelihood kernel of the REPEATS model on
// a dense grid.
//
// In RepeatsModel.compute_probabilities (covest/models.py:211-242)
//
//     p_j = sum_{o=1}^{T-1} b_o(q1,q2,q) * G[o][j],   G[o][j] = sum_s a_os * TP(o*l_s, j)
//
// everything expensive -- G -- depends only on (c, e); the other three parameters
// enter through the weights b_o and the cut-off T (models.py:185-208).  A dense
// grid (covest/grid.py:39-43: itertools.product of the axes) evaluates every
// (c, e) with the same Q = |q1| x |q2| x |q| weight vectors, so one workgroup
// takes one (c, e) and all Q of them, key tile by key tile (32 keys):
//
//   phase A  lane = copy number o: the 8 error-class streams of streams.h walk the
//            32 keys (2 fp64 instr per pmf term) and store G'[key][o] -- their sum, without
//            the key's scale (round 3, see the kernel) -- to LDS.  Waves whose lanes are
//            all beyond Tmax skip it.
//   phase B  P[key][q] = sum_o G[key][o] * b_o(q) on the fp64 matrix pipe:
//            v_mfma_f64_16x16x4_f64, A = 16 keys x 4 o from LDS (conflict-free
//            ds_read_b64: row stride = 4 dwords mod 64), B = 4 o x 16 q generated
//            IN REGISTERS: b_{o+4} = b_o (1-q)^4 is one multiply per MFMA, the first
//            8 weights and the cut-off T come from the host (libm pow, as CPython)
//            -- the contraction reads no weights from memory at all.
//   phase C  h_j * log P[key][q] straight from the accumulator registers: in the
//            f64 C/D layout a lane keeps ONE q column, so the running LL of a unit
//            is a single register per lane (fast_log, fastmath.h).
//
// Round 2 (each step in DESIGN.md 6):
//   * phase A walks a tile with the LIVE error classes only: the classes' rates fall geometrically, so beyond the
//     first few hundred keys two of the eight streams are left and the others hold exact zeros in every lane
//     (streams.h enter_tile / `gone`): variants of the straight-line walk for 8, 4, 2, 1 and no stream;
//   * SHARED STEPS (tiles.h): the host lays the weight vectors out so that a q-tile's 16 columns differ in q1, q2
//     only; below the tile's smallest cut-off the contraction is then beta_col times a sum that does not depend
//     on the column -- summed once per key on the vector unit (Horner in (1-q)^-4) and brought in by ONE MFMA;
//   * the four logs of a unit go through fast_log_n stage by stage (their table reads in flight together);
//   * a p_j deep in the subnormal range is clamped and its row recorded: ll_fix_list_kernel (ll_fix.hip) redoes
//     those rows with K-direct's arithmetic (mix_lot.h).
//
// The unit of phases B/C is (q-tile of 16 weight vectors, half of the key tile);
// the host deals units to waves longest-first, balanced per SIMD (tiles.h), and a
// wave's o-loop stops at its own unit's T.  gfx950 measured (tools/
// microbench_f64.hip): v_fma_f64 62 TFLOP/s, v_mfma_f64_16x16x4 75 TFLOP/s, and
// the two do NOT overlap (one fp64 datapath), so the phases are sequential and the
// kernel is bound by the fp64 pipe:
//   flops per (c,e) = B*8*(Tmax-1)*2  +  B*sum_q(T_q-1)*2  +  B*Q*(one log)
// against B*8*sum_q(T_q-1)*4 for the per-point formulation of SURVEY 8(d).
//
// Reference restated: covest/models.py:100-107 (LL), :211-242 (p_j), over
// covest/grid.py:59-64 (the grid map).
//
// This file is the kernel and its launcher, compiled once per variant (-DCOVEST_FACTORED_VARIANT=v, the row of
// factored_launch.h's table); the finishing kernels and the dispatcher are ll_factored_launch.hip.  The stages that
// stand on their own are in headers (which, and why the others are still written out in the kernel):
//   factored_build.h     phase A: the walk of a tile, the tile's entry and dispatch, an item
//   factored_contract.h  phase B: an MFMA step, the shared steps' sum, the pieces' adding, an item's bands (band.h BandBytes)
//   factored_log.h       phase C: the chunks' shares of p_j on their way to HBM
//   factored_epilogue.h  the result entries' unit-table words
//   factored_diag.h      the stamps of the diagnostic build (empty otherwise)
//   factored_state.h     the layout made afresh, the rows' scale
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "band.h"
#include "factored_build.h"
#include "factored_contract.h"
#include "factored_diag.h"
#include "factored_epilogue.h"
#include "factored_launch.h"
#include "factored_log.h"
#include "fastmath.h"
#include "handback.h"
#include "kernels.h"
#include "point_fetch.h"
#include "streams.h"
#include "wave.h"

namespace covest {

namespace {

// (PLAIN, LDC: factored_launch.h, the table of variants.)
//
// Round 3: the rows of a plain item stay UNSCALED in LDS and in the accumulators -- G' = the sum of the streams'
// scaled terms (streams.h), P'_j = p_j / scal_j -- because the per-key scale is the same for every copy number and
// every weight vector: log p_j = log(P'_j 2^-SC) + ln((k0-1)!/(k0+b)!), and the second term, weighted by h_j, is a
// CONSTANT of the histogram (tiles.h item_lconst, long double on the host) added once per point.  Phase A loses two
// multiplies per key pair and the 64 scalar registers the tile's scales took (the compiler fetched them pair by pair
// right before their use: an exposed scalar-load latency every two keys); the 2^-SC disappears into the exponent
// arithmetic of the log (fastmath.h fast_log_bits_n).  Only where p_j itself is needed -- sp_j with a tail, the
// chunks' shares of p_j in list modes 2 and 3 -- a row is multiplied by its scale, read from LDS.
template <int NT, int HU, bool TAIL, bool PLAIN, int LDC = 0>
__global__ __launch_bounds__(NT) void ll_factored_kernel(const DevModel m, const int32_t n_tiles, const int32_t n_items,
                                                         const double *__restrict__ tile_dbl,
                                                         const int32_t *__restrict__ tile_int,
                                                         const FactoredPlan plan,
                                                         double *__restrict__ out_ll, const SubList sub_list)
{
    const TileView tv = tile_view_from(n_tiles, n_items, tile_dbl, tile_int);
    constexpr int NW = NT / kWave;
    constexpr int MU = 2 * HU; // accumulator slots per wave (6: the specialised step loops below assume it)
    static_assert(MU == 6, "contract loops are written for 6 slots");
    // SPO (round 5): a plain grid WITH A TAIL sums sp_j -- the sum of p_j over EVERY key, covest/models.py:103 -- per COPY
    // NUMBER in phase A instead of per weight vector in phase C:
    //     sp_q = sum_j sum_o b_o(q) G[o][j] = sum_o b_o(q) S[o],   S[o] = sum_j G[o][j]  (scaled: sum_j scal_j G'[j][o]),
    // one fused multiply-add a key in the builder lane that holds G'[j][o] in a register anyway, a compensated add a tile,
    // and ONE extra contraction at the very end whose two rows are S (hi, lo) -- instead of a multiply and a two-sum
    // (seven dependent instructions) per row, unit and tile in phase C, twelve accumulator registers a lane, and a
    // contraction per thirty-two count-less tiles.  The tiles without a count then only cost their walk, and a unit
    // whose sums are all -inf needs nothing more at all (the tail term is finite or 0): the dead-unit skip and the
    // last-tile-first order of the tail-less grids apply.
    constexpr bool SPO = PLAIN && TAIL;
    constexpr bool NEED_SCAL = !PLAIN; // p_j itself is needed row by row: the chunks' shares, a point list's sp_j
    constexpr int LOG_DEG = PLAIN ? 3 : 5;     // (point lists keep the 2e-16 log: refinements difference their values;
                                               // dense grids: 6e-13 absolute and the exponent's bias taken off per sum)
    const int LD = LDC ? LDC : plan.ld; // G row stride in doubles: 4 dwords (mod 64) -> conflict-free A reads
    constexpr int NE = FactoredLds::entries_of(NT); // [waves][slots][16] entries: one per (wave, slot, weight vector)
    const FactoredLds lay{NT, plan.n_buf, LD, SPO}; // every offset into Gs (tiles.h)
    extern __shared__ double Gs[]; // G's buffers; reused for the final per-q combine
    __shared__ __attribute__((aligned(16))) double log_tab[kLogTableDoubles];
    // rows handed back (handback.h), per accumulator slot and weight vector: first unit, last unit + 1 (0: none;
    // a unit = the 16 rows of a half tile: index 2 * tile + half).  One writer per entry: the lane with kq == 0.
    __shared__ unsigned sub_rec[NE * 2];
    // per row of the key tile being logged and of the next one: {h_j, p_clamp in the row's units (0: no count -- such
    // a row is never "low")}, and the row's scale where p_j itself is needed.  Every unit reads the 4 rows of its lanes
    // from here (LDS, addressed by the unit's half) instead of selecting between two register sets per row.
    __shared__ __attribute__((aligned(16))) double2 rowc[2][kTileBins];
    __shared__ __attribute__((aligned(16))) double rows[NEED_SCAL ? 2 : 1][NEED_SCAL ? kTileBins : 2];
    // {(1-q)^16, ln(1-q), (1-q)^4, (1-q)^(-4 nsh)} of every slot with shared steps (tiles.h): wave-uniform, read back as LDS broadcasts
    __shared__ __attribute__((aligned(16))) double rho_tab[PLAIN ? NW * MU * 4 : 4];
    __shared__ double lconst_s; // the constant the rows' scales add to every point's sum (tiles.h item_lconst)
    __shared__ double band_ln[PLAIN ? kBandClasses : 1]; // ln of the error classes' rates, for the units' bands (band.h)
    // THE COLUMN LIMIT (band.h; tiles.h FactoredPlan::col_floor): per item of the walk (the last entry: every item from the
    // 64th on, as the bands) the largest copy number a unit of this workgroup reads with a weight that matters.  Made in
    // the prologue by the waves that build nothing, read by the builders from the walk's first barrier on: a builder
    // wave whose copy numbers all lie above an item's limit skips the item (factored_build.h build_item).
    __shared__ int col_hi[PLAIN ? kWave : 1];
    static_assert(MU == kMaxUnits, "the LDS layout counts kMaxUnits slots a wave");
    // (+ 15 bytes of alignment in front of each array at most)
    static_assert(sizeof(log_tab) + sizeof(sub_rec) + sizeof(rowc) + sizeof(rows) + sizeof(rho_tab) + sizeof(lconst_s) +
                          sizeof(band_ln) + sizeof(col_hi) + 8 * 15 <= kFactoredStaticLds, "the planners' LDS budget (tiles.h) must hold the kernel's static LDS");

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    Stamps stamps(plan, NW, wave); // (diagnostic builds only: factored_diag.h)
    const double p_clamp = plan.p_clamp; // handback.h
    const double zero_frac = kZeroSteps * (kGridStep / p_clamp); // handback.h kZeroSteps, in units of p_clamp
    const int list_mode = PLAIN ? 0 : plan.list_mode;

    // ---- the (c, e) of this workgroup ----
    // list mode: workgroup = (unit, key segment); a unit is a point or a chunk of a point's copy numbers, the
    // key tiles are cut into n_seg contiguous segments so that even ONE point spreads over several CUs
    const int n_seg = list_mode ? plan.n_seg : 1;
    const int unit = list_mode ? (int)blockIdx.x / n_seg : (int)blockIdx.x;
    const int seg = list_mode ? (int)blockIdx.x - unit * n_seg : 0;
    // (the loop below walks ITEMS, tiles.h: a plain tile, or up to 32 all-zero-count tiles summed -- the latter
    // only exist with a tail; without one item i is tile i)
    const int seg_items = (n_items + n_seg - 1) / n_seg;
    const int t_begin = seg * seg_items, t_end = min(n_items, t_begin + seg_items);
    // (a dense grid's (c, e) pairs are taken from the END of the block: a pair costs the more the larger its rates are --
    // 452 k to 467 k ticks along c on C3 -- and the workgroups launched last decide how long the chip's last round runs;
    // round 4, from the per-workgroup stamps: 1.6 % of the launch was that tail, 0.4 % with the long ones first)
    const int64_t ce = (PLAIN || list_mode == 0) ? plan.ce_end - 1 - unit : plan.ce_begin + unit;
    // (list mode: workgroup i takes point i of a point list -- its own (c, e) AND its own single weight
    // vector, see tiles.h FactoredPlan::list_mode)
    const bool list = list_mode == 1 || list_mode == 2; // (3 is a dense grid's chunk: addressed like mode 0)
    const int64_t ic = list ? ce : ce / plan.n_e;
    const int64_t ie = list ? ce : ce - ic * plan.n_e;
    // A workgroup's start (round 5): everything it fetches before its first barrier -- the point, the log table, the
    // shared steps' constants, the items' constants -- is ASKED FOR first and written to LDS afterwards.  In the order
    // of their uses each fetch stood behind the LDS store of the one before (a loop or a branch between them: the
    // compiler moves no load across those), four round trips to the cache one after the other in front of every
    // workgroup's first barrier (the stage stamps of the diagnostic build, profiles/r05_c3_factored_stage_stamps.txt).
    double par[kMaxParams] = {plan.c_axis[ic], plan.e_axis[ie], 0, 0, 0};
    constexpr int kLogPerThread = (kLogTableDoubles + NT - 1) / NT;
    double log_v[kLogPerThread];
#pragma unroll
    for (int u = 0; u < kLogPerThread; ++u)
        log_v[u] = kLogTable[min(tid + u * NT, kLogTableDoubles - 1)];
    const double rho_v = PLAIN ? plan.unit_rho[(int64_t)blockIdx.y * NW * MU * 4 + min(tid, NW * MU * 4 - 1)] : 0.0;
    // (the items' constants: the last wave's, one load per lane and 64 items, added in a fixed order below)
    double lc_first = 0.0;
    if (wave == NW - 1 && t_begin + lane < t_end)
        lc_first = tv.item_lconst[t_begin + lane];
#pragma unroll
    for (int u = 0; u < kLogPerThread; ++u)
        if (tid + u * NT < kLogTableDoubles)
            log_tab[tid + u * NT] = log_v[u];
    if (PLAIN && tid < NW * MU * 4)
        rho_tab[tid] = rho_v;
#pragma unroll
    for (int u = 0; u < (NE + NT - 1) / NT; ++u)
        if (tid + u * NT < NE) {
            sub_rec[2 * (tid + u * NT)] = 0xFFFFFFFFu;
            sub_rec[2 * (tid + u * NT) + 1] = 0;
        }
    clamp_point<2>(m, par);
    const bool finite = isfinite(par[0]) && isfinite(par[1]);
    // the rates of ALL error classes (padded to a multiple of 8; comb = 0 beyond the model's: such a class weighs 0)
    const int n_pass = PLAIN ? 1 : plan.n_pass; // lanes per copy number: one per 8 error classes (1 when max_error <= 8)
    // (by multiplication, as K-basic forms them -- point_fetch.h error_class_rate_mul, round 5: the device library's two
    // pows were 420 dependent instructions that every wave of the workgroup waited for at the barrier below; the strict
    // re-evaluation of the rows handed back, ll_fix.hip, forms the same products)
    if (tid < 8 * n_pass)
        Gs[lay.rates() + tid] = error_class_rate_mul(m, par[0], par[1], tid, m.n_err);
    if (wave == NW - 1) { // the items' constants: one load per lane and 64 items, added in a fixed order
        double lc = 0.0 + lc_first; // (the first 64 items' were asked for above)
        for (int t = t_begin + lane + kWave; t < t_end; t += kWave)
            lc += tv.item_lconst[t];
        lc = wave_sum(lc);
        if (lane == 0) // (PLAIN: the logs come with the exponent's bias on, fastmath.h RAW -- off again for the whole sum:
                       // sum of h_j over the counted keys of this workgroup's items, tiles.h suf_h; a plain grid has one segment)
            lconst_s = PLAIN ? lc - kLogRawBias<kScaleBits> * tv.suf_h[0] : lc;
    }
    __syncthreads();
    stamps.stage(Stamps::kFetched);

    // ---- phase-A state: lane = (pass, copy number): column pass * pass_stride + (o - o_base - 1) of G ----
    // With more than 8 error classes a copy number's classes are dealt to n_pass lanes, 8 each, whose columns the
    // contraction treats as extra copy numbers with the same weight: sum_s a_os TP = sum over the passes' partial sums.
    const int my_pass = n_pass == 1 ? 0 : tid / plan.pass_stride;
    const int o_local = n_pass == 1 ? tid : tid - my_pass * plan.pass_stride; // 0-based inside the chunk
    const bool wave_builds = wave * kWave < plan.n_columns; // wave-uniform
    // chunked point list (list_mode 2): copy numbers before the chunk per item; dense chunks (3): one for the launch
    const int o_base = PLAIN ? 0 : list_mode == 2 ? plan.item_obase[ce] : plan.o_base;
    const int o_mine = o_base + o_local + 1;
    double lam[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
        lam[s] = Gs[lay.rates() + 8 * my_pass + s];
    // (the logarithms of the rates, for the units' bands below: the kernel's own logarithm, once the table is there; read
    // behind the next barrier.  A class without a rate gets a finite number where band.h expects -inf: the class then
    // counts for more than it is worth, never for less)
    if (PLAIN && tid < kBandClasses)
        band_ln[tid] = fast_log(Gs[lay.rates() + tid], log_tab);
    // (the column limit starts from what the planner knows; the bands raise it behind the next barrier)
    if (PLAIN && tid >= NT - kWave)
        col_hi[tid - (NT - kWave)] = plan.col_floor;
    double n_total = -1.0;
    if (n_pass > 1) { // the mixture weights a_os are normalised over ALL classes: covest/models.py:225-233
        n_total = 0.0;
        for (int s = 0; s < 8 * n_pass; ++s)
            n_total += m.comb[s] * (1.0 - exp_neg_rn((double)o_mine * Gs[lay.rates() + s]));
    }
    __syncthreads();
    StreamSet<8> st;
    // (measured and not kept, round 4: the prologue by ALL the waves -- the 8 max_o (copy number, class) pairs dealt to
    // the 512 lanes, n_os / ln x / the normaliser of each made once into the G area, the copy number's lane adding,
    // dividing and taking ln a_os: 30 KB less code, the same bits -- 0.705 against 0.702 ms: no gain, although the three
    // waves that build nothing wait 23 k ticks at the first barrier by the stamps of the diagnostic build)
    if (wave_builds) { // (wave-uniform) the waves that build nothing skip the mixture weights' exps, divisions and logs
        // (the stream constants by the reference's own route for every lane: the lanes of a wave are copy numbers, their
        // rates o x lambda_s span all three regimes of StreamSet::init's shortcut, and a wave that takes all three pays more
        // than the one route costs -- measured, round 5: C3 0.675 against 0.667 ms with the shortcut)
        // (measured and not kept, round 5: the constants stage by stage over the classes, four streams side by side -- exp(-x)
        // with both of its routes evaluated and one selected, the two logs and the division -- and the normaliser stream by
        // stream (without its branches the kernel spills 40 to 56 registers): the first four builder waves' constants
        // 15.3 k -> 13.4 k cycles by the stage stamps, the LAST builder wave's -- copy numbers beyond 256, every route of
        // every class taken, the one the first barrier waits for -- 17.3 k -> 20.2 k: C3 0.647 against 0.640 ms,
        // profiles/r05_c3_ab_staged_stream_constants_not_kept.txt)
        st.template init<false>(m, lam, o_mine, finite && my_pass < n_pass && o_local < plan.max_o, log_tab,
                                log_tab, 8 * my_pass, n_total);
    } else {
        st.gone = 0u;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            st.v[s] = 0.0;
            st.x[s] = 0.0;
            st.an.set(s, 0.0, -INFINITY);
        }
    }
    stamps.stage(Stamps::kStreams);
    const bool lane_in_row = tid < LD - 2; // columns of G that exist (waves past them build nothing)
    if (tid < FactoredLds::kSlack)
        Gs[lay.slack() + tid] = 0.0; // the slack behind the buffers
    // the two pad columns of every row are read by masked steps too: keep them finite
    if (tid < lay.rows()) {
        Gs[lay.pad(tid)] = 0.0;
        Gs[lay.pad(tid) + 1] = 0.0;
    }

    // ---- phase-B/C state: this wave's (q-tile, half) units ----
    const int col = lane & 15; // q column inside a tile / key row of the A fragment
    const int kq = lane >> 4;  // which of the 4 o of an MFMA step
    int len[MU], cont[MU], uhalf[MU], qslot[MU], cut[MU], a_off0[MU], nsh[MU];
    double r4[MU], llacc[MU];
    uint64_t dead[MU]; // lanes that met a p_j <= 0 with h_j != 0
    // (round 4) slots whose unit is DEAD: every one of its 16 weight vectors has met a p_j = 0 at a counted key, so
    // each of their sums is -inf whatever the later keys are worth (utils.safe_log; a tail term is finite or 0) --
    // the unit's remaining shared steps, MFMA steps and logs are skipped.  The units that die are the short ones
    // (small threshold_o against large keys): 13 % of C3's logs.  Wave-uniform, bit k = slot k and its pieces.
    unsigned off_slots = 0;
    bool newly_dead = false; // a column of this wave's met its first zero in the item just logged
    CompSum spacc[(TAIL && !SPO) ? MU : 1]; // (a point list's sp_j: per row, in phase C)
    CompSum so = {0.0, 0.0};                // (SPO, builder lanes) S[o] of this lane's copy number, times 2^SC
    // wave w's block of MU slots in the unit tables
    auto wave_block = [&](int w) -> int {
        if (list) // block 0 is empty (waves with no unit); point i owns blocks 1 + 2 i and 2 + 2 i, for the last two waves
            return w >= NW - 2 ? 1 + 2 * (int)ce + (w - (NW - 2)) : 0;
        return (int)blockIdx.y * NW + w;
    };
    const int slot_base = wave_block(wave) * MU;
    // The slots' entries of the unit tables in THREE rounds of loads, each round's in flight together (round 5): every
    // table holds a harmless entry for a slot without a unit (tile -1, lengths 0, first copy number 1 -- tiles.h), so
    // nothing needs to wait for the slot's tile to know whether it may be read.  Until then every load of a slot stood
    // behind `on ? ... : 0`, the slot's tile came first and the six slots one after the other: a dozen round trips to
    // the cache, 7 000 cycles of a builder wave between its streams' constants and the first key tile (the stage
    // stamps of the diagnostic build, profiles/r05_c3_factored_stage_stamps.txt).
    int u_qt[MU], u_s0[MU], u_len[MU], u_cont[MU], u_half[MU], u_nsh[MU], u_o0[MU], u_T[MU];
#pragma unroll
    for (int k = 0; k < MU; ++k) {
        const int at = slot_base + k;
        u_qt[k] = plan.unit_tile[at];
        u_s0[k] = plan.unit_s0[at];
        u_len[k] = plan.unit_len[at];
        u_cont[k] = plan.unit_cont[at];
        u_half[k] = plan.unit_half[at];
        u_nsh[k] = PLAIN ? plan.unit_nsh[at] : 0;
        u_o0[k] = plan.unit_o0[at];
    }
#pragma unroll
    for (int k = 0; k < MU; ++k) {
        const int qt = __builtin_amdgcn_readfirstlane(u_qt[k]);
        const bool on = qt >= 0;
        const int slot = (on ? qt : 0) * 16 + col;
        qslot[k] = on ? slot : -1;
        u_T[k] = plan.q_T[slot];
        r4[k] = plan.q_r4[slot];
    }
#pragma unroll
    for (int k = 0; k < MU; ++k) {
        const bool on = qslot[k] >= 0;
        const int first_step = __builtin_amdgcn_readfirstlane(u_s0[k]);
        len[k] = __builtin_amdgcn_readfirstlane(u_len[k]);
        cont[k] = __builtin_amdgcn_readfirstlane(u_cont[k]);
        uhalf[k] = __builtin_amdgcn_readfirstlane(u_half[k]);
        // shared steps (tiles.h): steps 1 .. nsh of the unit are summed on the vector unit; the MFMA loops below
        // then run over step 0 and the steps AFTER them, which is what a_off, cut and len are counted in
        nsh[k] = PLAIN ? __builtin_amdgcn_readfirstlane(u_nsh[k]) : 0;
        a_off0[k] = (16 * uhalf[k] + col) * LD + kq + 4 * first_step; // this lane's A fragment of the piece's first step
        // iterations of the piece during which this lane's copy number o0 + 4 i + kq (o0: the piece's first one,
        // counted from the chunk's start) is below T (the chunk's local one)
        const int t_lane = on ? u_T[k] : 0;
        const int o0 = __builtin_amdgcn_readfirstlane(u_o0[k]);
        cut[k] = ((t_lane - (o0 + kq) + 3) >> 2) - nsh[k];
        llacc[k] = 0.0;
        dead[k] = 0;
        spacc[(TAIL && !SPO) ? k : 0].hi = 0.0;
        spacc[(TAIL && !SPO) ? k : 0].lo = 0.0;
    }

    // what kind of slot k is, as bit k of a mask (wave-uniform; tested once per tile and slot): the first slot of a unit
    // (it takes the logs), a piece behind one (its accumulator is added to the slot before), a unit with shared steps
    unsigned m_first = 0, m_cont = 0, m_sh = 0;
#pragma unroll
    for (int k = 0; k < MU; ++k) {
        m_first |= (qslot[k] >= 0 && !cont[k]) ? 1u << k : 0u;
        m_cont |= cont[k] ? 1u << k : 0u;
        m_sh |= nsh[k] > 0 ? 1u << k : 0u;
    }
    // THE BANDS (band.h) of this wave's slots, lane = item of the walk (the last lane: every item from the 64th on, as
    // one range of keys): the MFMA steps from step_hi on add less than 2^-64 of P_j for every key of the item and every
    // column of the unit -- at a large key the low copy numbers' Poissons are all that is left of a row, and the
    // contraction need not run on to the unit's cut-off.  Only units with kBandMinShared shared steps or more have a band
    // (one q a tile: the weights are geometric); a byte a slot in two registers, 255: not banded.  The item's entry is
    // read with one lane read a register and tile; nothing else is held across the walk.
    BandBytes bands; // (band.h)
    // Only a wave that builds nothing makes bands: it waits for the builders' first item anyway (15 k cycles on C3, by the
    // stage stamps of the diagnostic build), while in a builder wave the same few thousand cycles stand in front of
    // every wave's first barrier -- and in the late key tiles, where a band is narrow, the builders are not the waves
    // the barrier waits for.
    bool wave_bands = false; // (wave-uniform) a unit of this wave's is long enough for a band
#pragma unroll
    for (int k = 0; k < MU; ++k)
        wave_bands = wave_bands || (PLAIN && !wave_builds && nsh[k] >= kBandMinShared);
    // ... and THE COLUMN LIMIT with them: the largest copy number below a band's edge, over the wave's own banded units and
    // over the builders' long units the planner hands it (tiles.h band_extra: entry j to the (j mod makers)-th of these
    // waves) -- where the planner's floor leaves a column to skip at all.  A maximum in LDS per lane = item.
    const bool wave_limit = PLAIN && !wave_builds && plan.col_floor < plan.max_o; // (wave-uniform)
    if (PLAIN && (wave_bands || wave_limit)) {
        // (the kernel's own logarithm, 2e-16 absolute, and the hardware's reciprocal with one Newton step: band.h, roundings)
        struct {
            const double *tab;
            __device__ double ln(double x) const { return fast_log(x, tab); }
            __device__ double rcp(double x) const
            {
                const double r = __builtin_amdgcn_rcp(x);
                return fma(fma(-x, r, 1.0), r, r);
            }
        } const mth = {log_tab};
        const int it = min(lane, t_end - 1);
        const double key_first = tv.rec[TAIL ? tv.item_first[it] : it].k0;
        const double key_last = (lane < kWave - 1 ? key_first : tv.rec[n_tiles - 1].k0) + (double)(kTileBins - 1);
        const BandTile bt = band_tile(band_ln, m.ln_comb, key_first, key_last);
        int hi = 0; // the largest copy number this wave's bands leave in the lane's item
#pragma unroll
        for (int k = 0; k < MU; ++k) {
            if (nsh[k] < kBandMinShared) // wave-uniform
                continue;
            const Band b = band_of_unit(mth, lam[0], rho_tab[4 * (wave * MU + k) + 1], 4 + 4 * nsh[k], nsh[k] + len[k], bt);
            bands.set(k, b.step_hi);
            hi = max(hi, band_top_column(b));
        }
        if (wave_limit) {
            const int n_build_waves = (plan.n_columns + kWave - 1) / kWave; // (this wave is none of them)
#pragma unroll 1
            for (int j = wave - n_build_waves; j < kBandExtra; j += NW - n_build_waves) {
                const int e = __builtin_amdgcn_readfirstlane(plan.band_extra[(int)blockIdx.y * kBandExtra + j]);
                if (e < 0)
                    continue;
                // (a builder's unit: its shared steps and length from the tables, its ln(1-q) from rho_tab as above)
                const int at = (int)blockIdx.y * NW * MU + e;
                const int nsh_x = __builtin_amdgcn_readfirstlane(plan.unit_nsh[at]);
                const int len_x = __builtin_amdgcn_readfirstlane(plan.unit_len[at]);
                const Band b = band_of_unit(mth, lam[0], rho_tab[4 * e + 1], 4 + 4 * nsh_x, nsh_x + len_x, bt);
                hi = max(hi, band_top_column(b));
            }
            if (hi > 0)
                atomicMax(&col_hi[lane], hi);
        }
    }
    // b_o of every slot's first (wfirst) and second (wrun, then advanced by (1-q)^4 per step) MFMA step:
    // an L2-resident host table.  The loads for tile t+1 are issued between tile t's MFMAs and its
    // logs, so their latency (2-3 us per tile when exposed) hides behind the logs and the barrier.
    double wfirst[MU], wrun[MU];
    auto load_weights = [&]() {
#pragma unroll
        for (int k = 0; k < MU; ++k) {
            // ONE 16-byte load per slot: {b_o of the first step, b_o the running weight starts from}
            const double2 pw = reinterpret_cast<const double2 *>(plan.piece_w)[(int64_t)(slot_base + k) * kWave + lane];
            wfirst[k] = pw.x;
            wrun[k] = pw.y;
        }
    };
    load_weights();
    // A NaN among (q1, q2, q) makes every b_o from the third on a NaN (covest/models.py:193-208; its threshold_o is
    // max(hist)), and the reference's likelihood with it.  The logs below work on the bits and would turn it into
    // a finite number: the columns concerned are found from the weights themselves -- AFTER the walk (round 4: found
    // here and kept, the six masks held twelve scalar registers through the whole kernel, which spills them).

    // ================= phase A (factored_build.h): G'[key][o] of an item into a buffer =================
    bool resync = false; // (PLAIN, wave-uniform) tiles were skipped: the next one walked anchors every stream afresh
    unsigned zeroed = 0; // (PLAIN, wave-uniform) bit b: this wave's columns of buffer b hold the zeros of a skipped item
    // (A local lambda forwards to the stage, here and below, and the stages take the kernel's variables one by one, where
    // they are declared: called directly, or with the state gathered into a struct, the compiler numbers the streams'
    // registers otherwise and fuses other products of a key's sum -- DESIGN.md 6z.)
    auto build = [&](int it, bool seg_start, bool skip, int buf_bit, double *dst) __attribute__((always_inline)) {
        build_item<TAIL, SPO, PLAIN>(tv, plan, st, so, resync, zeroed, tid, LD, lane_in_row, stamps, it, seg_start, skip, buf_bit, dst);
    };
    stamps.walk_begins();
    stamps.stage(Stamps::kUnits);

    // With two buffers the builders fill item t+1 while every wave contracts item t: one barrier per item, and the
    // host's unit assignment charges the builders for phase A.  ONE loop for both set-ups (and ONE copy of phase A in
    // the code: three used to be inlined): interval p builds the item of position p + 1 and contracts that of position p.
    // (Measured and not kept, round 3: no barrier between the items but two counters per buffer in LDS -- builder waves
    // that have filled it, waves that are done with it -- so that a wave may run an item ahead: 0.846-0.849 against
    // 0.831-0.832 ms; the polling costs more than the hardware barrier's lock step, whose waits are 10 % of the kernel.)
    const bool dbuf = plan.n_buf == 2;
    // the rows' constants of the item an interval builds are fetched one interval ahead (32 lanes of wave 0; the two
    // or three loads are independent and have a whole interval to arrive)
    double nxt_h = 0.0, nxt_c = 0.0, nxt_s = 0.0;
    auto fetch_rows = [&](int it) {
        if (tid < kTileBins && it < t_end) {
            const int64_t at = (int64_t)it * kTileBins + tid;
            nxt_h = tv.item_cnt[at];
            nxt_c = tv.item_iscal[at]; // (0 for a row without a count)
            if (NEED_SCAL)
                nxt_s = tv.item_scal[at];
        }
    };
    // THE LAST KEY TILE FIRST (a plain grid without a tail; round 4).  A weight vector whose sum is -inf -- 44 % of C3's
    // points -- has met a p_j = 0 at a counted key, and the key where that happens is, with hardly an exception, the
    // LARGEST one: p_j is a mixture of Poissons whose means stop at (threshold_o - 1) c, so it only underflows beyond
    // them.  Taken in ascending order a doomed unit is walked, contracted and logged until its columns die near the end;
    // with the last tile taken first it dies in the first interval and the dead-unit skip (above) leaves out all the
    // rest.  The order of a point's sums changes by that one term; its value is -inf or finite either way, and the rows
    // handed back are recorded as a range (min, max).  Position p of the walk is tile tile_at(p); the buffers, rowc and
    // rows alternate with the POSITION.  The streams are anchored afresh at the first position (the last tile: nothing
    // is on yet) and at the second (tile 0 is a run start anyway; what they know of the last tile -- `gone` -- is
    // forgotten there).
    // Round 5, WITH A TAIL (SPO): the same, with the last item that HOLDS A COUNT taken first (the items behind it are
    // sums over count-less tiles: nothing dies there) -- sp_j no longer hangs on the contraction (S[o] above), and the
    // streams are anchored afresh once more, at the item behind the one taken out of turn.
    int last_item = t_end - 1; // the item taken first
    if (SPO)
        while (last_item > t_begin && tv.item_sum[last_item] != 0)
            --last_item;
    const bool last_first = PLAIN && t_end - t_begin >= 2 && last_item > t_begin;
    auto tile_at = [&](int p) -> int { return last_first ? (p == t_begin ? last_item : (p <= last_item ? p - 1 : p)) : p; };
    // SPO: one more position behind the items -- the contraction of S (rows 0 and 1 of the buffer: hi, lo)
    const int t_endx = t_end + (SPO ? 1 : 0);
    fetch_rows(tile_at(t_begin));
    for (int p = t_begin - (dbuf ? 1 : 0); p < t_endx; ++p) {
        const int pb = dbuf ? p + 1 : p;
        if (SPO && pb == t_end) {
            if (wave_builds && lane_in_row) { // S[o] (x 2^-kBasicShift: exact) as the two rows of one more "item"
                double *dst = Gs + lay.buf(pb) + tid;
                dst[0] = so.hi * 0x1p-540;
                dst[LD] = so.lo * 0x1p-540;
            }
        } else if (pb < t_end) {
            if (tid < kTileBins) { // read after the barrier that makes the item readable
                rowc[pb & 1][tid] = make_double2(nxt_h, p_clamp * nxt_c);
                if (NEED_SCAL)
                    rows[pb & 1][tid] = nxt_s;
            }
            fetch_rows(pb + 1 < t_end ? tile_at(pb + 1) : t_end);
            if (wave_builds) {
                if (last_first && pb == t_begin + 1)
                    st.gone = 0u;
                const int it = tile_at(pb);
                // the item's column limit: below all of this wave's copy numbers (wave-uniform) -- not at the walk's
                // first position: the table is there from the first barrier on, and the last tile is built in full
                bool skip = false;
                if (PLAIN && pb > t_begin)
                    skip = wave * kWave + 1 > __builtin_amdgcn_readfirstlane(col_hi[min(it, kWave - 1)]);
                build(it, pb == t_begin || (last_first && (pb == t_begin + 1 || pb == last_item + 1)), skip, dbuf ? pb & 1 : 0,
                      Gs + lay.buf(pb));
            }
        }
        stamps.lap(Stamps::kBuild);
        if (!dbuf)
            __syncthreads();
        const bool sp_item = SPO && p == t_end; // (wave-uniform) the last position: S x b
        if (p >= t_begin && !(SPO && !sp_item && tv.item_sum[tile_at(p)] != 0)) { // (SPO: a sum item was phase A only)
            const int t = tile_at(p); // the tile this interval contracts and logs
            const double *cur = Gs + lay.buf(p);
            // ================= phase B (its steps: factored_contract.h): P' = G' x b on the matrix pipe =================
            d4 acc[MU];
            const d4 zero4 = (d4){0.0, 0.0, 0.0, 0.0};
            // Every slot's accumulator starts from its first MFMA (C = 0 costs nothing; zeroing 8 registers per slot
            // does); the step-0 fragments of all slots are read first, in flight together.
            // A unit with shared steps (tiles.h) sums them on the vector unit (factored_contract.h shared_steps_sum) and
            // ONE MFMA brings the sum in: the four lanes of a key add up inside it, every column gets its own b_o of
            // that first shared step, made from the weight the slot holds (b_o of the first step after them) times r^-nsh.
            double a0[MU];
#pragma unroll
            for (int k = 0; k < MU; ++k)
                a0[k] = cur[a_off0[k]]; // (an idle slot reads a valid address and uses nothing)
            // this item's bands (above): the slots' step_hi, a byte each.  (S x b, the last position of a grid with a
            // tail, is a sum over every key: the full range)
            BandBytes item_bands;
            if (PLAIN && !sp_item)
                item_bands = bands_of_item(bands, t);
            stamps.first_fragments(a0, wfirst);
#pragma unroll
            for (int k = 0; k < MU; ++k) {
                // (a dead unit, off_slots: its len[k] is 0 by now and its bit of m_sh cleared -- it takes the branch below
                // and starts from zero)
                if (!PLAIN || !((m_sh >> k) & 1u) || COVEST_SKIP_PHASE(plan, 8)) { // wave-uniform
                    acc[k] = len[k] > 0 ? __builtin_amdgcn_mfma_f64_16x16x4f64(a0[k], wfirst[k], zero4, 0, 0, 0) : zero4;
                    continue;
                }
                const double rr16 = rho_tab[4 * (wave * MU + k)]; // (LDS broadcasts)
                const double2 rt = *reinterpret_cast<const double2 *>(&rho_tab[4 * (wave * MU + k) + 2]);
                const double rr4 = rt.x, rho_n = rt.y;
                const double *g1 = cur + a_off0[k]; // step 0 of the unit (o = 1 .. 4); step i at g1[4 i]
                // (the empty asm: what derives from the slot's step count -- the trip count, the three "is there a head"
                // masks -- is made afresh per tile, five scalar instructions, instead of being held across the walk: the
                // compiler hoisted all of it out of the tile loop, 40 scalar registers that it then spilled to vector
                // lanes and fetched back with v_readlane, a VECTOR instruction, every tile)
                int nsh_k = nsh[k];
                asm volatile("" : "+s"(nsh_k));
                if (PLAIN) // the shared steps above the band are left out: the weights are relative to the FIRST shared step
                    nsh_k = min(nsh_k, item_bands.get(k) - 1);
                // (the slack: a head that does not exist is read from there; the layout made afresh from the plan, factored_state.h)
                const double hs = shared_steps_sum(g1, nsh_k, Gs + fresh_lds<NT, SPO>(plan, LD).slack(), rr16, rr4);
                acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(hs, wrun[k] * rho_n, zero4, 0, 0, 0);
                acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[k], wfirst[k], acc[k], 0, 0, 0);
            }
            stamps.lap(Stamps::kShared);
            // the remaining steps, specialised on the number of slots still running (len is sorted)
            if (!COVEST_SKIP_PHASE(plan, 2)) {
                int a_off[MU]; // this lane's A fragments counted from the first step after the shared ones (per tile: 6 adds
                               // instead of 6 registers held through the other phases)
                // lenb: of the steps after the shared ones a slot runs those below its band's edge -- none where the band ends
                // at or below its last shared step.  (The loops stay correct with such entries among the sorted lengths, as
                // with a dead unit's 0: slot k gets max(lenb[k..5]) steps, the suffix maximum, which is at most len[k]; a
                // step beyond the band is only unnecessary.)
                int lenb[MU];
#pragma unroll
                for (int k = 0; k < MU; ++k)
                {
                    int nsh_k = nsh[k];
                    asm volatile("" : "+s"(nsh_k));
                    a_off[k] = a_off0[k] + 4 * nsh_k;
                    lenb[k] = PLAIN ? min(len[k], max(item_bands.get(k) - nsh_k, 1)) : len[k];
                }
                // (measured and not kept, round 4: one address register a slot with the buffer's base folded in and two
                // steps a trip, the second fragment an immediate offset away -- the compiler moves the induction to the
                // scalar unit, six s_add a trip: 0.867-0.871 against 0.855-0.858 ms)
                int i = 1;
                for (; i < lenb[5]; ++i)
                    contract_step<6, MU>(i, cur, a_off, cut, r4, wrun, acc);
                for (; i < lenb[4]; ++i)
                    contract_step<5, MU>(i, cur, a_off, cut, r4, wrun, acc);
                for (; i < lenb[3]; ++i)
                    contract_step<4, MU>(i, cur, a_off, cut, r4, wrun, acc);
                for (; i < lenb[2]; ++i)
                    contract_step<3, MU>(i, cur, a_off, cut, r4, wrun, acc);
                for (; i < lenb[1]; ++i)
                    contract_step<2, MU>(i, cur, a_off, cut, r4, wrun, acc);
                for (; i < lenb[0]; ++i)
                    contract_step<1, MU>(i, cur, a_off, cut, r4, wrun, acc);
            }
            add_pieces<MU>(m_cont, acc);
            stamps.lap(Stamps::kContract);
            // ================= phase C: h_j * log p_j from the accumulators =================
            const bool item_is_sum = TAIL && !SPO && tv.item_sum[t] != 0; // wave-uniform
            // f64 C/D layout: register r of a lane is row (lane>>4) + 4r, column lane&15.
#pragma unroll
            for (int k = 0; k < MU; ++k) {
                if (list_mode == 2) { // a chunk of a point's copy numbers: hand p_j's share on (column 0 only)
                    if (qslot[k] >= 0 && !cont[k] && col == 0)
                        store_shares<NEED_SCAL>(plan.partial + (ce * tv.n_items + t) * kTileBins + 16 * uhalf[k] + kq, false, acc[k],
                                                row_scale<NEED_SCAL>(rows, p, 16 * uhalf[k] + kq));
                    continue;
                }
                if (list_mode == 3) { // a chunk of the copy numbers of a dense grid's LONG weight vectors: every
                                           // column's share of p_j goes to (the first chunk) or is added to the block's
                                           // buffer in HBM; ll_finish_dense takes the logs.
                    if (qslot[k] >= 0 && !cont[k])
                        store_shares<NEED_SCAL>(plan.partial + (((ce - plan.ce_first) * plan.n_cols_partial + qslot[k]) * tv.n_items + t) * kTileBins +
                                                    16 * uhalf[k] + kq,
                                                plan.o_base != 0, acc[k], row_scale<NEED_SCAL>(rows, p, 16 * uhalf[k] + kq));
                    continue;
                }
                if (SPO && sp_item) {
                    // rows 0 and 1 are S (hi, lo): register 0 of the lanes with kq = 0 and kq = 1 holds this column's
                    // sum_o b_o S_hi[o] and sum_o b_o S_lo[o].  Straight to where the last step below looks for them
                    // (the SPO parts, tiles.h FactoredLds: out of the last interval's way) -- held in registers until then
                    // they would be carried through every interval of the walk.  A dead unit writes its zeros: its sum is
                    // -inf whatever sp_j is.
                    if (qslot[k] >= 0 && !cont[k] && uhalf[k] == 0 && lane < 32)
                        Gs[lay.spo_parts(t_end) + kq * NE + (wave * MU + k) * 16 + col] = acc[k][0];
                    continue;
                }
                if (TAIL && !SPO && item_is_sum) { // rows are sums over count-less tiles (scaled ones): they only enter sp_j
                    if ((m_first >> k) & 1u) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            spacc[k].add(acc[k][r]);
                    }
                    continue;
                }
                // (a dead unit's bit of m_first is cleared: nothing it could add changes its -inf)
                if (((m_first >> k) & 1u) && !COVEST_SKIP_PHASE(plan, 4)) { // wave-uniform: first slot of a unit
                    // Everything out of the ordinary -- p_j <= 0, or deep in the subnormal range (below p_clamp,
                    // handback.h), at a key with h_j != 0 -- is caught by ONE compare per row against the clamp in
                    // the row's own units (0 for a row without a count: filler keys, a tile's padding, zero counts
                    // with a tail -- never "low"), made BEFORE the logs, and sorted out in a branch the wave takes
                    // for one unit in twenty.  Rows without a count add 0 * log below.
                    const double2 *rc = &rowc[p & 1][16 * uhalf[k] + kq]; // {h, clamp} of this lane's rows kq, kq + 4, ...
                    double h4[4], c4[4], x4[4], lg4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double2 hc = rc[4 * r];
                        h4[r] = hc.x;
                        c4[r] = hc.y;
                    }
                    if (TAIL && !SPO) { // sp_j needs p_j itself (filler and padding keys: scale 0), before the clamp
                        const double *sr = row_scale<NEED_SCAL>(rows, p, 16 * uhalf[k] + kq);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            spacc[k].add(acc[k][r] * sr[NEED_SCAL ? 4 * r : 0]);
                    }
                    uint64_t low[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        low[r] = __ballot(acc[k][r] < c4[r]);
                    if (__builtin_expect(((low[0] | low[1] | low[2] | low[3]) & ~dead[k]) != 0, 0)) {
                        // wave-uniform, cold (a lane that is dead already has nothing more to report).  Kept SHORT: a
                        // wave in here holds up its whole workgroup at the tile's barrier
                        uint64_t subm = 0, zero = 0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            // p_j = 0 in the reference: every term of its sum is at most the sum, and a term below
                            // 2^-1075 is flushed by the extension's cast to double (c_src/covest_poissonmodule.c:32) --
                            // so a row whose p_j (row value x scale) is safely below 1/8 of a grid step (the roundings
                            // on the reference's way can keep anything above that alive: handback.h kZeroSteps) is a
                            // zero, not a candidate for the strict evaluation.  (The unscaled row value itself never
                            // underflows: half of the C3 grid is -inf this way, and would otherwise queue up for the
                            // strict kernel.)
                            const uint64_t z = __ballot(acc[k][r] <= c4[r] * zero_frac) & low[r];
                            zero |= z;
                            subm |= low[r] & ~z;
                            // log(max(p_j, p_clamp)): what a p_j deep in the subnormal range contributes is then a
                            // known constant, which the strict evaluation of that key replaces (handback.h).  In
                            // place: the accumulator is of no further use, and a copy would cost every unit a move.
                            acc[k][r] = max_raw(acc[k][r], c4[r]);
                        }
                        // utils.safe_log: p_j <= 0 with h_j != 0 makes the sum -inf; kept as a lane mask in SGPRs -- for
                        // all four row groups of the weight vector (column) at once: its sum is -inf whichever of them
                        // met the zero, and the other three need not come through here for it
                        const uint64_t zc = (zero | (zero >> 16) | (zero >> 32) | (zero >> 48)) & 0xFFFFull;
                        dead[k] |= zc * 0x0001000100010001ull;
                        newly_dead = newly_dead || zc != 0; // (wave-uniform: look for dead units after this item's logs)
                        // p_j DEEP IN THE SUBNORMAL RANGE: the unit (this half tile) is recorded for every weight vector
                        // (column) concerned -- first and last unit met; one writer per entry, the lane of row group 0.
                        // The strict evaluation of its counted rows follows in ll_fix_list_kernel (ll_fix.hip)
                        const uint64_t cm = (subm | (subm >> 16) | (subm >> 32) | (subm >> 48)) & 0xFFFFull;
                        if (kq == 0 && ((cm >> col) & 1)) {
                            const unsigned u = 2u * (unsigned)(TAIL ? tv.item_first[t] : t) + (unsigned)uhalf[k];
                            unsigned *rec = &sub_rec[((wave * MU + k) * 16 + col) * 2];
                            rec[0] = min(rec[0], u);
                            rec[1] = max(rec[1], u + 1);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        x4[r] = acc[k][r];
                    // no branch on h (it differs between the lanes' rows): the four logs of a unit go through
                    // fast_log_bits_n stage by stage, their table reads in flight together.  (A dead lane's row may be
                    // 0 here: the log of those bits is a finite number nobody uses.)
                    fast_log_bits_n<4, LOG_DEG, kScaleBits, PLAIN>(x4, lg4, log_tab);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        llacc[k] = fma(h4[r], lg4[r], llacc[k]);
                    __builtin_amdgcn_sched_barrier(0); // ... one unit at a time: registers
                }
            }
            // the weights of the next key tile, behind the logs (round 4: issued before them -- where their latency hides
            // best -- the 24 registers they land in were live through the logs and the kernel spilled 18-74; here it
            // spills none and measures the same, 0.856 against 0.856-0.862 ms: the builders' phase A and the barrier hide
            // the loads just as well)
            load_weights();
            if (PLAIN && newly_dead) { // retire the units that died in this item: the first slot and the pieces behind it
                newly_dead = false;
#pragma unroll
                for (int k = 0; k < MU; ++k) {
                    const bool first_dead = ((m_first >> k) & 1u) && dead[k] == ~0ull;
                    const bool piece_dead = k > 0 && ((m_cont >> k) & 1u) && ((off_slots >> (k - 1)) & 1u);
                    if (first_dead || piece_dead) { // wave-uniform
                        off_slots |= 1u << k;
                        m_first &= ~(1u << k); // no logs, no shared steps any more ...
                        m_sh &= ~(1u << k);
                        len[k] = 0; // ... and no MFMA steps (the step loops stay correct with a zero among the sorted
                                    // lengths: every live slot k still gets max(len[k..5]) = len[k] steps)
                    }
                }
            }
            stamps.lap(Stamps::kLog);
        }
        __syncthreads(); // the tile just contracted may be overwritten, the one just built may be read
        stamps.barrier_passed(p, t_begin, t_end, lane);
    }
    stamps.dump_laps(lane);
    if (list_mode >= 2)
        return; // (wave-uniform for the whole workgroup) the chunks are combined by ll_finish_partials / _dense
    // ---- per-q results: sum the 4 row groups of the accumulator layout, then the two
    //      halves of each q-tile (they may live on different waves) through LDS ----
    const double lconst = lconst_s; // (read before the buffer below is reused: lconst_s is static LDS of its own)
    // The unit-table words of the entries this thread finishes below -- the four words of an entry, then its weight
    // vector's place in the grid: two round trips to the cache -- asked for together (round 5: entry after entry, word
    // after word behind `||`, they stood between the last barrier and every workgroup's stores).  With a tail they are
    // asked for HERE, and pass during the sums and the barrier below; without one, behind the barrier in the loop as
    // before: the walk's register allocation hangs on the shape of this epilogue, and the tail-less kernel measured
    // 0.6384 and 0.6500 against 0.6354 ms with two forms of the early fetch (the trimmed C3 with its tail: 0.3817 and
    // 0.3851 against 0.3861) -- profiles/r05_c3_ab_result_entries_early.txt.
    constexpr int kEntries = (NE + NT - 1) / NT;
    constexpr bool kEntriesEarly = TAIL;
    int en_qt[kEntries], en_half[kEntries], en_cont[kEntries], en_pair[kEntries], en_qo[kEntries];
    auto fetch_entries = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kEntries; ++u) {
            const int e = min(tid + u * NT, NE - 1);
            const int at = wave_block(e / (MU * 16)) * MU + (e / 16) % MU;
            const ResultEntry en = fetch_entry(plan, at);
            en_qt[u] = en.qt;
            en_half[u] = en.half;
            en_cont[u] = en.cont;
            en_pair[u] = en.pair;
        }
#pragma unroll
        for (int u = 0; u < kEntries; ++u)
            en_qo[u] = plan.q_orig[max(en_qt[u], 0) * 16 + (tid & 15)]; // (NT is a multiple of 16: the entry's column is tid & 15)
    };
    if (kEntriesEarly)
        fetch_entries();
    // compensated sp_j parts (SPO: where the last contraction left them).  (The layout made afresh here, its row stride
    // pinned by the empty asm: the choice of the SPO parts' place, hoisted into the walk, cost it 25 spilled registers.)
    int ld_end = LD;
    if (SPO && LDC == 0)
        asm volatile("" : "+s"(ld_end));
    const FactoredLds lay_end = fresh_lds<NT, SPO>(plan, ld_end);
    double *part_ll = Gs + lay_end.part_ll();
    double *part_hi = Gs + lay_end.part_hi(t_end);
    double *part_lo = Gs + lay_end.part_lo(t_end);
    // (the slots' first weights are in the registers: they do not depend on the key tile, and every interval that used
    // them up fetched them again behind its logs -- until round 5 they were loaded once more here, a round trip to the
    // cache in front of every workgroup's results.  A NaN column is a NaN in them)
#pragma unroll
    for (int k = 0; k < MU; ++k) {
        double ll = llacc[k];
        const uint64_t nm = __ballot(wfirst[k] != wfirst[k] || wrun[k] != wrun[k]);
        const uint64_t nan_cols_k = ((nm | (nm >> 16) | (nm >> 32) | (nm >> 48)) & 0xFFFFull) * 0x0001000100010001ull;
        if ((nan_cols_k >> lane) & 1)
            ll = NAN; // a NaN weight vector: math.log(nan), covest/models.py:105
        if ((dead[k] >> lane) & 1)
            ll = isnan(ll) ? ll : -INFINITY; // h * -inf summed with finite terms
        ll += __shfl_xor(ll, 16, kWave);
        ll += __shfl_xor(ll, 32, kWave);
        CompSum sp = spacc[(TAIL && !SPO) ? k : 0];
        if (TAIL && !SPO) {
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const double ohi = __shfl_xor(sp.hi, off, kWave);
                const double olo = __shfl_xor(sp.lo, off, kWave);
                double e;
                two_sum(sp.hi, ohi, sp.hi, e);
                sp.lo += olo + e;
            }
        }
        if (lane < 16) {
            const int at = (wave * MU + k) * 16 + lane;
            part_ll[at] = ll;
            if (TAIL && !SPO) {
                part_hi[at] = sp.hi;
                part_lo[at] = sp.lo;
            }
        }
    }
    __syncthreads();
    // one thread per (wave, unit, q) entry of a half-0 unit; it looks up the half-1 partner
    auto finish_entry = [&](int e, int qt, int e_half, int e_cont, int pslot, int qo_early) __attribute__((always_inline)) {
        const int c = e & 15;
        if (qt < 0 || e_half != 0 || e_cont)
            return;
        // the unit with the same tile and half 1 (always in the same workgroup): named by the host (tiles.h unit_pair;
        // until round 4 every thread searched the 48 slots for it, three dependent loads a slot)
        const int pe = pslot >= 0 ? pslot * 16 + c : -1;
        // + the constant of the rows' scales (see the kernel's header): sum_j h_j ln((k0-1)!/(k0+b)!) over this
        // workgroup's items
        const double ll = (part_ll[e] + (pe >= 0 ? part_ll[pe] : 0.0)) + lconst;
        // the units handed back for this weight vector: this half-0 slot's record and its half-1 partner's
        unsigned u_first = sub_rec[2 * e], u_end = sub_rec[2 * e + 1];
        if (pe >= 0) {
            u_first = min(u_first, sub_rec[2 * pe]);
            u_end = max(u_end, sub_rec[2 * pe + 1]);
        }
        const unsigned long long word = u_end ? sub_word(u_first, u_end - 1, true) : 0ull;
        double tail_term = 0.0;
        double hi = 0.0, lo = 0.0;
        if (TAIL) {
            hi = part_hi[e];
            lo = part_lo[e];
            if (pe >= 0 && !SPO) { // (SPO: the half-0 unit alone contracted S)
                double err;
                two_sum(hi, part_hi[pe], hi, err);
                lo += part_lo[pe] + err;
            }
        }
        const int32_t qo = kEntriesEarly ? qo_early : plan.q_orig[qt * 16 + c];
        if (list_mode == 1) { // a key segment of a point: {LL part, sp_j part (hi, lo)}; the host adds the segments
            if (qo >= 0) {
                double *o = plan.partial + ((int64_t)ce * n_seg + seg) * 4;
                o[0] = finite ? ll : NAN;
                o[1] = hi;
                o[2] = lo;
                o[3] = __longlong_as_double((long long)(finite ? word : 0ull)); // (bits; the host merges the segments' words)
            }
            return;
        }
        if (TAIL) {
            double s = hi + lo;
            if (!(s < 1.0))
                s = 1.0; // min(1, fsum(...)), NaN -> 1
            if (s < 1.0)
                tail_term = m.tail * log(1.0 - s);
        }
        if (qo >= 0) {
            const int64_t flat = ce * plan.n_q + qo;
            if (flat >= plan.flat_begin && flat < plan.flat_end) {
                const double v = finite ? ll + tail_term : NAN;
                out_ll[flat - plan.flat_begin] = v;
                if (word != 0 && isfinite(v)) // (rare; -inf stays -inf whatever the keys are worth)
                    sub_list.push(flat - plan.flat_begin, word);
            }
        }
    };
    if (kEntriesEarly) {
#pragma unroll
        for (int u = 0; u < kEntries; ++u)
            if (tid + u * NT < NE)
                finish_entry(tid + u * NT, en_qt[u], en_half[u], en_cont[u], en_pair[u], en_qo[u]);
    } else {
        for (int e = tid; e < NE; e += NT) {
            const int at = wave_block(e / (MU * 16)) * MU + (e / 16) % MU;
            const ResultEntry en = fetch_entry(plan, at);
            finish_entry(e, en.qt, en.half, en.cont, en.pair, 0);
        }
    }
    stamps.dump_stages(lane);
}

} // namespace

// Variant COVEST_FACTORED_VARIANT of factored_launch.h's table: its launcher, and with it the kernel, instantiated below.
template <int V>
hipError_t launch_ll_factored_variant(const DevModel &m, const TileView &tv, const FactoredPlan &plan,
                                      double *out_ll, const SubList &sub_list, hipStream_t stream)
{
    constexpr int NT = kFactoredVariantTable[V].nt, LDC = kFactoredVariantTable[V].ldc;
    constexpr bool TAIL = kFactoredVariantTable[V].tail, PLAIN = kFactoredVariantTable[V].plain;
    constexpr int HU = kHalfUnits;
    const FactoredLds lay{NT, plan.n_buf, plan.ld, PLAIN && TAIL}; // (tiles.h)
    if (!lay.fits())
        return hipErrorInvalidValue;
    const size_t lds = (size_t)lay.total() * sizeof(double);
    // the dynamic-LDS ceiling is a per-device attribute of the kernel: raise it once per device
    static size_t configured[64] = {0};
    static std::mutex configured_lock; // two model handles may be used from two host threads
    std::lock_guard<std::mutex> guard(configured_lock);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        dev = 0;
    if (lds > configured[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ll_factored_kernel<NT, HU, TAIL, PLAIN, LDC>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
        configured[dev] = lds;
    }
    const int64_t per_launch = factored_rows_per_launch(plan);
    for (int64_t first = plan.ce_begin; first < plan.ce_end; first += per_launch) {
        FactoredPlan part = plan;
        part.ce_begin = first;
        part.ce_end = std::min(plan.ce_end, first + per_launch);
        const dim3 grid((unsigned)((part.ce_end - part.ce_begin) * (plan.list_mode ? plan.n_seg : 1)),
                        (unsigned)plan.n_qblocks);
        hipLaunchKernelGGL((ll_factored_kernel<NT, HU, TAIL, PLAIN, LDC>), grid, dim3(NT), lds, stream, m, tv.n_tiles, tv.n_items,
                           tv.dbl_base, tv.int_base, part, out_ll, sub_list);
    }
    return hipGetLastError();
}

template hipError_t launch_ll_factored_variant<COVEST_FACTORED_VARIANT>(const DevModel &, const TileView &, const FactoredPlan &,
                                                                        double *, const SubList &, hipStream_t);

} // namespace covest
