// plan_factored.cpp -- K-factored's work descriptions (tiles.h FactoredPlan): the parts of a dense repeats-model grid
// (units dealt to waves longest-first, pieces, shared steps) and the point lists of list mode.
//
// The file reads top to bottom as the stages of a plan, one function each; only the last of them touches HIP:
//   PlanPack, upload_to_grid / _model   the one buffer a kernel reads a plan from: its arrays in the builder's order
//   fill_plan                           the FactoredPlan fields every builder sets the same way
//   part_columns                        per slot and per q-tile of a part: thresholds, (1-q)^4, step counts
//   part_geometry                       columns of G, LDS stride, workgroup size, workgroups per (c, e)
//   planner_charges                     the cost model's constants (unit_deal.h; in tuning builds, their overrides)
//   deal_qblock                         units to waves, pieces, slots -> UnitTables
//   slot_weights, pair_halves           per-lane starting weights; the half-1 partner of every half-0 unit
//   column_limit                        what the kernel's column limit cannot learn from the bands (band.h)
//   build_plan_part                     the driver over the stages above, for one part
//   plain_order / shared_order ...      build_factored_plan's own stages: the order of the weight vectors, the parts
//   build_list_plan                     the point lists of list mode, on the same UnitTables and PlanPack
#include "band.h"
#include "host.h"
#include "unit_deal.h"

#include <initializer_list>

using namespace covest;

namespace covest {

// RepeatsModel.get_b_o, covest/models.py:193-208, with libm pow as CPython's float ** int.
double copy_number_weight_host(double q1, double q2, double q, int o)
{
    if (o == 1)
        return q1;
    if (o == 2)
        return (1 - q1) * q2;
    return (1 - q1) * (1 - q2) * q * std::pow(1 - q, (double)(o - 3));
}

namespace {

constexpr int kQTileSlots = 16; // weight vectors (columns of the contraction's B) of a q-tile
constexpr int kStepColumns = 4; // columns of G -- copy numbers -- one MFMA step takes
constexpr int kStepLanes = kStepColumns * kQTileSlots; // a slot's weights of one step: lane = 16 * (o mod 4) + column
static_assert(kStepLanes == 64, "one wave holds the weights of a step");
static_assert(2 * kHalfUnits == kMaxUnits, "a wave's slots are two halves' (tiles.h)");
constexpr int mfma_steps_of(int columns) { return (columns + kStepColumns - 1) / kStepColumns; }

// ---- the eight unit tables (tiles.h FactoredPlan::unit_*), [blocks][waves][kMaxUnits] ----
struct UnitTables {
    std::vector<int32_t> tile, half, s0, o0, len, cont, nsh, pair;
    explicit UnitTables(size_t n) : tile(n, -1), half(n, 0), s0(n, 0), o0(n, 1), len(n, 0), cont(n, 0), nsh(n, 0), pair(n, -1) {}
    size_t size() const { return tile.size(); }
    // one slot: a piece of `len_` steps from step `s0_` (copy number `o0_`) of the half `half_` of q-tile `tile_`
    void set(size_t at, int tile_, int half_, int s0_, int o0_, int len_, bool cont_, int nsh_)
    {
        tile[at] = tile_;
        half[at] = half_;
        s0[at] = s0_;
        o0[at] = o0_;
        len[at] = len_; // equal lengths: steps past the unit's end are cut off by T
        cont[at] = cont_ ? 1 : 0;
        nsh[at] = nsh_;
    }
};

// ---- the one buffer of a plan: doubles first, then int32, each array where the builder's list puts it ----
// A builder names its arrays ONCE, in the order their bytes take; sizes, staging offsets and the device pointers all
// follow from that list.  An array a builder does not list has no device pointer (nullptr).
class PlanPack {
  public:
    enum Array { Axes, QR4, PieceW, UnitRho, QT, QOrig, UnitTile, UnitHalf, UnitS0, UnitO0, UnitLen, UnitCont, UnitNsh, UnitPair, BandExtra, kArrays };
    PlanPack(std::initializer_list<std::pair<Array, const std::vector<double> *>> dbl,
             std::initializer_list<std::pair<Array, const std::vector<int32_t> *>> ints)
    {
        for (const auto &d : dbl)
            add(d.first, d.second->data(), d.second->size() * sizeof(double));
        for (const auto &i : ints)
            add(i.first, i.second->data(), i.second->size() * sizeof(int32_t));
    }
    size_t bytes() const { return bytes_; }
    void stage(char *dst) const
    {
        for (int k = 0; k < n_; ++k) {
            const Part &p = part_[order_[k]];
            if (p.bytes)
                std::memcpy(dst + p.off, p.src, p.bytes);
        }
    }
    void bind(const void *device_base) { base_ = static_cast<const char *>(device_base); }
    const double *f64(Array a) const { return static_cast<const double *>(at(a)); }
    const int32_t *i32(Array a) const { return static_cast<const int32_t *>(at(a)); }

  private:
    struct Part {
        const void *src = nullptr;
        size_t off = 0, bytes = 0;
        bool listed = false;
    };
    void add(Array a, const void *src, size_t bytes)
    {
        part_[a] = Part{src, bytes_, bytes, true};
        order_[n_++] = a;
        bytes_ += bytes;
    }
    const void *at(Array a) const { return part_[a].listed ? base_ + part_[a].off : nullptr; }
    Part part_[kArrays];
    Array order_[kArrays];
    int n_ = 0;
    size_t bytes_ = 0;
    const char *base_ = nullptr;
};

// A grid's plan: staged on the host in the device layout, ONE copy (a dozen small copies cost ~150 us of the plan
// build); blocking through the process's staging buffer, or asynchronous through the handle's own (covest_grid_reset)
int upload_to_grid(covest_grid *g, DevBuf &buf, PlanPack &pack)
{
    HIP_TRY(buf.reserve(pack.bytes()));
    StageSlot slot;
    const int src = grid_stage_begin(g, pack.bytes(), slot);
    if (src != COVEST_OK)
        return src;
    pack.stage(slot.ptr);
    const int crc = grid_stage_commit(g, slot, buf.ptr, pack.bytes());
    if (crc != COVEST_OK)
        return crc;
    pack.bind(buf.ptr);
    return COVEST_OK;
}

// A point list's plan: one staging buffer (page-locked, the model's), one copy -- or none (in_place: build_list_plan)
int upload_to_model(covest_model *m, DevBuf &buf, bool in_place, PlanPack &pack)
{
    HIP_TRY(m->ws_stage.reserve(pack.bytes()));
    char *stage = m->ws_stage.as<char>();
    if (!in_place)
        HIP_TRY(buf.reserve(pack.bytes()));
    pack.stage(stage);
    // (asynchronous, from the model's page-locked staging memory: the launch queues up behind the copy on the null stream,
    // and the caller waits for the stream before it builds another list -- covest_eval_points)
    if (!in_place)
        HIP_TRY(hipMemcpyAsync(buf.ptr, stage, pack.bytes(), hipMemcpyHostToDevice, nullptr));
    pack.bind(in_place ? static_cast<const void *>(stage) : buf.ptr);
    return COVEST_OK;
}

// What the kernel needs to know of G and of the workgroups that build and contract it.
struct PartGeometry {
    int max_o;       // copy numbers to build: the largest LOCAL threshold - 1
    int pass_stride; // a pass begins on an MFMA step
    int n_columns, ld, n_buf;
    int n_threads, units_per_wave, n_qblocks;
    bool one_block_a_pair = false; // a grid with enough (c, e) pairs to fill the chip with one workgroup each (part_geometry)
    int n_waves() const { return n_threads / 64; }
    size_t block_slots() const { return (size_t)n_waves() * kMaxUnits; } // unit slots of one workgroup
    size_t n_unit() const { return (size_t)n_qblocks * block_slots(); }
};

// The fields of a FactoredPlan that every builder sets the same way: the geometry and the device pointers of the
// arrays the builder packed.  Everything else starts out zero; the builder sets what is its own afterwards.
// (q_first8, qtile_nsteps and qtile_nfull are never set and read by no kernel; half_units is always kHalfUnits.)
void fill_plan(FactoredPlan &pl, const PartGeometry &geo, int n_pass, const PlanPack &pack)
{
    pl = FactoredPlan{};
    pl.max_o = geo.max_o;
    pl.n_pass = n_pass;
    pl.pass_stride = geo.pass_stride;
    pl.n_columns = geo.n_columns;
    pl.n_threads = geo.n_threads;
    pl.half_units = kHalfUnits; // (768 threads with 2 slots per half, 3 waves/SIMD, was measured: +1 %)
    pl.n_qblocks = geo.n_qblocks;
    pl.ld = geo.ld;
    pl.n_buf = geo.n_buf;
    pl.unit_tile = pack.i32(PlanPack::UnitTile);
    pl.unit_half = pack.i32(PlanPack::UnitHalf);
    pl.unit_s0 = pack.i32(PlanPack::UnitS0);
    pl.unit_o0 = pack.i32(PlanPack::UnitO0);
    pl.unit_len = pack.i32(PlanPack::UnitLen);
    pl.unit_cont = pack.i32(PlanPack::UnitCont);
    pl.unit_nsh = pack.i32(PlanPack::UnitNsh); // (list modes are not the PLAIN kernel: not packed, never read)
    pl.unit_pair = pack.i32(PlanPack::UnitPair);
    pl.band_extra = pack.i32(PlanPack::BandExtra); // (a dense grid's parts only)
    pl.col_floor = geo.max_o;                      // (nothing above it is built: no wave skips)
    pl.unit_rho = pack.f64(PlanPack::UnitRho);
    pl.piece_w = pack.f64(PlanPack::PieceW);
    pl.q_r4 = pack.f64(PlanPack::QR4);
    pl.q_T = pack.i32(PlanPack::QT);
    pl.q_orig = pack.i32(PlanPack::QOrig);
    pl.n_seg = 1;
}

// ---- K-factored plans of a dense repeats grid (tiles.h FactoredPlan) ----
// The Q = |q1| x |q2| x |q| weight vectors are sorted by threshold_o (descending) into slots, 16 per q-tile.  A PART
// is one launch's work description: a range of q-tiles and a CHUNK of copy numbers o_base + 1 .. o_base + chunk.
//   * weight vectors whose threshold_o - 1 fits the lanes of a workgroup (`chunk` copy numbers) form ONE part that
//     writes log-likelihoods (list_mode 0);
//   * the longer ones (optimize_grid walks q down to 0.01: threshold_o ~ 1500) are the first q-tiles of the sorted
//     order; they get one part per chunk (list_mode 3) that sums p_j into HBM, and ll_finish_dense takes the logs.
//     Only those tiles pay for it: the rest of the grid stays on the one-launch path.
// With more than 8 error classes (max_error = k + 1 = 22 when a model is built directly, covest/models.py:28-31) a
// copy number's classes are dealt to n_pass = ceil(S / 8) lanes, which the contraction treats as extra columns with
// the same weight; a chunk then holds 512 / n_pass copy numbers.
struct QOrder {
    int64_t n1, n2, n3, nq;
    // slot -> index in the (q1, q2, q) product, -1 = padding; [n_qtiles * 16].  Either all weight vectors by
    // descending threshold_o, or (shared steps, tiles.h) tile by tile: the 16 slots of a tile share q, descending
    // threshold_o inside, the tiles by descending largest threshold_o.
    std::vector<int32_t> order;
    std::vector<int32_t> tile_nsh; // [n_qtiles] shared steps of the tile's units (0: none)
    int32_t n_qtiles;
    int t_max;
};

// One part: q-tiles [tile_lo, tile_hi) of the sorted order, copy numbers o_base + 1 .. o_base + chunk.
struct PartSpec {
    int32_t tile_lo, tile_hi;
    int o_base, chunk, n_pass, list_mode;
    int32_t n_qtiles() const { return tile_hi - tile_lo; }
};

struct SlotQ {
    double q1, q2, q; // clamped to the model's bounds
};

// Per slot [n_qtiles * 16] and per q-tile [n_qtiles] of a part.
struct PartColumns {
    std::vector<int32_t> q_t, q_orig; // LOCAL threshold (0: padding); index in the (q1, q2, q) product (-1: padding)
    std::vector<double> r4;           // (1 - q)^4
    std::vector<SlotQ> w;             // (live slots only)
    std::vector<int32_t> nsteps, nsh; // MFMA steps of the tile's longest column; the tile's shared steps (tiles.h)
    int t_loc_max = 1; // largest LOCAL threshold: copy numbers of the chunk are o_base + 1 .. o_base + t_local - 1
    // MFMA steps of a tile's units: all of them, or step 0 and those after the shared ones
    int mfma_steps(int qt) const { return (int)nsteps[(size_t)qt] - (int)nsh[(size_t)qt]; }
};

PartColumns part_columns(const covest_model *m, const double *const *axes, const std::vector<int32_t> &t_table,
                         const QOrder &qo, const PartSpec &ps)
{
    const size_t n_qtiles = (size_t)ps.n_qtiles(), n_slots = n_qtiles * kQTileSlots;
    PartColumns pc;
    pc.q_t.assign(n_slots, 0);
    pc.q_orig.assign(n_slots, -1);
    pc.r4.assign(n_slots, 0.0);
    pc.w.resize(n_slots);
    pc.nsteps.assign(n_qtiles, 0);
    pc.nsh.assign(n_qtiles, 0);
    // shared steps (tiles.h): only the plain dense shape has them
    if (ps.list_mode == 0 && ps.n_pass == 1 && ps.o_base == 0)
        for (size_t qt = 0; qt < n_qtiles; ++qt)
            pc.nsh[qt] = qo.tile_nsh[(size_t)ps.tile_lo + qt];
    double r4_q = NAN, r4_of_q = 0.0; // (neighbouring slots of a shared tile have one q: one pow for them)
    for (size_t ls = 0; ls < n_slots; ++ls) {
        const int64_t qi = qo.order[(size_t)ps.tile_lo * kQTileSlots + ls];
        if (qi < 0)
            continue; // padding column
        const int t_loc = std::min(ps.chunk + 1, std::max(0, (int)t_table[(size_t)qi] - ps.o_base));
        pc.q_t[ls] = t_loc;
        pc.q_orig[ls] = (int32_t)qi;
        const int64_t a = qi / (qo.n2 * qo.n3), b = (qi / qo.n3) % qo.n2, c = qi % qo.n3;
        const SlotQ w = {clamp_one(m->dm, 2, axes[2][a]), clamp_one(m->dm, 3, axes[3][b]), clamp_one(m->dm, 4, axes[4][c])};
        pc.w[ls] = w;
        if (!(w.q == r4_q)) {
            r4_q = w.q;
            r4_of_q = std::pow(1 - w.q, 4.0);
        }
        pc.r4[ls] = r4_of_q;
        const int steps = t_loc > 1 ? mfma_steps_of(t_loc - 1) : 0;
        pc.nsteps[ls / kQTileSlots] = std::max(pc.nsteps[ls / kQTileSlots], steps);
        pc.t_loc_max = std::max(pc.t_loc_max, t_loc);
    }
    return pc;
}

// n_ce_grid: the (c, e) pairs of the WHOLE grid.
PartGeometry part_geometry(int t_loc_max, int n_pass, int32_t n_qtiles, int64_t n_ce_grid)
{
    PartGeometry geo;
    geo.max_o = t_loc_max - 1;
    geo.pass_stride = mfma_steps_of(geo.max_o) * kStepColumns; // a pass begins on an MFMA step
    geo.n_columns = n_pass == 1 ? geo.max_o : n_pass * geo.pass_stride;
    geo.ld = factored_ld(geo.n_columns);
    geo.n_buf = factored_n_buf(geo.ld);
    const int n_units = 2 * n_qtiles; // (q-tile, half)
    // a unit needs at least one piece per pass: fewer units fit a wave's slots
    geo.units_per_wave = std::max(1, kMaxUnits / n_pass);
    geo.n_threads = (geo.n_columns <= 256 && n_units <= 4 * geo.units_per_wave) ? 256 : 512;
    const int cap_block = geo.n_waves() * geo.units_per_wave;
    // workgroups per (c, e): as many as the units need -- and, for a grid with few (c, e) pairs (optimize_grid's
    // have 36), enough to put the chip's 256 CUs to work: each rebuilds G, but they share the contraction and the logs
    // (decided by the WHOLE grid's (c, e) count, not the block's: a point's value may not depend on how the grid was
    // cut into blocks, and the assignment of units to waves fixes the order of its sums)
    // (as many as FIT the chip in one round: 36 (c, e) pairs x 8 would be 288 workgroups for 256 CUs, a second round for the
    // last 32 -- round 5: 7, by the trace of an optimize_grid search whose K-factored launches took 25 us for 15 keys)
    geo.one_block_a_pair = n_ce_grid >= 192;
    const int want_blocks = geo.one_block_a_pair ? 1 : (int)std::min<int64_t>(n_qtiles, std::max<int64_t>(1, 256 / n_ce_grid));
    geo.n_qblocks = std::max(std::max(1, (n_units + cap_block - 1) / cap_block), want_blocks);
    return geo;
}

// Cost model of the assignment, in MFMA steps: a unit costs its steps (in every pass) plus its share of the
// logs; a builder wave starts with the cost of phase A (tuned on C3 with the in-kernel stamps).  The charges, their
// overrides in tuning builds and the deal itself: unit_deal.h.
Charges planner_charges(const covest_model *m)
{
    Charges ch = {kUnitOverhead, kBuildCost, kSharedStepsPerMfma, kLastBuilderExtra, kMinSharedSteps, {}};
    // (with a tail an item may stand for up to 32 count-less tiles, tiles.h: the builders walk every one of them
    // while the contraction sees one item -- charge them for the tiles an item holds on average)
    const bool low_keys = m->has_tiles && m->tv.n_items > 0 && m->low_tile_share >= 0.75;
    if (m->has_tiles && m->tv.n_items > 0)
        ch.build_cost = (int)std::lround((double)(low_keys ? kBuildCostLowKeys : kBuildCost) *
                                         (double)m->tv.n_tiles / (double)m->tv.n_items);
    for (int w = 0; w < kBuildShareWaves; ++w)
        ch.build_share[w] = wave_share(low_keys, w);
#if defined(COVEST_DIAG) || defined(COVEST_TUNE)
    charges_from_env(ch);
#endif
    return ch;
}

// ---- deal (q-tile, half) units to the waves of a workgroup (tiles.h) ----
struct Unit {
    int tile, half, cost, pieces; // pieces: per pass
};

// The units of q-block `blk`, longest first into the lightest SIMD (waves w and w + 4 share one) that still has room,
// then into the lighter of that SIMD's waves with room.  held: [n_waves]
int place_units(int blk, const PartSpec &ps, const PartColumns &pc, const PartGeometry &geo, const Charges &ch,
                std::vector<std::vector<Unit>> &held)
{
    const int nw = geo.n_waves();
    std::vector<Unit> units;
    for (int qt = blk; qt < ps.n_qtiles(); qt += geo.n_qblocks) // tiles are sorted by T: interleave over blocks
        for (int h = 0; h < 2; ++h) {
            const int nsh = pc.nsh[(size_t)qt];
            units.push_back({qt, h, ps.n_pass * std::max(1, pc.mfma_steps(qt)) + ch.unit_overhead +
                                        (nsh ? 1 + (nsh + ch.shared_div - 1) / ch.shared_div : 0), 1});
        }
    std::stable_sort(units.begin(), units.end(), [](const Unit &a, const Unit &b) { return a.cost > b.cost; });
    // (the upper builder waves of a plain part skip the items whose limit lies below their copy numbers, band.h: what
    // they are charged for phase A falls with the wave -- unit_deal.h)
    const bool shares = wave_shares_apply(geo.one_block_a_pair, ps.list_mode, ps.n_pass, ps.o_base);
    std::vector<int> cost(units.size()), wave_of(units.size(), -1);
    for (size_t i = 0; i < units.size(); ++i)
        cost[i] = units[i].cost;
    // (two buffers: builders contract less, they fill the next key tile in the same interval)
    if (!deal_units(cost.data(), (int)units.size(), nw, geo.n_columns, geo.n_buf == 2, geo.units_per_wave, ch, shares, wave_of.data()))
        return fail(COVEST_E_INVALID, "K-factored plan: no wave has room for a unit (internal)");
    held.assign((size_t)nw, {});
    for (size_t i = 0; i < units.size(); ++i)
        held[(size_t)wave_of[i]].push_back(units[i]);
    return COVEST_OK;
}

// One wave's units cut into pieces and written to its slots, which begin at `slot0`.
void write_wave_slots(std::vector<Unit> &mine, size_t slot0, const PartSpec &ps, const PartColumns &pc,
                      const PartGeometry &geo, UnitTables &ut)
{
    const int n_pass = ps.n_pass;
    // cut the unit with the longest pieces once more (in every pass) while slots are free (tiles.h)
    auto piece_len = [&](const Unit &u) { return (pc.mfma_steps(u.tile) + u.pieces - 1) / u.pieces; };
    int used = (int)mine.size() * n_pass;
    while (used + n_pass <= kMaxUnits && !mine.empty()) {
        size_t longest = 0;
        for (size_t i = 1; i < mine.size(); ++i)
            if (piece_len(mine[i]) > piece_len(mine[longest]))
                longest = i;
        if (pc.nsh[(size_t)mine[longest].tile])
            break; // (a unit with shared steps is short already, and stays in one piece)
        Unit trial = mine[longest];
        trial.pieces += 1;
        if (piece_len(trial) < kMinPieceSteps)
            break;
        mine[longest].pieces += 1;
        used += n_pass;
    }
    // slots sorted by piece length (descending), the pieces of a unit adjacent
    std::stable_sort(mine.begin(), mine.end(), [&](const Unit &a, const Unit &b) { return piece_len(a) > piece_len(b); });
    size_t k = 0;
    for (const Unit &u : mine) {
        bool first = true;
        for (int pass = 0; pass < n_pass; ++pass)
            for (int p = 0; p < u.pieces; ++p, ++k) {
                ut.set(slot0 + k, u.tile, u.half, pass * (geo.pass_stride / kStepColumns) + p * piece_len(u),
                       1 + kStepColumns * p * piece_len(u), piece_len(u), !first, pc.nsh[(size_t)u.tile]);
                first = false;
            }
    }
}

int deal_qblock(int blk, const PartSpec &ps, const PartColumns &pc, const PartGeometry &geo, const Charges &ch, UnitTables &ut)
{
    std::vector<std::vector<Unit>> held;
    const int rc = place_units(blk, ps, pc, geo, ch, held);
    if (rc != COVEST_OK)
        return rc;
    for (int w = 0; w < geo.n_waves(); ++w)
        write_wave_slots(held[(size_t)w], ((size_t)blk * geo.n_waves() + w) * kMaxUnits, ps, pc, geo, ut);
    return COVEST_OK;
}

// Weights of slot `at`'s first two MFMA steps, per lane (lane = 16 * (o mod 4) + column), and its rho.
// piece_w: [slot][lane][2] = {first step, the step the kernel's running weight starts from} -- the second step of the
// piece, or (units with shared steps) the first step after them.
// (eight consecutive copy numbers per slot and column: one libm pow, the rest by multiplication -- the kernel
// advances the weights the same way from the third step on; a grid with few (c, e) pairs has many slots)
void slot_weights(size_t at, const PartSpec &ps, const PartColumns &pc, const UnitTables &ut, double *piece_w, double *unit_rho)
{
    const int qt = ut.tile[at], nsh = ut.nsh[at], o0 = ut.o0[at];
    const int o_first = ps.o_base + o0;
    // (the columns of a shared tile have ONE q: its powers are made once per slot, not once per column -- the same
    // calls of pow with the same arguments, so the same bits; they were most of a plan's build time, which is a third
    // of an optimize_grid iteration)
    double pw_q = NAN, pw_geo = 0.0, pw_16 = 0.0, pw_4 = 0.0, pw_inv = 0.0, pw_after = 0.0;
    for (int colx = 0; colx < kQTileSlots; ++colx) {
        const size_t ls = (size_t)qt * kQTileSlots + (size_t)colx;
        if (pc.q_orig[ls] < 0)
            continue; // padding column
        const double q1 = pc.w[ls].q1, q2 = pc.w[ls].q2, q = pc.w[ls].q;
        const double head = (1 - q1) * (1 - q2) * q, base = 1 - q;
        if (!(q == pw_q)) { // (NaN: never equal, made afresh)
            pw_q = q;
            pw_geo = o_first >= 3 ? std::pow(base, (double)(o_first - 3)) : 1.0;
            if (nsh > 0) {
                pw_16 = std::pow(base, 16.0);
                pw_4 = std::pow(base, 4.0);
                pw_inv = 1.0 / std::pow(base, 4.0 * (double)nsh);
                pw_after = std::pow(base, (double)(o_first + kStepColumns * (nsh + 1) - 3));
            }
        }
        double geo = pw_geo; // base^(o - 3) at o = max(o_first, 3)
        for (int d = 0; d < 2 * kStepColumns; ++d) {
            const int o = o_first + d;
            double w;
            if (o < 3) {
                w = copy_number_weight_host(q1, q2, q, o);
            } else {
                w = head * geo;
                geo *= base;
            }
            // (the piece's first step needs no mask in the kernel: a copy number at or beyond the column's
            // cut-off gets weight 0 here -- covest/models.py:239; later steps are cut off by the step count)
            if (d < kStepColumns && o0 + d >= (int)pc.q_t[ls])
                w = 0.0;
            // (units with shared steps: the second entry is the first step after them, written below)
            if (d < kStepColumns || nsh == 0)
                piece_w[(at * kStepLanes + (size_t)((d % kStepColumns) * kQTileSlots + colx)) * 2 + (size_t)(d / kStepColumns)] = w;
        }
        if (nsh > 0) {
            // (one q per tile: every live column writes the same values) -- the shared steps are summed with
            // weights RELATIVE TO THE FIRST of them, (1-q)^(4 (i - 1)) <= 1 (Horner in (1-q)^4, four chains in
            // (1-q)^16), and the MFMA that brings the sum in multiplies by b_o of that first step, which the kernel
            // makes from the weight it holds anyway -- b_o of the first step AFTER them -- times (1-q)^(-4 nsh)
            // (<= 1e10: the cut-off is where b_o reaches 1e-8)
            unit_rho[4 * at] = pw_16;
            unit_rho[4 * at + 1] = std::log(base); // ln(1-q): the unit's band is made from it (band.h)
            unit_rho[4 * at + 2] = pw_4;
            unit_rho[4 * at + 3] = pw_inv;
            // the first step after the shared ones: o = 5 + 4 nsh .. 8 + 4 nsh
            double g2 = pw_after; // base^(o_after - 3), o_after = o_first + 4 (nsh + 1)
            for (int d = 0; d < kStepColumns; ++d, g2 *= base)
                piece_w[(at * kStepLanes + (size_t)(d * kQTileSlots + colx)) * 2 + 1] = head * g2;
        }
    }
}

// The half-1 partner of every half-0 unit (the same workgroup holds both): looked up by the kernel's last step.
void pair_halves(UnitTables &ut, size_t block_slots)
{
    for (size_t b0 = 0; b0 < ut.size(); b0 += block_slots) {
        const size_t b1 = b0 + block_slots;
        for (size_t at = b0; at < b1; ++at) {
            if (ut.tile[at] < 0 || ut.half[at] != 0 || ut.cont[at])
                continue;
            for (size_t at2 = b0; at2 < b1; ++at2)
                if (ut.tile[at2] == ut.tile[at] && ut.half[at2] == 1 && !ut.cont[at2]) {
                    ut.pair[at] = (int32_t)(at2 - b0);
                    break;
                }
        }
    }
}

// The column limit (tiles.h FactoredPlan::col_floor, band_extra): the rule is band.h column_limit_of_block, q-block by
// q-block; one floor for the part, the largest of its q-blocks'.
int column_limit(const PartSpec &ps, const PartColumns &pc, const PartGeometry &geo, const UnitTables &ut, std::vector<int32_t> &extra)
{
    std::vector<int32_t> top((size_t)ps.n_qtiles(), 0); // the largest copy number a unit of the q-tile reads
    for (size_t ls = 0; ls < pc.q_t.size(); ++ls)
        top[ls / kQTileSlots] = std::max(top[ls / kQTileSlots], pc.q_t[ls] - 1);
    const bool plain = ps.list_mode == 0 && ps.n_pass == 1;
    const int n_build = std::min(geo.n_waves(), (geo.n_columns + 63) / 64);
    extra.assign((size_t)geo.n_qblocks * kBandExtra, -1);
    int floor = 1; // (copy number 1 is always read: the first builder wave never skips)
    for (int blk = 0; blk < geo.n_qblocks; ++blk) {
        const size_t b0 = (size_t)blk * geo.block_slots();
        floor = std::max(floor, column_limit_of_block(&ut.tile[b0], &ut.nsh[b0], &ut.cont[b0], top.data(), geo.n_waves(), kMaxUnits,
                                                      n_build, plain, 1, &extra[(size_t)blk * kBandExtra], kBandExtra));
    }
    return floor;
}

// Diagnostic builds only (tiles.h): the shipped library has no knob that changes values.
void apply_diag_env(FactoredPlan &pl)
{
#ifdef COVEST_DIAG
    if (std::getenv("COVEST_FACTORED_NBUF")) // (one buffer, or two where they fit)
        pl.n_buf = std::max(1, std::min(pl.n_buf, std::atoi(std::getenv("COVEST_FACTORED_NBUF"))));
    const char *skip = std::getenv("COVEST_FACTORED_SKIP");
    pl.skip_phases = skip ? std::atoi(skip) : 0;
    if (pl.list_mode == 0 && std::getenv("COVEST_FACTORED_DIAG")) { // leaked on purpose
        void *dp = nullptr;
        const size_t bytes = (size_t)(pl.ce_end - pl.ce_begin) * pl.n_qblocks * (pl.n_threads / 64) * 8 * sizeof(long long);
        if (hipMalloc(&dp, bytes) == hipSuccess && hipMemset(dp, 0, bytes) == hipSuccess) {
            pl.diag = static_cast<long long *>(dp);
            if (std::atoi(std::getenv("COVEST_FACTORED_DIAG")) >= 2)
                pl.skip_phases |= 0x10000; // the barrier waits by eighths of the walk instead of the phase sums
            if (std::atoi(std::getenv("COVEST_FACTORED_DIAG")) == 3)
                pl.skip_phases |= 0x20000; // ... of the first seven intervals one by one, the rest in the eighth
            if (std::atoi(std::getenv("COVEST_FACTORED_DIAG")) == 4)
                pl.skip_phases = (pl.skip_phases & ~0x10000) | 0x40000; // the stages outside the walk
            std::fprintf(stderr, "COVEST_FACTORED_DIAG %p %zu\n", dp, bytes);
        }
    }
#else
    (void)pl;
#endif
}

// One part of a dense grid, stage by stage.  q_orig_out: where the caller wants the part's q_orig (or null).
int build_plan_part(covest_grid *g, const double *const *axes, const std::vector<int32_t> &t_table, const QOrder &qo,
                    const PartSpec &ps, const Charges &ch, DevBuf &buf, FactoredPlan &pl, std::vector<int32_t> *q_orig_out)
{
    const covest_model *m = g->model;
    const PartColumns pc = part_columns(m, axes, t_table, qo, ps);
    if (q_orig_out)
        *q_orig_out = pc.q_orig;
    const PartGeometry geo =
        part_geometry(pc.t_loc_max, ps.n_pass, ps.n_qtiles(), std::max<int64_t>(1, g->len[0] * g->len[1]));
    UnitTables ut(geo.n_unit());
    for (int blk = 0; blk < geo.n_qblocks; ++blk) {
        const int rc = deal_qblock(blk, ps, pc, geo, ch, ut);
        if (rc != COVEST_OK)
            return rc;
    }
    std::vector<double> piece_w(ut.size() * kStepLanes * 2, 0.0), unit_rho(ut.size() * 4, 1.0);
    for (size_t at = 0; at < ut.size(); ++at)
        if (ut.tile[at] >= 0)
            slot_weights(at, ps, pc, ut, piece_w.data(), unit_rho.data());
    pair_halves(ut, geo.block_slots());
    std::vector<int32_t> band_extra;
    const int col_floor = column_limit(ps, pc, geo, ut, band_extra);
    // one buffer: doubles first (r4 | piece_w | rho), then int32 (q_T | q_orig | unit tables)
    PlanPack pack({{PlanPack::QR4, &pc.r4}, {PlanPack::PieceW, &piece_w}, {PlanPack::UnitRho, &unit_rho}},
                  {{PlanPack::QT, &pc.q_t}, {PlanPack::QOrig, &pc.q_orig}, {PlanPack::UnitTile, &ut.tile},
                   {PlanPack::UnitHalf, &ut.half}, {PlanPack::UnitS0, &ut.s0}, {PlanPack::UnitO0, &ut.o0},
                   {PlanPack::UnitLen, &ut.len}, {PlanPack::UnitCont, &ut.cont}, {PlanPack::UnitNsh, &ut.nsh},
                   {PlanPack::UnitPair, &ut.pair}, {PlanPack::BandExtra, &band_extra}});
    const int rc = upload_to_grid(g, buf, pack);
    if (rc != COVEST_OK)
        return rc;
    fill_plan(pl, geo, ps.n_pass, pack);
    pl.c_axis = g->src.axis[0];
    pl.e_axis = g->src.axis[1];
    pl.n_e = g->len[1];
    pl.n_q = qo.nq;
    pl.ce_begin = g->flat_begin / qo.nq;
    pl.ce_end = (g->flat_end + qo.nq - 1) / qo.nq;
    pl.n_qtiles = ps.n_qtiles();
    pl.o_base = ps.o_base;
    pl.flat_begin = g->flat_begin;
    pl.flat_end = g->flat_end;
    pl.list_mode = ps.list_mode;
    pl.p_clamp = clamp_for(m, qo.t_max);
    pl.ce_first = pl.ce_begin;
    pl.n_cols_partial = (int64_t)ps.n_qtiles() * kQTileSlots;
    pl.col_floor = col_floor;
    apply_diag_env(pl);
    return COVEST_OK;
}

// ---- the order of the weight vectors: slots of 16 per q-tile ----
struct ByThreshold { // descending threshold_o
    const std::vector<int32_t> &t_table;
    bool operator()(int32_t a, int32_t b) const { return t_table[(size_t)a] > t_table[(size_t)b]; }
};

// Shared steps (tiles.h) want the 16 columns of a tile to differ in q1 and q2 only: the n1 * n2 vectors of one q
// are then laid out by descending threshold_o and padded to whole tiles.  Padding columns cost logs, shared steps
// save MFMAs: taken when the padding stays below a third (n1 * n2 = 12, 16, 24, 27 .. 32, 36 ...), one lane per
// copy number (max_error <= 8).  (Diagnostic builds: COVEST_FACTORED_SHARE=0 switches it off for A/B runs.)
bool wants_shared_order(const QOrder &qo, int n_pass)
{
    const int64_t group = qo.n1 * qo.n2, group_padded = (group + kQTileSlots - 1) / kQTileSlots * kQTileSlots;
    bool share = n_pass == 1 && 3 * (group_padded - group) <= group;
#ifdef COVEST_DIAG
    if (const char *share_env = std::getenv("COVEST_FACTORED_SHARE"))
        share = share && std::atoi(share_env) != 0;
#endif
    return share;
}

// All weight vectors by descending threshold_o.  qo: the axis lengths and t_max set.
QOrder plain_order(QOrder qo, const std::vector<int32_t> &t_table)
{
    std::vector<int32_t> all((size_t)qo.nq);
    for (int64_t i = 0; i < qo.nq; ++i)
        all[(size_t)i] = (int32_t)i;
    std::stable_sort(all.begin(), all.end(), ByThreshold{t_table});
    qo.n_qtiles = (int32_t)((qo.nq + kQTileSlots - 1) / kQTileSlots);
    qo.order.assign((size_t)qo.n_qtiles * kQTileSlots, -1);
    std::copy(all.begin(), all.end(), qo.order.begin());
    qo.tile_nsh.assign((size_t)qo.n_qtiles, 0);
    return qo;
}

// Tile by tile: the slots of a tile share q (see wants_shared_order).  qo: the axis lengths and t_max set.
QOrder shared_order(QOrder qo, const std::vector<int32_t> &t_table, int chunk, int min_shared)
{
    struct Tile {
        int32_t slot[kQTileSlots];
        int t_hi, t_lo;
    };
    const int64_t group = qo.n1 * qo.n2;
    std::vector<Tile> tiles;
    std::vector<int32_t> one((size_t)group);
    for (int64_t c = 0; c < qo.n3; ++c) {
        for (int64_t ab = 0; ab < group; ++ab)
            one[(size_t)ab] = (int32_t)(ab * qo.n3 + c);
        std::stable_sort(one.begin(), one.end(), ByThreshold{t_table});
        for (int64_t at = 0; at < group; at += kQTileSlots) {
            Tile t;
            const int64_t live = std::min<int64_t>(kQTileSlots, group - at);
            for (int64_t i = 0; i < kQTileSlots; ++i)
                t.slot[i] = i < live ? one[(size_t)(at + i)] : -1;
            t.t_hi = (int)t_table[(size_t)t.slot[0]];
            t.t_lo = (int)t_table[(size_t)t.slot[live - 1]];
            tiles.push_back(t);
        }
    }
    std::stable_sort(tiles.begin(), tiles.end(), [](const Tile &a, const Tile &b) { return a.t_hi > b.t_hi; });
    qo.n_qtiles = (int32_t)tiles.size();
    qo.order.resize(tiles.size() * kQTileSlots);
    qo.tile_nsh.assign(tiles.size(), 0);
    for (size_t t = 0; t < tiles.size(); ++t) {
        std::copy(tiles[t].slot, tiles[t].slot + kQTileSlots, qo.order.begin() + (std::ptrdiff_t)t * kQTileSlots);
        // steps 1 .. nsh cover o = 5 .. 4 + 4 nsh, all below the tile's smallest threshold_o; a tile of the
        // long part (threshold_o - 1 > chunk) is contracted chunk by chunk, without them
        const int n = (tiles[t].t_lo - (kStepColumns + 1)) / kStepColumns;
        qo.tile_nsh[t] = (tiles[t].t_hi - 1 <= chunk && n >= min_shared) ? n : 0;
    }
    return qo;
}

// Useful flops of the contraction per row (covest_grid_work): 2 per (column, o < T) of the MFMA steps, 2 per
// (o mod 4 lane, shared step) and the 4-term MFMA per column that brings a shared sum in.
double contract_flops_per_row(const QOrder &qo, const std::vector<int32_t> &t_table)
{
    double flops = 0.0;
    for (int32_t t = 0; t < qo.n_qtiles; ++t) {
        const int n = qo.tile_nsh[(size_t)t];
        for (int i = 0; i < kQTileSlots; ++i) {
            const int32_t qi = qo.order[(size_t)t * kQTileSlots + (size_t)i];
            if (qi >= 0)
                flops += 2.0 * (double)((int)t_table[(size_t)qi] - 1 - kStepColumns * n) + (n ? 2.0 * kStepColumns : 0.0);
        }
        flops += 2.0 * kStepColumns * n;
    }
    return flops;
}

// largest threshold_o of a tile of the order: its first slot's
int tile_t_hi(const QOrder &qo, const std::vector<int32_t> &t_table, int32_t tile)
{
    return (int)t_table[(size_t)qo.order[(size_t)tile * kQTileSlots]];
}

// The long weight vectors -- the first n_long_tiles tiles of the order -- one part per chunk of copy numbers.
int build_long_parts(covest_grid *g, const double *const *axes, const std::vector<int32_t> &t_table, const QOrder &qo,
                     int32_t n_long_tiles, int chunk, int n_pass, const Charges &ch)
{
    const int n_chunks = (qo.t_max - 1 + chunk - 1) / chunk;
    g->long_parts.resize((size_t)n_chunks);
    for (int c = 0; c < n_chunks; ++c) {
        // tiles that still have copy numbers in this chunk: a prefix (sorted by threshold_o)
        int32_t hi = 0;
        while (hi < n_long_tiles && tile_t_hi(qo, t_table, hi) - 1 > c * chunk)
            ++hi;
        if (hi == 0) {
            g->long_parts.resize((size_t)c);
            break;
        }
        covest_grid::Part &part = g->long_parts[(size_t)c];
        const int rc = build_plan_part(g, axes, t_table, qo, PartSpec{0, hi, c * chunk, chunk, n_pass, 3}, ch, part.buf,
                                       part.plan, c == 0 ? &g->long_q_orig_host : nullptr);
        if (rc != COVEST_OK)
            return rc;
    }
    g->n_long_tiles = n_long_tiles;
    // q_orig of the long slots on the device, for ll_finish_dense (padded to whole tiles)
    g->long_q_orig_host.resize((size_t)n_long_tiles * kQTileSlots, -1);
    HIP_TRY(g->long_q_orig.reserve(g->long_q_orig_host.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(g->long_q_orig.ptr, g->long_q_orig_host.data(), g->long_q_orig_host.size() * sizeof(int32_t),
                      hipMemcpyHostToDevice));
    return COVEST_OK;
}

// The rest of the order, tiles [n_long_tiles, n_qtiles): one part that writes log-likelihoods -- or none.
int build_short_part(covest_grid *g, const double *const *axes, const std::vector<int32_t> &t_table, const QOrder &qo,
                     int32_t n_long_tiles, int chunk, int n_pass, const Charges &ch)
{
    g->has_short_part = n_long_tiles < qo.n_qtiles;
    g->n_shared_tiles = 0;
    for (int32_t t = n_long_tiles; t < qo.n_qtiles; ++t)
        g->n_shared_tiles += qo.tile_nsh[(size_t)t] > 0 ? 1 : 0;
    if (g->has_short_part)
        return build_plan_part(g, axes, t_table, qo, PartSpec{n_long_tiles, qo.n_qtiles, 0, chunk, n_pass, 0}, ch,
                               g->plan_buf, g->plan, nullptr);
    g->plan = FactoredPlan{};
    g->plan.n_q = qo.nq;
    g->plan.ce_begin = g->flat_begin / qo.nq;
    g->plan.ce_end = (g->flat_end + qo.nq - 1) / qo.nq;
    g->plan.max_o = 0;
    return COVEST_OK;
}

void release_long_parts(covest_grid *g)
{
    if (!g->long_parts.empty()) {
        (void)hipDeviceSynchronize(); // (their buffers go back to the process's cache, host.h)
        DeviceIdleScope idle;
        for (covest_grid::Part &part : g->long_parts)
            part.buf.release();
        g->long_parts.clear();
    }
    g->n_long_tiles = 0;
}

} // namespace

// All the parts of a dense repeats grid (see above).  g->has_plan stays false where K-factored does not apply:
// no tile table (keys beyond 16384 ...), more than 32 error classes, or more weight vectors than 2^24.
int build_factored_plan(covest_grid *g, const double *const *axes, const int64_t *axis_len,
                        const std::vector<int32_t> &t_table)
{
    covest_model *m = g->model;
    g->has_plan = false;
    release_long_parts(g);
    if (!m->has_tiles || m->n_par != 5 || m->dm.n_err > 32)
        return COVEST_OK;
    QOrder qo;
    qo.n1 = axis_len[2];
    qo.n2 = axis_len[3];
    qo.n3 = axis_len[4];
    qo.nq = qo.n1 * qo.n2 * qo.n3;
    if (qo.nq > (int64_t)1 << 24)
        return COVEST_OK;
    qo.t_max = 1;
    for (int64_t i = 0; i < qo.nq; ++i)
        qo.t_max = std::max(qo.t_max, (int)t_table[(size_t)i]);
    const int n_pass = (m->dm.n_err + 7) / 8;
    const int chunk = ((512 / n_pass) / kStepColumns) * kStepColumns; // copy numbers one workgroup's lanes hold
    g->t_max = qo.t_max;
    const Charges ch = planner_charges(m);
    qo = wants_shared_order(qo, n_pass) ? shared_order(std::move(qo), t_table, chunk, ch.min_shared)
                                        : plain_order(std::move(qo), t_table);
    g->contract_flops_per_row = contract_flops_per_row(qo, t_table);
    // the long weight vectors are the first tiles of the order
    int32_t n_long_tiles = 0;
    while (n_long_tiles < qo.n_qtiles && tile_t_hi(qo, t_table, n_long_tiles) - 1 > chunk)
        ++n_long_tiles;
    if (n_long_tiles > 0) {
        const int rc = build_long_parts(g, axes, t_table, qo, n_long_tiles, chunk, n_pass, ch);
        if (rc != COVEST_OK)
            return rc;
    }
    const int rc = build_short_part(g, axes, t_table, qo, n_long_tiles, chunk, n_pass, ch);
    if (rc != COVEST_OK)
        return rc;
    g->has_plan = qo.t_max >= 2;
    return COVEST_OK;
}

namespace {

struct ListTables {
    std::vector<double> axes, r4, piece_w; // axes: [2][n] the points' c, then their e
    std::vector<int32_t> q_t, q_orig;
    UnitTables ut;
    ListTables(size_t n, size_t n_unit)
        : axes(2 * n), r4(n * kQTileSlots, 0.0), piece_w(n_unit * kStepLanes * 2, 0.0), q_t(n * kQTileSlots, 0),
          q_orig(n * kQTileSlots, -1), ut(n_unit)
    {
    }
};

// Item p of n: the point `par` with threshold_o `t_point`, or its copy numbers from ob + 1 on.
void list_item(const covest_model *m, size_t p, size_t n, const double *par, int t_point, int ob, ListTables &lt)
{
    constexpr int NW = 8, MU = kMaxUnits;
    lt.axes[p] = par[0];
    lt.axes[n + p] = par[1];
    const double q1 = clamp_one(m->dm, 2, par[2]), q2 = clamp_one(m->dm, 3, par[3]), q = clamp_one(m->dm, 4, par[4]);
    // local threshold: the kernel's lanes count from the chunk's start, and a chunk ends after kListLanes copy numbers
    const int t = std::min(kListLanes + 1, std::max(0, t_point - ob));
    const size_t slot = p * kQTileSlots;
    lt.q_t[slot] = t;
    lt.q_orig[slot] = 0;
    lt.r4[slot] = std::pow(1 - q, 4.0);
    const int steps = t > 1 ? mfma_steps_of(t - 1) : 0;
    // the two halves of the key tile go to the workgroup's last two waves, each cut into equal pieces
    const int pieces = std::max(1, std::min(MU, steps / kMinPieceSteps));
    const int piece_len = std::max(1, (steps + pieces - 1) / pieces);
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < pieces; ++k) {
            const size_t at = (1 + 2 * p + (size_t)h) * MU + (size_t)k;
            lt.ut.set(at, (int)p, h, k * piece_len, 1 + kStepColumns * k * piece_len, piece_len, k > 0, 0);
            if (h == 0 && k == 0) // its half-1 partner: the first slot of the workgroup's last wave (tiles.h unit_pair)
                lt.ut.pair[at] = (NW - 1) * MU;
            for (int which = 0; which < 2; ++which)
                for (int kq = 0; kq < kStepColumns; ++kq) { // column 0 only: lanes 16 kq
                    const int o_local = 1 + kStepColumns * (k * piece_len + which) + kq;
                    // (the piece's first step comes masked by the cut-off, as in slot_weights)
                    lt.piece_w[(at * kStepLanes + (size_t)(kQTileSlots * kq)) * 2 + (size_t)which] =
                        (which == 0 && o_local >= t) ? 0.0 : copy_number_weight_host(q1, q2, q, ob + o_local);
                }
        }
}

} // namespace

// K-factored on a POINT LIST (tiles.h FactoredPlan::list_mode): every point is its own (c, e) workgroup with
// a q-tile of one real column.  What a refinement step needs -- a handful of points, each a full likelihood --
// then costs one workgroup's pass over the keys (the recurrence over o in 5 waves, a few MFMAs) instead of
// K-direct's single wave looping over every (key, o, s).  Built per call: ~13 KB of tables per point.
// An item is a point (o_base 0, list_mode 1) or a chunk of a point's copy numbers (list_mode 2): params of the
// point, threshold_o of the point, copy numbers before the chunk.
// in_place: the kernel reads the tables where they are staged -- page-locked host memory mapped into the device's
// address space -- instead of from a copy in HBM: for a handful of points (13 KB of tables each, read once by the
// point's 8 workgroups) the reads over the link cost less than the copy engine's start-up, 15-20 us of a single
// evaluation's 65.
int build_list_plan(covest_model *m, int64_t n, const double *params, const std::vector<int32_t> &t_list,
                    const std::vector<int32_t> *o_base_list, DevBuf &buf, FactoredPlan &pl, bool in_place)
{
    auto o_base_of = [&](int64_t i) { return o_base_list ? (*o_base_list)[(size_t)i] : 0; };
    int t_max = 1; // largest LOCAL threshold: copy numbers of an item are o_base + 1 .. o_base + t_local - 1
    for (int64_t i = 0; i < n; ++i)
        t_max = std::max(t_max, std::min(kListLanes + 1, (int)t_list[(size_t)i] - o_base_of(i)));
    // eight waves a workgroup, one workgroup per item: one empty wave block, then two per item (tiles.h list_mode)
    PartGeometry geo;
    geo.max_o = t_max - 1;
    geo.pass_stride = mfma_steps_of(geo.max_o) * kStepColumns;
    geo.n_columns = geo.max_o;
    geo.ld = factored_ld(geo.n_columns);
    geo.n_buf = factored_n_buf(geo.ld);
    geo.n_threads = 8 * 64;
    geo.units_per_wave = kMaxUnits;
    geo.n_qblocks = 1;
    ListTables lt((size_t)n, (1 + 2 * (size_t)n) * kMaxUnits);
    for (int64_t p = 0; p < n; ++p)
        list_item(m, (size_t)p, (size_t)n, params + p * 5, (int)t_list[(size_t)p], o_base_of(p), lt);
    // one buffer: doubles first (c | e | r4 | piece_w), then int32 (q_T | q_orig | unit tables, without unit_nsh)
    PlanPack pack({{PlanPack::Axes, &lt.axes}, {PlanPack::QR4, &lt.r4}, {PlanPack::PieceW, &lt.piece_w}},
                  {{PlanPack::QT, &lt.q_t}, {PlanPack::QOrig, &lt.q_orig}, {PlanPack::UnitTile, &lt.ut.tile},
                   {PlanPack::UnitHalf, &lt.ut.half}, {PlanPack::UnitS0, &lt.ut.s0}, {PlanPack::UnitLen, &lt.ut.len},
                   {PlanPack::UnitCont, &lt.ut.cont}, {PlanPack::UnitO0, &lt.ut.o0}, {PlanPack::UnitPair, &lt.ut.pair}});
    const int rc = upload_to_model(m, buf, in_place, pack);
    if (rc != COVEST_OK)
        return rc;
    fill_plan(pl, geo, 1, pack);
    pl.c_axis = pack.f64(PlanPack::Axes);
    pl.e_axis = pl.c_axis + n;
    pl.n_e = 1;
    pl.ce_begin = 0;
    pl.ce_end = n;
    pl.n_q = 1;
    pl.n_qtiles = (int32_t)n;
    pl.o_base = 0;
    pl.flat_begin = 0;
    pl.flat_end = n;
    pl.list_mode = 1;
    // (one value for every point list, whatever it holds: a point's value must not depend on its company)
    pl.p_clamp = clamp_for(m, kListLanes + 1);
    pl.n_seg = std::max(1, std::min(kListSegments, (int)m->tv.n_items)); // a function of the histogram alone
    return COVEST_OK;
}

} // namespace covest
