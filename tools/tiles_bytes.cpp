// tiles_bytes.cpp -- the tile table (tiles_host.cpp: build_tiles) and a grid handle's set-up (abi_grid.cpp:
// covest_grid_create / covest_grid_reset) without a GPU: everything they upload, every view they bind (pointers as
// offsets), the model's and the handle's fields and every HIP call they make, written to a file that two builds must
// produce identically.  HIP and host_common.cpp are replaced by tools/host_standins.h; the planner, threshold_o and the
// launchers by the stand-ins below (the same on both sides).  tools/tiles_bytes.sh builds it against a revision's two
// files and the tree's and compares.  `tiles_bytes OUT time N` times input N instead.
#include "host_standins.h"
#include <chrono>
#include <functional>
#include <map>
#include <random>

namespace covest {
// threshold_o look-alike: where a geometric weight falls below 1e-8, capped at 600
void threshold_table(const covest_model *, const double *a1, int64_t n1, const double *a2, int64_t n2, const double *a3, int64_t n3, int32_t *out)
{
    for (int64_t a = 0; a < n1; ++a)
        for (int64_t b = 0; b < n2; ++b)
            for (int64_t k = 0; k < n3; ++k) {
                const double q = std::min(std::max(a3[k], 1e-3), 1.0), q1 = std::min(std::max(a1[a], 0.0), 1.0), q2 = std::min(std::max(a2[b], 0.0), 1.0);
                int t = 1;
                if (q1 < 1) {
                    t = 3;
                    const double head = (1 - q1) * (1 - q2) * q;
                    if (head > 0 && q < 1)
                        t = 3 + (int)std::max(0.0, std::ceil(std::log(1e-8 / head) / std::log(1 - q)));
                }
                out[(a * n2 + b) * n3 + k] = std::min(t, 600);
            }
}
// the planner's place: it stages a table of its own behind the handle's (64 bytes a weight vector), as the real one does
int build_factored_plan(covest_grid *g, const double *const *, const int64_t *axis_len, const std::vector<int32_t> &t)
{
    const size_t bytes = 64 * t.size();
    HIP_TRY(g->plan_buf.reserve(bytes));
    StageSlot slot;
    int rc = grid_stage_begin(g, bytes, slot);
    if (rc != COVEST_OK)
        return rc;
    memset(slot.ptr, 0x33, bytes);
    rc = grid_stage_commit(g, slot, g->plan_buf.ptr, bytes);
    g->has_plan = true;
    g->t_max = *std::max_element(t.begin(), t.end());
    (void)axis_len;
    return rc;
}
int resolve_kernel(const covest_model *, int32_t, const covest_grid *) { return 0; }
SubList sub_list_of(const covest_model *, int, void *, void *, void *) { return SubList{}; }
hipError_t launch_ll(const covest_model *, int, const PointSource &, int64_t, double *, const SubList &, hipStream_t, const char **, const covest_grid *) { return hipSuccess; }
void *pinned_block_take() { return calloc(1, kPinnedBlockBytes); }
void pinned_block_give(void *) {}
int64_t launch_record_text(const LaunchRecord &, char *, int64_t) { return 0; }
LaunchRecordScope::LaunchRecordScope(LaunchRecord &) : prev(nullptr) {}
LaunchRecordScope::LaunchRecordScope(LaunchRecord &, bool) : prev(nullptr) {}
LaunchRecordScope::~LaunchRecordScope() {}
hipError_t launch_ll_unfixed(const covest_model *, int, const PointSource &, int64_t, double *, const SubList &, hipStream_t, const char **, const covest_grid *) { return hipSuccess; }
hipError_t launch_ll_fix_list(const DevModel &, const TileView &, const PointSource &, double *, const SubList &, hipStream_t, int64_t) { return hipSuccess; }
hipError_t launch_argmin_proving(const double *, int64_t, int64_t, double *, int64_t *, ArgminResult *, ArgminResult *, unsigned *, const int64_t *, hipStream_t) { return hipSuccess; }
hipError_t launch_argmin(const double *, int64_t, int64_t, double *, int64_t *, ArgminResult *, ArgminResult *, unsigned *, hipStream_t) { return hipSuccess; }
hipError_t launch_argmin_scan(const double *, int64_t, int64_t, double, ArgminResult *, ArgminResult *, ScanRecords *, unsigned *, hipStream_t) { return hipSuccess; }
bool axis_min_plan(const int64_t *, int, uint32_t, int64_t, int64_t, AxisMinPlan *) { return false; }
hipError_t launch_axis_min(const AxisMinPlan &, const double *, double *, int64_t *, double *, int64_t *, hipStream_t) { return hipSuccess; }
} // namespace covest

static FILE *out;
static std::map<std::string, int> g_reached; // inputs that reached each feature the issue lists
static void reached(const char *f, bool yes) { g_reached[f] += yes ? 1 : 0; }
static unsigned long long fnv(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i)
        h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}
static void dump_bytes(const char *tag, const void *p, size_t n)
{
    fprintf(out, "%s %zu bytes fnv %016llx\n", tag, n, fnv(p, n));
    fwrite(p, 1, n, out);
    fputc('\n', out);
}
static void dump_log()
{
    fprintf(out, "calls:\n%s", g_hip_log.c_str());
    g_hip_log.clear();
}

// ---- build_tiles
typedef std::vector<std::pair<int, double>> Hist; // (key, count), any order
static std::vector<HostBin> bins_of(const Hist &h, bool keep_zero)
{
    std::vector<HostBin> b;
    for (auto &kv : h)
        if (keep_zero || kv.second != 0.0)
            b.push_back({kv.first, kv.second, (int32_t)b.size()});
    return b;
}
static Hist read_hist(const std::string &path)
{
    Hist h;
    FILE *f = fopen(path.c_str(), "r");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path.c_str());
        exit(2);
    }
    char line[256];
    long k;
    double c;
    while (fgets(line, sizeof line, f))
        if (line[0] != '#' && sscanf(line, "%ld %lf", &k, &c) == 2)
            h.push_back({(int)k, c});
    if (h.empty()) {
        fprintf(stderr, "no bins in %s\n", path.c_str());
        exit(2);
    }
    fclose(f);
    return h;
}
static void input_features(std::vector<HostBin> b, int n_err)
{
    std::sort(b.begin(), b.end(), [](const HostBin &x, const HostBin &y) { return x.key < y.key; });
    bool g0 = false, g1 = false, g2 = false;
    for (size_t i = 1; i < b.size(); ++i) {
        const int d = b[i].key - b[i - 1].key;
        g0 |= d == kGapFill, g1 |= d == kGapFill + 1, g2 |= d == kGapFill + 2;
    }
    reached("gap kGapFill", g0), reached("gap kGapFill+1 (bridged)", g1), reached("gap kGapFill+2 (new run)", g2);
    reached("key 1", !b.empty() && b.front().key == 1), reached("key kMaxFastKey", !b.empty() && b.back().key == kMaxFastKey);
    reached("single bin", b.size() == 1);
    reached("no tiles: n_err > 32", n_err > 32), reached("no tiles: empty", b.empty());
    reached("no tiles: key out of range", !b.empty() && n_err <= 32 && (b.front().key < 1 || b.back().key > kMaxFastKey));
}
static void run_tiles(const std::string &tag, int n_err, const std::vector<HostBin> &bins)
{
    covest_model m;
    m.dm.n_err = n_err;
    input_features(bins, n_err);
    const int rc = build_tiles(&m, bins);
    fprintf(out, "== tiles %s n_err=%d bins=%zu rc=%d has_tiles=%d rows=%a low=%a logged=%a\n", tag.c_str(), n_err, bins.size(), rc, m.has_tiles,
            m.rows_contracted, m.low_tile_share, m.keys_logged);
    if (m.has_tiles) {
        const TileView &v = m.tv;
        const char *base = (const char *)m.tiles_buf.ptr;
        const void *ptrs[] = {v.dbl_base, v.int_base, v.first_key, v.n_bins, v.run_start, v.all_zero, v.has_filler, v.lgam_prev, v.lgam_last, v.renorm, v.scal,
                              v.cnt, v.item_cnt, v.item_scal, v.item_iscal, v.item_lconst, v.suf_h, v.suf_jh, v.suf_lgh, v.suf_first, v.suf_first_lg,
                              v.last_key, v.item_first, v.item_ntiles, v.item_sum, v.row_bin, v.rec};
        fprintf(out, "view nt=%d ni=%d off", v.n_tiles, v.n_items);
        for (const void *p : ptrs)
            fprintf(out, " %ld", (long)((const char *)p - base));
        fputc('\n', out);
        dump_bytes("table", base, alloc_size(base));
        bool cap = false, between = false, zero_tile = false;
        for (int i = 0; i < v.n_items; ++i) {
            cap |= v.item_sum[i] && v.item_ntiles[i] == kTileBins && i + 1 < v.n_items && v.item_sum[i + 1];
            between |= v.item_sum[i] && i > 0 && i + 1 < v.n_items && !v.item_sum[i - 1] && !v.item_sum[i + 1];
        }
        for (int t = 0; t < v.n_tiles; ++t) {
            bool z = true;
            for (int b = 0; b < kTileBins; ++b)
                z &= v.cnt[t * kTileBins + b] == 0.0;
            zero_tile |= z;
        }
        reached("sum item at its cap of 32 tiles", cap), reached("sum item between plain ones", between);
        reached("COVEST_NO_SUM_ITEMS (diag build)", getenv("COVEST_NO_SUM_ITEMS") && zero_tile && v.n_items == v.n_tiles);
    }
    dump_log();
}
static Hist random_hist(std::mt19937_64 &rng, int kind)
{
    Hist h;
    int key = kind % 3 == 0 ? 1 : 1 + (int)(rng() % 40);
    const int gaps[] = {1, kGapFill, kGapFill + 1, kGapFill + 2, kGapFill + 3, 2, 5, 40};
    const int n_seg = 2 + (int)(rng() % 6);
    for (int s = 0; s < n_seg && key <= kMaxFastKey; ++s) {
        // a stretch of consecutive keys: counted, or (kinds with a tail) count-less -- some long enough for > 32 tiles
        const bool zero = kind % 2 == 1 && s % 2 == 1;
        const int len = zero ? (rng() % 3 == 0 ? 1100 + (int)(rng() % 1500) : 40 + (int)(rng() % 200)) : 1 + (int)(rng() % 150);
        for (int i = 0; i < len && key <= kMaxFastKey; ++i, ++key)
            if (zero || rng() % 7)
                h.push_back({key, zero ? 0.0 : (double)(1 + rng() % 100000)});
        key += gaps[rng() % 8] - 1;
    }
    if (kind % 5 == 4 && (h.empty() || h.back().first < kMaxFastKey))
        h.push_back({kMaxFastKey, 3.0});
    std::shuffle(h.begin(), h.end(), rng);
    return h;
}
static void all_tiles(const std::string &golden)
{
    for (const char *name : {"H256", "H10k_basic", "H10k_rep", "H10k_basic_trim", "H10k_rep_trim"}) {
        const bool trimmed = strstr(name, "_trim") != nullptr; // (a tail model passes zero-count keys on)
        run_tiles(name, 8, bins_of(read_hist(golden + "/" + name + ".hist"), trimmed));
    }
    run_tiles("single bin", 8, bins_of({{77, 5.0}}, false));
    run_tiles("n_err 33", 33, bins_of({{3, 5.0}, {4, 1.0}}, false));
    run_tiles("empty", 8, {});
    run_tiles("key 0", 8, bins_of({{0, 5.0}, {4, 1.0}}, false));
    run_tiles("key beyond kMaxFastKey", 8, bins_of({{3, 5.0}, {kMaxFastKey + 1, 1.0}}, false));
    run_tiles("keys 1 and kMaxFastKey", 32, bins_of({{1, 5.0}, {kMaxFastKey, 1.0}}, false));
    run_tiles("the three gaps", 8, bins_of({{5, 1.0}, {5 + kGapFill, 2.0}, {6 + 2 * kGapFill, 3.0}, {8 + 3 * kGapFill, 4.0}}, false));
    {
        Hist h; // plain, 40 count-less tiles (a sum item at its cap, then a second), plain
        for (int k = 1; k <= 42 * kTileBins; ++k)
            h.push_back({k, k <= kTileBins || k > 41 * kTileBins ? 7.0 : 0.0});
        run_tiles("zero run past the cap", 8, bins_of(h, true));
        h.resize(5 * kTileBins);
        h.push_back({5 * kTileBins + 1, 9.0});
        run_tiles("sum item between plain ones", 8, bins_of(h, true));
    }
    std::mt19937_64 rng(2024);
    for (int i = 0; i < 48; ++i)
        run_tiles("random " + std::to_string(i), 1 + (int)(rng() % 32), bins_of(random_hist(rng, i), i % 2 == 1));
}

// ---- covest_grid_create / covest_grid_reset
static std::string where(const covest_grid *g, const void *p)
{
    if (!p)
        return "null";
    auto in = [&](const void *b, size_t cap) { return b && (const char *)p >= (const char *)b && (const char *)p < (const char *)b + cap; };
    auto rel = [&](const char *name, const void *b) { return std::string(name) + "+" + std::to_string((const char *)p - (const char *)b); };
    if (in(g->arena.ptr, g->arena.cap))
        return rel("arena", g->arena.ptr);
    if (in(g->stage.ptr, g->stage.cap))
        return rel("stage", g->stage.ptr);
    if (in(shared_stage().buf.ptr, shared_stage().buf.cap))
        return rel("shared", shared_stage().buf.ptr);
    for (size_t i = 0; i < g->stage_retired.size(); ++i)
        if (in(g->stage_retired[i].ptr, g->stage_retired[i].cap))
            return rel(("retired" + std::to_string(i)).c_str(), g->stage_retired[i].ptr);
    return "elsewhere";
}
struct GridCase {
    std::vector<int64_t> len;
    int64_t begin, end;
    const char *what;
};
static std::vector<std::vector<double>> axes_of(const GridCase &c, std::mt19937_64 &rng)
{
    std::vector<std::vector<double>> ax(c.len.size());
    for (size_t d = 0; d < c.len.size(); ++d)
        for (int64_t i = 0; i < std::max<int64_t>(c.len[d], 0); ++i)
            ax[d].push_back(d < 2 ? 1.0 + (double)(rng() % 30000) / 1000.0 : d == 4 ? 0.02 + 1.0 * (double)i / (double)c.len[d] : (double)(rng() % 1100) / 1000.0 - 0.05);
    return ax;
}
static void dump_grid(const char *call, const GridCase &c, int rc, const covest_grid *g)
{
    fprintf(out, "== grid %s (%s) rc=%d error=\"%s\"\n", call, c.what, rc, rc ? g_last_error.c_str() : "");
    g_last_error.clear();
    if (!g) {
        dump_log();
        return;
    }
    fprintf(out, "configured=%d flat=%ld..%ld len=%ld,%ld,%ld,%ld,%ld async=%d pending=%d clean=%d stage_off=%zu retired=%zu has_plan=%d evaluated=%d sum=%a qsum=%a\n",
            g->configured, (long)g->flat_begin, (long)g->flat_end, (long)g->len[0], (long)g->len[1], (long)g->len[2], (long)g->len[3], (long)g->len[4],
            g->async_uploads, g->upload_pending, g->counter_clean, g->stage_off, g->stage_retired.size(), g->has_plan, g->evaluated, g->sum_t_minus_1, g->q_sum_t_minus_1);
    if (g->configured && rc == 0) {
        const covest_grid::View *views[] = {&g->axes, &g->t_table, &g->ll, &g->sub_index, &g->sub_word, &g->sub_ctl, &g->partial_val, &g->partial_idx, &g->result};
        fprintf(out, "views");
        for (const covest_grid::View *v : views)
            fprintf(out, " %s", where(g, v->ptr).c_str());
        fprintf(out, "\nsrc grid=%d flat_begin=%ld t_table=%s", g->src.is_grid, (long)g->src.flat_begin, where(g, g->src.t_table).c_str());
        for (int d = 0; d < kMaxParams; ++d)
            fprintf(out, " %ld:%s", (long)g->src.len[d], where(g, g->src.axis[d]).c_str());
        fputc('\n', out);
        const size_t staged = (size_t)((const char *)g->ll.ptr - (const char *)g->arena.ptr); // [counter | axes | table], rounded
        dump_bytes("staged", (const char *)g->axes.ptr - 8, staged);
        const bool in_place = where(g, g->axes.ptr).compare(0, 5, "arena") != 0;
        reached("grid: read in place", in_place), reached("grid: copied", !in_place);
        reached("grid: staging block retired", !g->stage_retired.empty());
        reached("grid: ragged block", g->flat_begin > 0 && g->flat_end < g->len[0] * g->len[1] * g->len[2] * g->len[3] * g->len[4]);
        reached("grid: counter cleared by a memset", g_hip_log.find("hipMemsetAsync") != std::string::npos);
    }
    reached("grid: argument error", rc != 0);
    dump_log();
}
static void grid_sequence(int n_par, std::mt19937_64 &rng)
{
    covest_model m;
    m.n_par = n_par;
    auto L = [&](std::vector<int64_t> five) { five.resize((size_t)n_par); return five; };
    const std::vector<GridCase> seq = {
        {L({24, 16, 4, 2, 5}), 0, -1, "create, small"},
        {L({24, 16, 4, 2, 5}), 0, -1, "reset, same shape: first in place"},
        {L({24, 16, 4, 2, 5}), 0, -1, "reset, same shape: counter left clean"},
        {L({32, 16, 4, 2, 4}), 0, -1, "reset, other axis lengths, more points: in place, the arena grows, the counter is cleared"},
        {L({6, 6, 6, 6, 6}), 0, -1, "reset, optimize_grid's 6^5 (basic: 6^2)"},
        {L({300, 200, 4, 2, 5}), 1000, 59000, "reset, large: copied, the arena grows"},
        {L({24, 16, 4, 2, 5}), 5, 3001, "reset, small again, ragged"},
        {L({70000, 3, 1, 1, 2}), 100, 9000, "reset, axes beyond the staging block: retired, read in place"},
        {L({70000, 3, 1, 1, 2}), 0, -1, "reset, the same axes, whole grid: copied"},
        {L({5, 4, 3, 2, 2}), 0, 0, "reset, empty block"},
        {L({24, 16, 4, 2, 5}), -1, -1, "error: negative flat_begin"},
        {L({24, 16, 4, 2, 5}), 9, 3, "error: flat_begin beyond flat_end"},
        {L({24, 16, 4, 2, 5}), 0, 1 << 30, "error: flat_end beyond the grid"},
        {L({24, 0, 4, 2, 5}), 0, -1, "error: an axis without a value"},
        {L({1 << 21, 1 << 21, 1 << 21, 2, 2}), 0, -1, n_par == 5 ? "error: grid too large" : "reset, 2^42 points asked of no allocation? no: basic has two axes"},
        {L({24, 16, 4, 2, 5}), 0, -1, "reset after the errors"}};
    covest_grid *g = nullptr;
    for (size_t i = 0; i < seq.size(); ++i) {
        GridCase c = seq[i];
        if (n_par == 2 && c.len[0] == (1 << 21))
            continue; // (two such axes are a valid 2^42-point grid: nothing to allocate it in)
        auto ax = axes_of(c, rng);
        std::vector<const double *> ptr;
        for (auto &a : ax)
            ptr.push_back(a.data());
        const int rc = i == 0 ? covest_grid_create(&m, n_par, ptr.data(), c.len.data(), c.begin, c.end, &g)
                              : covest_grid_reset(g, n_par, ptr.data(), c.len.data(), c.begin, c.end);
        dump_grid(i == 0 ? "create" : "reset", c, rc, g);
        if (i == 2) { // the remaining argument errors, on a configured handle
            ptr[1] = nullptr;
            dump_grid("reset", {c.len, 0, -1, "error: a null axis"}, covest_grid_reset(g, n_par, ptr.data(), c.len.data(), 0, -1), g);
            dump_grid("reset", {c.len, 0, -1, "error: null axes"}, covest_grid_reset(g, n_par, nullptr, c.len.data(), 0, -1), g);
            dump_grid("reset", {c.len, 0, -1, "error: null axis_len"}, covest_grid_reset(g, n_par, ptr.data(), nullptr, 0, -1), g);
            dump_grid("reset", {c.len, 0, -1, "error: n_axes"}, covest_grid_reset(g, n_par + 1, ptr.data(), c.len.data(), 0, -1), g);
            covest_grid *g2 = nullptr;
            dump_grid("create", {c.len, 0, -1, "error: create with a null axis"}, covest_grid_create(&m, n_par, ptr.data(), c.len.data(), 0, -1, &g2), g2);
        }
    }
    covest_grid_destroy(g);
    dump_log();
}

// ---- host time
static double best_us(const std::function<void()> &f)
{
    double best = 1e30;
    for (int rep = 0; rep < 7; ++rep) {
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < 300; ++i)
            f();
        best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 300);
    }
    return best;
}
static int time_input(int which, const std::string &golden)
{
    const char *names[] = {"build_tiles H10k_rep", "build_tiles H10k_rep_trim", "grid_configure C3's shape (32x32x16x1x16)", "grid_configure 6^5"};
    covest_model m;
    double us = 0;
    if (which < 2) {
        m.dm.n_err = 8;
        const std::vector<HostBin> bins = bins_of(read_hist(golden + (which ? "/H10k_rep_trim.hist" : "/H10k_rep.hist")), which == 1);
        build_tiles(&m, bins);
        g_timing = true;
        us = best_us([&] { build_tiles(&m, bins); });
    } else {
        m.n_par = 5;
        std::mt19937_64 rng(7);
        GridCase c{which == 2 ? std::vector<int64_t>{32, 32, 16, 1, 16} : std::vector<int64_t>{6, 6, 6, 6, 6}, 0, -1, ""};
        auto ax = axes_of(c, rng);
        std::vector<const double *> ptr;
        for (auto &a : ax)
            ptr.push_back(a.data());
        covest_grid *g = nullptr;
        covest_grid_create(&m, 5, ptr.data(), c.len.data(), 0, -1, &g);
        covest_grid_reset(g, 5, ptr.data(), c.len.data(), 0, -1);
        g_timing = true;
        us = best_us([&] { covest_grid_reset(g, 5, ptr.data(), c.len.data(), 0, -1); });
    }
    printf("%-44s %8.2f us (best of 7 x 300)\n", names[which], us);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string golden = argc > 2 ? argv[2] : "tests/golden";
    if (argc > 4 && !strcmp(argv[3], "time"))
        return time_input(atoi(argv[4]), golden);
    out = fopen(argv[1], "wb");
    all_tiles(golden);
    std::mt19937_64 rng(99);
    grid_sequence(2, rng);
    grid_sequence(5, rng);
    fclose(out);
    int missed = 0;
    for (auto &kv : g_reached) {
        const bool no_sums = getenv("COVEST_NO_SUM_ITEMS") != nullptr; // (then there is no sum item to reach)
        const bool need = kv.first.find("diag build") != std::string::npos ? no_sums : kv.first.find("sum item") != std::string::npos ? !no_sums : true;
        printf("  %-40s %d inputs%s\n", kv.first.c_str(), kv.second, need && !kv.second ? "  MISSED" : "");
        missed += need && !kv.second;
    }
    printf("features missed: %d\n", missed);
    return missed ? 1 : 0;
}
