// plan_bytes.cpp -- K-factored's planner (plan_factored.cpp) without a GPU: every byte it uploads and every field of every
// FactoredPlan it fills, over dense grids (shared and plain order, 1 to 4 passes, q-blocks, long parts, tails; each built
// twice on one handle) and point lists (list modes 1 and 2, in place and copied), written to a file that two builds of the
// planner must produce identically.  HIP and the staging of host.h are replaced by malloc and memcpy, clamp_one and clamp_for
// by look-alikes (pure functions of the same arguments): tools/host_standins.h, shared with tools/tiles_bytes.cpp.
// tools/plan_bytes.sh builds it against a revision's planner and the tree's and compares.  A third argument N times the plan
// of dense case N instead.
#define STANDIN_GRID_STAGE
#include "host_standins.h"
#include <random>
#include <chrono>
namespace covest {
double clamp_for(const covest_model *m, int t_max) { return (m->dm.n_err + t_max) * 7e-317; }
}
static FILE *out;
static const char *g_base; static size_t g_cap;
static long off(const void *p) { if (!p) return -1; const char *c = (const char*)p; return (c >= g_base && c < g_base + g_cap) ? (long)(c - g_base) : -2; }
static void dump_plan(const char *tag, const FactoredPlan &p, const void *base, size_t cap)
{
    g_base = (const char*)base; g_cap = cap;
    fprintf(out, "%s n_e=%ld ce=%ld..%ld n_q=%ld n_qtiles=%d max_o=%d n_pass=%d stride=%d cols=%d o_base=%d nt=%d hu=%d qb=%d ld=%d nbuf=%d "
            "flat=%ld..%ld mode=%d clamp=%a n_seg=%d ce_first=%ld ncp=%ld skip=%d\n  off c=%ld e=%ld tile=%ld half=%ld s0=%ld o0=%ld len=%ld cont=%ld nsh=%ld pair=%ld rho=%ld pw=%ld "
            "nst=%ld nf=%ld qT=%ld qo=%ld f8=%ld r4=%ld ob=%ld part=%ld diag=%ld\n", tag, (long)p.n_e, (long)p.ce_begin, (long)p.ce_end, (long)p.n_q, p.n_qtiles, p.max_o, p.n_pass, p.pass_stride,
            p.n_columns, p.o_base, p.n_threads, p.half_units, p.n_qblocks, p.ld, p.n_buf, (long)p.flat_begin, (long)p.flat_end, p.list_mode, p.p_clamp, p.n_seg,
            (long)p.ce_first, (long)p.n_cols_partial, p.skip_phases, off(p.c_axis), off(p.e_axis), off(p.unit_tile), off(p.unit_half), off(p.unit_s0), off(p.unit_o0), off(p.unit_len), off(p.unit_cont),
            off(p.unit_nsh), off(p.unit_pair), off(p.unit_rho), off(p.piece_w), off(p.qtile_nsteps), off(p.qtile_nfull), off(p.q_T), off(p.q_orig), off(p.q_first8), off(p.q_r4),
            off(p.item_obase), off(p.partial), off(p.diag));
}
static void dump_bytes(const char *tag, const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    fprintf(out, "%s %zu bytes fnv %016llx\n", tag, n, h);
    fwrite(p, 1, n, out); fputc('\n', out);
}
int main(int argc, char **argv)
{
    out = fopen(argv[1], "wb");
    std::mt19937_64 rng(12345);
    auto uni = [&](double a, double b) { return a + (b - a) * (rng() >> 11) * (1.0 / 9007199254740992.0); };
    int n_cases = 0;
    // dense: (n_err, n_ce0, n_ce1, n1, n2, n3, t cap, q lo, tail-ish scaling, async)
    struct Case { int n_err; int64_t l0, l1, n1, n2, n3; int t_cap; double qlo; int n_tiles, n_items; double low; };
    std::vector<Case> cases = {
        {8, 2, 2, 4, 1, 8, 61, 0.3, 0, 0, 0}, {8, 32, 32, 16, 1, 16, 10000, 0.05, 0, 0, 0}, {8, 32, 32, 16, 1, 16, 3000, 0.05, 40, 12, 0.9},
        {12, 1, 2, 2, 1, 5, 61, 0.1, 0, 0, 0}, {22, 2, 2, 7, 6, 16, 61, 0.08, 0, 0, 0}, {32, 2, 2, 7, 6, 16, 61, 0.08, 9, 9, 0.2},
        {8, 2, 2, 4, 2, 4, 281, 0.03, 0, 0, 0}, {8, 2, 2, 4, 2, 4, 451, 0.03, 0, 0, 0}, {8, 2, 2, 4, 4, 6, 61, 0.04, 0, 0, 0},
        {8, 2, 2, 3, 3, 6, 61, 0.04, 0, 0, 0}, {8, 2, 1, 4, 2, 4, 1601, 0.0105, 0, 0, 0}, {22, 2, 1, 4, 2, 4, 1601, 0.0105, 5, 3, 0.8},
        {8, 6, 6, 6, 6, 6, 16, 0.3, 0, 0, 0}, {8, 6, 6, 3, 6, 6, 16, 0.3, 0, 0, 0}, {8, 6, 6, 6, 6, 6, 2000, 0.01, 0, 0, 0},
        {8, 2049, 2049, 1, 1, 2, 21, 0.3, 0, 0, 0}, {8, 16, 12, 6, 6, 6, 33, 0.5, 3, 2, 1.0}, {8, 16, 12, 6, 6, 6, 129, 0.3, 0, 0, 0}};
    for (int rep = 0; rep < 40; ++rep)
        cases.push_back({(int)(1 + rng() % 32), (int64_t)(1 + rng() % 40), (int64_t)(1 + rng() % 40), (int64_t)(1 + rng() % 9), (int64_t)(1 + rng() % 7),
                         (int64_t)(1 + rng() % 20), (int)(2 + rng() % 2500), uni(0.005, 0.5), (int)(rng() % 3 ? 0 : 20 + rng() % 30), (int)(1 + rng() % 20), uni(0, 1)});
    for (const Case &c : cases) {
        covest_model m; m.n_par = 5; m.has_tiles = true; m.dm.n_err = c.n_err;
        for (int d = 0; d < 5; ++d) { m.dm.lo[d] = 0.0; m.dm.hi[d] = d >= 2 ? 1.0 : 1e9; }
        m.tv.n_tiles = c.n_tiles; m.tv.n_items = c.n_items; m.low_tile_share = c.low;
        covest_grid g; g.model = &m;
        std::vector<std::vector<double>> ax(5);
        int64_t lens[5] = {c.l0, c.l1, c.n1, c.n2, c.n3};
        for (int d = 0; d < 5; ++d) for (int64_t i = 0; i < lens[d]; ++i)
            ax[d].push_back(d < 2 ? uni(1, 30) : d == 4 ? c.qlo + (1.02 - c.qlo) * (double)i / (double)std::max<int64_t>(1, lens[d] - 1) : uni(-0.05, 1.05));
        const double *axes[5]; for (int d = 0; d < 5; ++d) { axes[d] = ax[d].data(); g.len[d] = lens[d]; }
        g.src.axis[0] = axes[0]; g.src.axis[1] = axes[1];
        const int64_t nq = c.n1 * c.n2 * c.n3, total = c.l0 * c.l1 * nq;
        g.flat_begin = total / 7; g.flat_end = total - total / 5;
        std::vector<int32_t> tt((size_t)nq);
        for (int64_t a = 0; a < c.n1; ++a) for (int64_t b = 0; b < c.n2; ++b) for (int64_t k = 0; k < c.n3; ++k) {
            const double q = std::min(std::max(ax[4][k], 1e-3), 1.0), q1 = std::min(std::max(ax[2][a], 0.0), 1.0), q2 = std::min(std::max(ax[3][b], 0.0), 1.0);
            // a threshold_o look-alike: where b_o falls below 1e-8, capped
            int t = 1; if (q1 < 1) { t = 3; const double head = (1 - q1) * (1 - q2) * q; if (head > 0 && q < 1) t = 3 + (int)std::max(0.0, std::ceil(std::log(1e-8 / head) / std::log(1 - q))); }
            tt[(size_t)((a * c.n2 + b) * c.n3 + k)] = std::min(t, c.t_cap);
        }
        if (argc > 2) {
            g_timing = true;
            if (n_cases != atoi(argv[2])) { ++n_cases; continue; }
            double best = 1e30;
            for (int rep = 0; rep < 7; ++rep) {
                auto t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < 300; ++i) build_factored_plan(&g, axes, lens, tt);
                best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 300);
            }
            printf("case %d: %.2f us a plan (best of 7 x 300) n_qblocks=%d n_qtiles=%d long=%d\n", n_cases, best, g.plan.n_qblocks, g.plan.n_qtiles, g.n_long_tiles);
            return 0;
        }
        for (int pass = 0; pass < 2; ++pass) { // the second build on the same handle: long parts released and rebuilt
            const int rc = build_factored_plan(&g, axes, lens, tt);
            fprintf(out, "== dense case %d pass %d rc=%d has_plan=%d short=%d long_tiles=%d shared=%d t_max=%d flops=%a parts=%zu\n", n_cases, pass, rc, g.has_plan,
                    g.has_short_part, g.n_long_tiles, g.n_shared_tiles, g.t_max, g.contract_flops_per_row, g.long_parts.size());
            if (rc) continue;
            if (g.has_plan && g.has_short_part) { dump_plan("short", g.plan, g.plan_buf.ptr, g.plan_buf.cap); dump_bytes("short", g.plan_buf.ptr, alloc_size(g.plan_buf.ptr)); }
            else dump_plan("noshort", g.plan, nullptr, 0);
            for (auto &part : g.long_parts) { dump_plan("long", part.plan, part.buf.ptr, part.buf.cap); dump_bytes("long", part.buf.ptr, alloc_size(part.buf.ptr)); }
            if (g.n_long_tiles) dump_bytes("long_q_orig", g.long_q_orig.ptr, g.long_q_orig_host.size() * 4);
        }
        ++n_cases;
    }
    // point lists
    for (int rep = 0; rep < 30; ++rep) {
        covest_model m; m.n_par = 5; m.has_tiles = true; m.dm.n_err = 8; m.tv.n_items = 1 + rng() % 40;
        for (int d = 0; d < 5; ++d) { m.dm.lo[d] = 0.0; m.dm.hi[d] = d >= 2 ? 1.0 : 1e9; }
        const int64_t n = rep < 3 ? 1 : 1 + rng() % 50;
        std::vector<double> par((size_t)n * 5); std::vector<int32_t> t((size_t)n), ob((size_t)n);
        for (int64_t i = 0; i < n; ++i) { par[i*5] = uni(1, 30); par[i*5+1] = uni(0.001, 0.1); par[i*5+2] = uni(-0.1, 1.1); par[i*5+3] = uni(-0.1, 1.1); par[i*5+4] = uni(0.005, 1.05);
            t[i] = (int32_t)(1 + rng() % (rep % 2 ? 3000 : 513)); ob[i] = (int32_t)(512 * (rng() % 4)); }
        DevBuf buf; FactoredPlan pl;
        const bool chunks = rep % 2, in_place = rep % 3 == 0;
        const int rc = build_list_plan(&m, n, par.data(), t, chunks ? &ob : nullptr, buf, pl, in_place);
        fprintf(out, "== list %d n=%ld chunks=%d in_place=%d rc=%d\n", rep, (long)n, chunks, in_place, rc);
        const void *base = in_place ? m.ws_stage.ptr : buf.ptr;
        dump_plan("list", pl, base, (size_t)1 << 30);
        size_t bytes = (size_t)n * (2 + 16) * 8 + (size_t)(1 + 2 * n) * 6 * 128 * 8 + (size_t)n * 32 * 4 + (size_t)(1 + 2 * n) * 6 * 7 * 4;
        dump_bytes("list", base, bytes);
    }
    fclose(out);
    return 0;
}
