// tiles_host.cpp -- the host side of the recurrence kernels' tables: the bin views and the tile table (tiles.h).
//
// build_tiles, top to bottom (the stages are local to this file; each makes host vectors, one writer uploads):
//   cut_tiles             sorted bins -> tiles {k0, nb, run_start} and the rows' scal, cnt, row_bin
//   group_items           tiles -> plain and sum items
//   item_scales           K-factored's item_scal, item_iscal, item_lconst
//   closed_form_suffixes  K-basic's five suffix arrays and last_key
//   tile_flags, tile_records   all_zero / has_filler, and the gathered TileRecs
//   upload_table          fills the staging block through tile_view_from (tiles.h: the ONE layout) and copies it up
//   build_tiles           the driver: the three "no tiles" returns, the model's fields
#include "host.h"

using namespace covest;

namespace covest {

// One buffer, one copy: [key | lgam | cnt].
int upload_bins(DevBuf &buf, BinView &view, const std::vector<double> &key,
                const std::vector<double> &lgam, const std::vector<double> &cnt)
{
    const size_t n = key.size();
    view.n = (int64_t)n;
    view.key = view.lgam = view.cnt = nullptr;
    if (n == 0)
        return COVEST_OK;
    HIP_TRY(buf.reserve(3 * n * sizeof(double)));
    double *base = buf.as<double>();
    {
        SharedStage &ss = shared_stage();
        std::lock_guard<std::mutex> hold(ss.mu);
        HIP_TRY(ss.buf.reserve(3 * n * sizeof(double)));
        double *stage = ss.buf.as<double>();
        std::copy(key.begin(), key.end(), stage);
        std::copy(lgam.begin(), lgam.end(), stage + n);
        std::copy(cnt.begin(), cnt.end(), stage + 2 * n);
        HIP_TRY(hipMemcpy(base, stage, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    }
    view.key = base;
    view.lgam = base + n;
    view.cnt = base + 2 * n;
    return COVEST_OK;
}

namespace {

struct Tile {
    int k0, nb, run_start;
};

// The tiles and their rows, kTileBins a tile (rows past a tile's nb keys are padding: scale 0, count 0, no bin).
struct TileRows {
    std::vector<Tile> tiles;
    std::vector<double> scal, cnt; // (scal WITHOUT the 2^kBasicShift the device table carries: applied at the upload)
    std::vector<int32_t> row_bin;
    size_t n_tiles() const { return tiles.size(); }
    bool all_zero(size_t t) const
    {
        for (int b = 0; b < kTileBins; ++b)
            if (cnt[t * kTileBins + (size_t)b] != 0.0)
                return false;
        return true;
    }
};

// Keys sorted ascending, split into runs of consecutive keys (gaps of up to kGapFill keys are bridged with filler
// keys that are stepped over but neither logged nor summed), each run cut into tiles of <= 32 keys.
TileRows cut_tiles(const std::vector<HostBin> &bins)
{
    TileRows r;
    size_t i = 0;
    while (i < bins.size()) {
        // one run: keys bins[i..j) with gaps <= kGapFill
        size_t j = i + 1;
        while (j < bins.size() && bins[j].key - bins[j - 1].key <= kGapFill + 1)
            ++j;
        const int first = bins[i].key, last = bins[j - 1].key;
        size_t cur = i;
        for (int k0 = first; k0 <= last; k0 += kTileBins) {
            const int nb = std::min(kTileBins, last - k0 + 1);
            r.tiles.push_back({k0, nb, k0 == first ? 1 : 0});
            long double sc = ldexpl(1.0L, -kScaleBits);
            for (int b = 0; b < kTileBins; ++b) {
                double sv = 0.0, cv = 0.0;
                int32_t which = -1;
                if (b < nb) {
                    const int key = k0 + b;
                    sc /= (long double)key;
                    if (cur < j && bins[cur].key == key) {
                        sv = (double)sc;
                        cv = bins[cur].cnt;
                        which = bins[cur].index;
                        ++cur;
                    } // else a FILLER key (a gap of the histogram the recurrence walks through): scale 0, so
                      // that its p_j is exactly 0 -- it is no key of the reference's p_j dict, and must add
                      // nothing to sp_j (covest/models.py:103) and take no log
                }
                r.scal.push_back(sv);
                r.cnt.push_back(cv);
                r.row_bin.push_back(which);
            }
        }
        i = j;
    }
    return r;
}

// Items (tiles.h): a plain item is one tile; runs of all-zero-count tiles (they exist only with a tail) are grouped,
// up to 32 per sum item.
struct Items {
    std::vector<int32_t> first, ntiles, sum;
    std::vector<double> cnt; // [items][32]: the tile's counts for a plain item, 0 for a sum item
    size_t size() const { return first.size(); }
};

Items group_items(const TileRows &r)
{
#ifdef COVEST_DIAG
    const bool no_sum_items = std::getenv("COVEST_NO_SUM_ITEMS") != nullptr; // diagnostic builds: every tile a plain item
#else
    const bool no_sum_items = false;
#endif
    Items it;
    const size_t nt = r.n_tiles();
    for (size_t t = 0; t < nt;) {
        if (!r.all_zero(t) || no_sum_items) {
            it.first.push_back((int32_t)t);
            it.ntiles.push_back(1);
            it.sum.push_back(0);
            it.cnt.insert(it.cnt.end(), r.cnt.begin() + (std::ptrdiff_t)(t * kTileBins),
                          r.cnt.begin() + (std::ptrdiff_t)((t + 1) * kTileBins));
            ++t;
            continue;
        }
        size_t e = t + 1;
        while (e < nt && e - t < (size_t)kTileBins && r.all_zero(e))
            ++e;
        it.first.push_back((int32_t)t);
        it.ntiles.push_back((int32_t)(e - t));
        it.sum.push_back(1);
        it.cnt.insert(it.cnt.end(), (size_t)kTileBins, 0.0);
        t = e;
    }
    return it;
}

// K-factored's view of the rows (tiles.h): the scale of a plain item's rows as a factor (and its reciprocal, for
// the clamp in the row's units) and as the constant it adds to the item's sum of h_j log p_j
struct ItemScales {
    std::vector<double> scal, iscal, lconst;
};

ItemScales item_scales(const TileRows &r, const Items &it)
{
    const size_t ni = it.size();
    ItemScales s{std::vector<double>(ni * kTileBins, 0.0), std::vector<double>(ni * kTileBins, 0.0), std::vector<double>(ni, 0.0)};
    for (size_t i = 0; i < ni; ++i) {
        if (it.sum[i]) {
            for (int b = 0; b < kTileBins; ++b)
                s.scal[i * kTileBins + (size_t)b] = 1.0;
            continue;
        }
        const size_t t = (size_t)it.first[i];
        long double lc = 0.0L, lratio = 0.0L; // ln((k0-1)!/(k0+b)!) = -sum_{i=k0}^{k0+b} ln i
        for (int b = 0; b < r.tiles[t].nb; ++b) {
            lratio -= logl((long double)(r.tiles[t].k0 + b));
            const double sv = r.scal[t * kTileBins + (size_t)b];
            if (sv == 0.0)
                continue; // filler key
            s.scal[i * kTileBins + (size_t)b] = sv;
            if (r.cnt[t * kTileBins + (size_t)b] != 0.0) // (a row without a count takes no log and is never "low": 0)
                s.iscal[i * kTileBins + (size_t)b] = 1.0 / sv;
            lc += (long double)r.cnt[t * kTileBins + (size_t)b] * lratio;
        }
        s.lconst[i] = (double)lc;
    }
    return s;
}

// K-basic's closed form (ll_basic.hip): suffix sums over the counted keys of the tiles t .. nt - 1, entry nt: 0
struct Suffixes {
    std::vector<double> h, jh, lgh, first, first_lg; // [nt + 1]
    std::vector<double> last_key;                    // [2] the last counted key of the table and its ln j!
};

Suffixes closed_form_suffixes(const TileRows &r)
{
    const size_t nt = r.n_tiles();
    const std::vector<double> zeros(nt + 1, 0.0);
    Suffixes s{zeros, zeros, zeros, zeros, zeros, std::vector<double>(2, 0.0)};
    long double s_h = 0.0L, s_jh = 0.0L, s_lgh = 0.0L;
    double first_key = 0.0, first_lg = 0.0;
    for (size_t t = nt; t-- > 0;) {
        for (int b = r.tiles[t].nb - 1; b >= 0; --b) {
            const double h = r.cnt[t * kTileBins + (size_t)b];
            if (h == 0.0)
                continue;
            const int key = r.tiles[t].k0 + b;
            const double lg = lgamma_at(key);
            s_h += (long double)h;
            s_jh += (long double)h * (long double)key;
            s_lgh += (long double)h * (long double)lg;
            first_key = (double)key;
            first_lg = lg;
            if (s.last_key[0] == 0.0) { // the first one met from the end: the last counted key
                s.last_key[0] = (double)key;
                s.last_key[1] = lg;
            }
        }
        s.h[t] = (double)s_h;
        s.jh[t] = (double)s_jh;
        s.lgh[t] = (double)s_lgh;
        s.first[t] = first_key;
        s.first_lg[t] = first_lg;
    }
    return s;
}

struct TileFlags {
    std::vector<int32_t> all_zero, has_filler;
};

TileFlags tile_flags(const TileRows &r, const Items &it)
{
    const size_t nt = r.n_tiles();
    TileFlags f{std::vector<int32_t>(nt, 0), std::vector<int32_t>(nt, 0)};
    for (size_t i = 0; i < it.size(); ++i)
        if (it.sum[i])
            for (int32_t k = 0; k < it.ntiles[i]; ++k)
                f.all_zero[(size_t)(it.first[i] + k)] = 1;
    for (size_t t = 0; t < nt; ++t) // a row inside the tile's keys that is no key of the histogram
        for (int b = 0; b < r.tiles[t].nb; ++b)
            if (r.row_bin[t * kTileBins + (size_t)b] < 0)
                f.has_filler[t] = 1;
    return f;
}

// A tile's constants in one record (tiles.h TileRec; pad stays 0).
std::vector<TileRec> tile_records(const TileRows &r, const TileFlags &f)
{
    std::vector<TileRec> recs(r.n_tiles());
    for (size_t t = 0; t < recs.size(); ++t) {
        const Tile &tl = r.tiles[t];
        TileRec &rec = recs[t];
        rec.k0 = (double)tl.k0;
        rec.lgam_prev = lgamma_of_factorial((int64_t)tl.k0 - 1);
        rec.lgam_last = lgamma_of_factorial((int64_t)(tl.k0 + tl.nb) - 1);
        long double rn = 1.0L;
        for (int b = 0; b < tl.nb; ++b)
            rn /= (long double)(tl.k0 + b);
        rec.renorm = (double)rn;
        rec.nb = tl.nb;
        rec.run_start = tl.run_start;
        rec.all_zero = f.all_zero[t];
        rec.has_filler = f.has_filler[t];
    }
    return recs;
}

// What the stages made, as the writer takes it.
struct HostTable {
    TileRows rows;
    Items items;
    ItemScales scales;
    Suffixes suf;
    std::vector<TileRec> recs;
};

// The table's one block, doubles then int32 (tiles.h: tile_dbl_count, tile_int_count), as a view.
TileView view_over(int32_t nt, int32_t ni, const double *block)
{
    return tile_view_from(nt, ni, block, reinterpret_cast<const int32_t *>(block + tile_dbl_count(nt, ni)));
}

// A view built over the STAGING block names host memory this file owns: the only place the view's const is cast away.
template <class T> T *staged(const T *p) { return const_cast<T *>(p); }
template <class T> void fill(const T *dst, const std::vector<T> &src) { std::copy(src.begin(), src.end(), staged(dst)); }

// Stages the whole table in the process's page-locked block -- zeroed first: the cache-line padding in front of the
// records is part of the upload -- and copies it to `buf` in one piece.  Every array's place comes from tile_view_from.
int upload_table(DevBuf &buf, const HostTable &h)
{
    const int32_t nt = (int32_t)h.rows.n_tiles(), ni = (int32_t)h.items.size();
    const size_t bytes = (size_t)tile_dbl_count(nt, ni) * sizeof(double) + (size_t)tile_int_count(nt, ni) * sizeof(int32_t);
    HIP_TRY(buf.reserve(bytes));
    SharedStage &ss = shared_stage();
    std::lock_guard<std::mutex> hold(ss.mu);
    HIP_TRY(ss.buf.reserve(bytes)); // one copy instead of five
    std::memset(ss.buf.ptr, 0, bytes);
    const TileView sv = view_over(nt, ni, ss.buf.as<double>());
    for (size_t t = 0; t < h.recs.size(); ++t) { // the per-tile arrays: what the records gather, once more
        const TileRec &r = h.recs[t];
        staged(sv.first_key)[t] = r.k0;
        staged(sv.lgam_prev)[t] = r.lgam_prev;
        staged(sv.lgam_last)[t] = r.lgam_last;
        staged(sv.renorm)[t] = r.renorm;
        staged(sv.n_bins)[t] = r.nb;
        staged(sv.run_start)[t] = r.run_start;
        staged(sv.all_zero)[t] = r.all_zero;
        staged(sv.has_filler)[t] = r.has_filler;
    }
    // tiles.h kBasicShift (exact: a power of two, and 2^-540 (k0-1)!/(k0+b)! >= 1e-303)
    std::transform(h.rows.scal.begin(), h.rows.scal.end(), staged(sv.scal), [](double v) { return v * kBasicScale; });
    fill(sv.cnt, h.rows.cnt);
    fill(sv.row_bin, h.rows.row_bin);
    fill(sv.item_cnt, h.items.cnt);
    fill(sv.item_first, h.items.first);
    fill(sv.item_ntiles, h.items.ntiles);
    fill(sv.item_sum, h.items.sum);
    fill(sv.item_scal, h.scales.scal);
    fill(sv.item_iscal, h.scales.iscal);
    fill(sv.item_lconst, h.scales.lconst);
    fill(sv.suf_h, h.suf.h);
    fill(sv.suf_jh, h.suf.jh);
    fill(sv.suf_lgh, h.suf.lgh);
    fill(sv.suf_first, h.suf.first);
    fill(sv.suf_first_lg, h.suf.first_lg);
    fill(sv.last_key, h.suf.last_key);
    fill(sv.rec, h.recs);
    HIP_TRY(hipMemcpy(buf.ptr, ss.buf.ptr, bytes, hipMemcpyHostToDevice));
    return COVEST_OK;
}

} // namespace

// Tile table of streams.h over the evaluated bins.  Leaves has_tiles false (and returns COVEST_OK) when the fast
// kernels do not apply.
int build_tiles(covest_model *m, std::vector<HostBin> bins)
{
    m->has_tiles = false;
    if (m->dm.n_err > 32 || bins.empty()) // (the recurrence kernels hold max_error <= 32 error classes)
        return COVEST_OK;
    std::sort(bins.begin(), bins.end(), [](const HostBin &a, const HostBin &b) { return a.key < b.key; });
    if (bins.front().key < 1 || bins.back().key > kMaxFastKey)
        return COVEST_OK;
    HostTable h;
    h.rows = cut_tiles(bins);
    h.items = group_items(h.rows);
    h.scales = item_scales(h.rows, h.items);
    h.suf = closed_form_suffixes(h.rows);
    h.recs = tile_records(h.rows, tile_flags(h.rows, h.items));
    const size_t nt = h.rows.n_tiles(), ni = h.items.size();
    m->rows_contracted = (double)ni * kTileBins;
    size_t low = 0;
    for (const Tile &tl : h.rows.tiles)
        low += tl.k0 <= kLowKeyTile ? 1 : 0;
    m->low_tile_share = nt ? (double)low / (double)nt : 0.0;
    m->keys_logged = 0.0;
    for (double c : h.rows.cnt)
        m->keys_logged += c != 0.0 ? 1.0 : 0.0;
    const int rc = upload_table(m->tiles_buf, h);
    if (rc != COVEST_OK)
        return rc;
    m->tv = view_over((int32_t)nt, (int32_t)ni, m->tiles_buf.as<double>());
    m->has_tiles = true;
    return COVEST_OK;
}

// p_clamp of handback.h for a launch whose largest threshold_o is t_max.
double clamp_for(const covest_model *m, int t_max)
{
    return (double)(m->dm.n_err + std::max(t_max, 2)) * kClampPerTerm;
}

} // namespace covest
