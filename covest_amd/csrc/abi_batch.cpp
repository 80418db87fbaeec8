// abi_batch.cpp -- covest_batch_* of the C ABI over ll_batch.hip: a batch of histograms on one model's key set, scored
// in one pass.  The argument rules, the chunking of a point list against the table budget and
// the cut of launches are batch_host.h's (plain C++, checked without a device).  A batch borrows its model; every call
// takes the model's lock and works on the model's device.
#include "host.h"

#include "batch_host.h"
#include "draw_host.h"

using namespace covest;

static_assert(kBatchHostTableBytes == kBatchTableBytes && kBatchHostMaxHist == kBatchMaxHist, "one budget, one cap");

struct covest_batch {
    covest_model *model = nullptr;
    int64_t n_hist = 0, n_keys = 0;
    DevBuf counts, tails;    // H[n_hist][n_keys], tails[n_hist]
    DevBuf zero_cnt;         // the count array of the table's DevModel: n_keys zeros
    DevBuf table, tl, dead;  // one chunk: log p [points][n_keys], log(1 - sp), keys with p <= 0 per point
    DevBuf points;           // a call's parameters, behind them its thresholds (repeats model)
    DevBuf out;              // a chunk's values: [n_hist][points of the chunk] (cross), [points] (pairs)
    DevBuf index, dead_list; // a pairs call's histogram numbers; the chunk's points with dead keys
    DevBuf run_val, run_idx; // the running arg-min of covest_batch_argmin_cross
    DevBuf partial, fin;     // the gradient's table: the derivative kernel's segment sums; its finishing pass's value
                             // [points] and gradient [points][P] (the tail coefficients before they are packed into tl)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ~covest_batch()
    {
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
    }
};

namespace {

int refuse(const char *who, const char *what) { return fail(COVEST_E_INVALID, std::string(who) + ": " + what); }

// the view over EVERY key (covest_probabilities uploads it the same way, on first use)
int ensure_all_bins(covest_model *m)
{
    if (m->all_bins_ready)
        return COVEST_OK;
    COVEST_TRY(upload_bins(m->bins_all, m->all_bins, m->host_all_key, m->host_all_lgam, m->host_all_cnt));
    m->all_bins_ready = true;
    return COVEST_OK;
}

// The model the table kernel evaluates: every key, counts 0, tail 1 -- direct_point_ll's value is then log(1 - sp).
DevModel table_model(const covest_batch *b)
{
    DevModel full = b->model->dm;
    full.bins = b->model->all_bins;
    full.bins.cnt = b->zero_cnt.as<double>();
    full.tail = 1.0;
    return full;
}

// what every batch holds besides its histograms
int batch_prepare(covest_batch *b)
{
    COVEST_TRY(ensure_all_bins(b->model));
    const size_t bytes = (size_t)b->n_keys * sizeof(double);
    HIP_TRY(b->zero_cnt.reserve(bytes));
    HIP_TRY(hipMemsetAsync(b->zero_cnt.ptr, 0, bytes, nullptr));
    for (hipEvent_t &e : b->ev)
        HIP_TRY(hipEventCreate(&e));
    return COVEST_OK;
}

// A call's point list on the device: parameters | thresholds.  src describes the whole list.
int upload_points(covest_batch *b, int64_t n, const double *params, PointSource &src)
{
    const covest_model *m = b->model;
    const int P = m->n_par;
    const size_t par_bytes = (size_t)n * P * sizeof(double);
    std::vector<int32_t> t;
    if (P == 5) {
        t.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            t[(size_t)i] = threshold_for_point(m, params + i * 5);
    }
    HIP_TRY(b->points.reserve(par_bytes + t.size() * sizeof(int32_t)));
    COVEST_TRY(stage_upload(b->points.ptr, params, par_bytes, "covest_batch: upload of the points"));
    if (!t.empty())
        COVEST_TRY(stage_upload(b->points.as<char>() + par_bytes, t.data(), t.size() * sizeof(int32_t),
                                "covest_batch: upload of the thresholds"));
    src = PointSource{};
    src.is_grid = 0;
    src.params = b->points.as<double>();
    src.t_list = P == 5 ? reinterpret_cast<const int32_t *>(b->points.as<char>() + par_bytes) : nullptr;
    return COVEST_OK;
}

PointSource points_from(const PointSource &src, int64_t first, int P)
{
    PointSource part = src;
    part.params = src.params + first * P;
    part.t_list = src.t_list ? src.t_list + first : nullptr;
    return part;
}

// The table of one chunk (points first .. first + nc of the list), and its points with dead keys: listed on the device
// (dead_list) and counted in *n_dead.  ev[0] .. ev[1] bracket the kernel.
int table_chunk(covest_batch *b, const PointSource &src, int64_t first, int64_t nc, int64_t *n_dead)
{
    const covest_model *m = b->model;
    HIP_TRY(hipEventRecord(b->ev[0], nullptr));
    HIP_TRY(launch_batch_table(table_model(b), points_from(src, first, m->n_par), nc, b->table.as<double>(),
                               b->tl.as<double>(), b->dead.as<int32_t>(), false, nullptr));
    HIP_TRY(hipEventRecord(b->ev[1], nullptr));
    std::vector<int32_t> dead((size_t)nc), list;
    HIP_TRY(hipMemcpy(dead.data(), b->dead.ptr, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nc; ++i)
        if (dead[(size_t)i] > 0)
            list.push_back((int32_t)i);
    *n_dead = (int64_t)list.size();
    if (!list.empty()) {
        HIP_TRY(b->dead_list.reserve(list.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(b->dead_list.ptr, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    b->info[0] += nc;
    b->info[1] += 1;
    b->info[3] += *n_dead;
    return COVEST_OK;
}

int reserve_chunk(covest_batch *b, int64_t nc_max)
{
    if (nc_max > std::numeric_limits<int32_t>::max())
        return fail(COVEST_E_UNSUPPORTED, "covest_batch: more than 2^31 points in a table chunk");
    HIP_TRY(b->table.reserve((size_t)nc_max * (size_t)b->n_keys * sizeof(double)));
    HIP_TRY(b->tl.reserve((size_t)nc_max * sizeof(double)));
    HIP_TRY(b->dead.reserve((size_t)nc_max * sizeof(int32_t)));
    return COVEST_OK;
}

// ---- the gradient: a table of R = P + 1 rows a point from the derivative kernel's walk ----
int rows_per_point(const covest_batch *b) { return b->model->n_par + 1; }

int reserve_grad_chunk(covest_batch *b, int64_t nc_max)
{
    const int64_t R = rows_per_point(b);
    if (nc_max * R > std::numeric_limits<int32_t>::max())
        return fail(COVEST_E_UNSUPPORTED, "covest_batch: more than 2^31 rows in a table chunk");
    HIP_TRY(b->table.reserve((size_t)nc_max * (size_t)R * (size_t)b->n_keys * sizeof(double)));
    HIP_TRY(b->tl.reserve((size_t)nc_max * (size_t)R * sizeof(double)));
    HIP_TRY(b->dead.reserve((size_t)nc_max * sizeof(int32_t)));
    HIP_TRY(b->partial.reserve(ll_deriv_partial_bytes(table_model(b), 1, nc_max)));
    HIP_TRY(b->fin.reserve((size_t)nc_max * (size_t)R * sizeof(double)));
    return COVEST_OK;
}

// table_chunk for the gradient: rows (P + 1) i .. of b->table are point i's, b->tl holds its P + 1 tail coefficients, and
// dead_list names the VALUE row (P + 1) i of every point with dead keys -- what launch_batch_fix_dead indexes by.
int grad_table_chunk(covest_batch *b, const PointSource &src, int64_t first, int64_t nc, int64_t *n_dead)
{
    const covest_model *m = b->model;
    const int R = rows_per_point(b);
    double *fin_ll = b->fin.as<double>(), *fin_grad = fin_ll + nc;
    HIP_TRY(hipEventRecord(b->ev[0], nullptr));
    HIP_TRY(launch_ll_deriv_table(table_model(b), points_from(src, first, m->n_par), nc, b->partial.as<double>(),
                                  b->table.as<double>(), b->dead.as<int32_t>(), fin_ll, fin_grad, nullptr));
    HIP_TRY(launch_batch_tail_pack(fin_ll, fin_grad, nc, R, b->tl.as<double>(), nullptr));
    HIP_TRY(hipEventRecord(b->ev[1], nullptr));
    std::vector<int32_t> dead((size_t)nc), list;
    HIP_TRY(hipMemcpy(dead.data(), b->dead.ptr, (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nc; ++i)
        if (dead[(size_t)i] > 0)
            list.push_back((int32_t)(i * R));
    *n_dead = (int64_t)list.size();
    if (!list.empty()) {
        HIP_TRY(b->dead_list.reserve(list.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(b->dead_list.ptr, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    b->info[0] += nc;
    b->info[1] += 1;
    b->info[3] += *n_dead;
    return COVEST_OK;
}

void add_elapsed(covest_batch *b, int slot, hipEvent_t from, hipEvent_t to)
{
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, from, to) == hipSuccess)
        b->info[slot] += (int64_t)((double)ms * 1e6);
    else
        (void)hipGetLastError();
}

// Every histogram at every point, chunk by chunk of the table; `after(first, nc)` takes a chunk's values from b->out
// ([n_hist][nc], row length nc).  Called with the model locked and its device current.
template <class After>
int cross_chunks(covest_batch *b, int64_t n, const double *params, After after)
{
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    const int64_t per = batch_points_per_chunk(b->n_keys, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_chunk(b, nc_max));
    HIP_TRY(b->out.reserve((size_t)b->n_hist * (size_t)nc_max * sizeof(double)));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0, tiles = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(table_chunk(b, src, first, nc, &n_dead));
        HIP_TRY(hipEventRecord(b->ev[2], nullptr));
        HIP_TRY(launch_batch_cross(b->counts.as<double>(), b->tails.as<double>(), b->n_hist, b->table.as<double>(),
                                   b->tl.as<double>(), nc, b->n_keys, b->out.as<double>(), nc, &tiles, nullptr));
        HIP_TRY(hipEventRecord(b->ev[3], nullptr));
        b->info[2] += tiles;
        if (n_dead > 0) {
            HIP_TRY(launch_batch_fix_dead(b->counts.as<double>(), b->n_hist, b->table.as<double>(), b->n_keys,
                                          b->dead_list.as<int32_t>(), n_dead, b->out.as<double>(), nc, nullptr));
            b->info[4] += b->n_hist * n_dead;
        }
        COVEST_TRY(after(first, nc));
        HIP_TRY(hipEventSynchronize(b->ev[3])); // (the events are the next chunk's too)
        add_elapsed(b, 6, b->ev[0], b->ev[1]);
        add_elapsed(b, 7, b->ev[2], b->ev[3]);
    }
    return COVEST_OK;
}

struct BatchCall { // the opening of an entry point on a batch: the model's lock, its device, fresh counters
    std::unique_lock<std::mutex> hold;
    std::optional<DeviceGuard> guard;
    int status = COVEST_OK;
    explicit BatchCall(covest_batch *b, bool counters = true) : hold(b->model->lock)
    {
        status = guard.emplace(b->model->device).status();
        if (counters)
            std::fill(b->info, b->info + 8, (int64_t)0);
    }
};

int new_batch(covest_model *m, int64_t n_hist, covest_batch **out)
{
    covest_batch *b = new (std::nothrow) covest_batch();
    if (!b)
        return fail(COVEST_E_NOMEM, "covest_batch: out of host memory");
    b->model = m;
    b->n_hist = n_hist;
    b->n_keys = m->n_keys;
    *out = b;
    return COVEST_OK;
}

void drop_batch(covest_batch *b) // with the batch's device current
{
    (void)hipDeviceSynchronize(); // (its small buffers go back to the process's cache: nothing may still work on them)
    DeviceIdleScope idle;
    delete b;
}

} // namespace

extern "C" {

int covest_batch_create(covest_model *m, int64_t n_hist, const double *counts, const double *tails, covest_batch **out)
{
    if (!m || !out)
        return refuse("covest_batch_create", "null argument");
    *out = nullptr;
    if (const char *bad = batch_check_create(m->n_keys, n_hist, counts, tails))
        return refuse("covest_batch_create", bad);
    covest_batch *b = nullptr;
    COVEST_TRY(new_batch(m, n_hist, &b));
    BatchCall call(b);
    int rc = call.status;
    if (rc == COVEST_OK)
        rc = batch_prepare(b);
    if (rc == COVEST_OK && n_hist > 0) {
        const size_t cells = (size_t)n_hist * (size_t)b->n_keys;
        const std::vector<double> zeros(tails ? 0 : (size_t)n_hist, 0.0);
        auto fill = [&]() -> int {
            HIP_TRY(b->counts.reserve(cells * sizeof(double)));
            HIP_TRY(b->tails.reserve((size_t)n_hist * sizeof(double)));
            COVEST_TRY(stage_upload(b->counts.ptr, counts, cells * sizeof(double), "covest_batch_create: upload of the counts"));
            return stage_upload(b->tails.ptr, tails ? tails : zeros.data(), (size_t)n_hist * sizeof(double),
                                "covest_batch_create: upload of the tails");
        };
        rc = fill();
    }
    if (rc != COVEST_OK) {
        drop_batch(b);
        return rc;
    }
    *out = b;
    return COVEST_OK;
}

int covest_batch_draw(covest_model *m, const double *params, int64_t n_draws, int64_t first_rep, int64_t n_hist,
                      uint64_t seed, covest_batch **out)
{
    if (!m || !out || !params)
        return refuse("covest_batch_draw", "null argument");
    *out = nullptr;
    if (m->n_keys < 1)
        return refuse("covest_batch_draw", "the model has no keys");
    const bool has_tail = !m->tail_is_zero;
    const int64_t cells = m->n_keys + (has_tail ? 1 : 0);
    if (const char *bad = draw_check_call(cells, n_draws, first_rep, n_hist))
        return refuse("covest_batch_draw", bad);
    if (n_hist > kBatchMaxHist)
        return refuse("covest_batch_draw", "more than 2^20 histograms");
    covest_batch *b = nullptr;
    COVEST_TRY(new_batch(m, n_hist, &b));
    BatchCall call(b);
    auto fill = [&]() -> int {
        COVEST_TRY(call.status);
        COVEST_TRY(batch_prepare(b));
        if (n_hist == 0)
            return COVEST_OK;
        // p_j at every key at the point after clamp_point: one row of the table, left as p
        PointSource src;
        COVEST_TRY(upload_points(b, 1, params, src));
        COVEST_TRY(reserve_chunk(b, 1));
        HIP_TRY(launch_batch_table(table_model(b), src, 1, b->table.as<double>(), b->tl.as<double>(), b->dead.as<int32_t>(),
                                   true, nullptr));
        std::vector<double> p((size_t)b->n_keys), w((size_t)cells);
        HIP_TRY(hipMemcpy(p.data(), b->table.ptr, p.size() * sizeof(double), hipMemcpyDeviceToHost));
        batch_draw_weights(b->n_keys, p.data(), has_tail, w.data());
        if (const char *bad = draw_check_weights(cells, w.data()))
            return refuse("covest_batch_draw", bad);
        DevBuf d_thr, d_rows;
        COVEST_TRY(draw_histograms_resident("covest_batch_draw", cells, w.data(), n_draws, first_rep, n_hist, seed, d_thr,
                                            d_rows));
        HIP_TRY(b->counts.reserve((size_t)n_hist * (size_t)b->n_keys * sizeof(double)));
        HIP_TRY(b->tails.reserve((size_t)n_hist * sizeof(double)));
        HIP_TRY(launch_batch_from_draw(d_rows.as<int64_t>(), n_hist, b->n_keys, has_tail, b->counts.as<double>(),
                                       b->tails.as<double>(), nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr)); // (d_thr and d_rows go with this scope)
        return COVEST_OK;
    };
    const int rc = fill();
    if (rc != COVEST_OK) {
        drop_batch(b);
        return rc;
    }
    *out = b;
    return COVEST_OK;
}

int covest_batch_counts(covest_batch *b, double *out_counts, double *out_tails)
{
    if (!b)
        return refuse("covest_batch_counts", "null batch");
    if (b->n_hist == 0)
        return COVEST_OK;
    if (!out_counts || !out_tails)
        return refuse("covest_batch_counts", "null buffer");
    BatchCall call(b, false);
    COVEST_TRY(call.status);
    HIP_TRY(hipMemcpy(out_counts, b->counts.ptr, (size_t)b->n_hist * (size_t)b->n_keys * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_tails, b->tails.ptr, (size_t)b->n_hist * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_batch_eval_cross(covest_batch *b, int64_t n, const double *params, double *out_ll)
{
    if (!b)
        return refuse("covest_batch_eval_cross", "null batch");
    if (const char *bad = batch_check_points(n, b->n_hist, params, out_ll))
        return refuse("covest_batch_eval_cross", bad);
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (n == 0 || b->n_hist == 0)
        return COVEST_OK;
    return cross_chunks(b, n, params, [&](int64_t first, int64_t nc) -> int {
        HIP_TRY(hipMemcpy2D(out_ll + first, (size_t)n * sizeof(double), b->out.ptr, (size_t)nc * sizeof(double),
                            (size_t)nc * sizeof(double), (size_t)b->n_hist, hipMemcpyDeviceToHost));
        return COVEST_OK;
    });
}

int covest_batch_argmin_cross(covest_batch *b, int64_t n, const double *params, double *out_min_negll, int64_t *out_arg)
{
    if (!b)
        return refuse("covest_batch_argmin_cross", "null batch");
    if (n < 0)
        return refuse("covest_batch_argmin_cross", "n must not be negative");
    if (b->n_hist > 0 && n > 0 && (!out_min_negll || !out_arg || !params))
        return refuse("covest_batch_argmin_cross", "null buffer");
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (b->n_hist == 0 || n == 0)
        return COVEST_OK;
    HIP_TRY(b->run_val.reserve((size_t)b->n_hist * sizeof(double)));
    HIP_TRY(b->run_idx.reserve((size_t)b->n_hist * sizeof(int64_t)));
    HIP_TRY(launch_batch_argmin_init(b->n_hist, b->run_val.as<double>(), b->run_idx.as<int64_t>(), nullptr));
    COVEST_TRY(cross_chunks(b, n, params, [&](int64_t first, int64_t nc) -> int {
        HIP_TRY(launch_batch_argmin(b->out.as<double>(), nc, b->n_hist, nc, first, b->run_val.as<double>(),
                                    b->run_idx.as<int64_t>(), nullptr));
        return COVEST_OK;
    }));
    HIP_TRY(hipMemcpy(out_min_negll, b->run_val.ptr, (size_t)b->n_hist * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_arg, b->run_idx.ptr, (size_t)b->n_hist * sizeof(int64_t), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_batch_eval_pairs(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out_ll)
{
    if (!b)
        return refuse("covest_batch_eval_pairs", "null batch");
    if (n < 0)
        return refuse("covest_batch_eval_pairs", "n must not be negative");
    if (n > 0 && (!params || !out_ll))
        return refuse("covest_batch_eval_pairs", "null buffer");
    if (const char *bad = batch_check_index(n, hist_index, b->n_hist))
        return refuse("covest_batch_eval_pairs", bad);
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (n == 0)
        return COVEST_OK;
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    HIP_TRY(b->index.reserve((size_t)n * sizeof(int64_t)));
    COVEST_TRY(stage_upload(b->index.ptr, hist_index, (size_t)n * sizeof(int64_t), "covest_batch_eval_pairs: upload of the index"));
    const int64_t per = batch_points_per_chunk(b->n_keys, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_chunk(b, nc_max));
    HIP_TRY(b->out.reserve((size_t)nc_max * sizeof(double)));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(table_chunk(b, src, first, nc, &n_dead));
        HIP_TRY(launch_batch_pairs(b->counts.as<double>(), b->tails.as<double>(), b->index.as<int64_t>() + first,
                                   b->table.as<double>(), b->tl.as<double>(), nc, b->n_keys, b->out.as<double>(), nullptr));
        HIP_TRY(hipMemcpy(out_ll + first, b->out.ptr, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost));
        add_elapsed(b, 6, b->ev[0], b->ev[1]);
        b->info[5] += nc;
    }
    return COVEST_OK;
}

int covest_batch_eval_cross_grad(covest_batch *b, int64_t n, const double *params, double *out)
{
    if (!b)
        return refuse("covest_batch_eval_cross_grad", "null batch");
    if (const char *bad = batch_check_points(n, b->n_hist, params, out))
        return refuse("covest_batch_eval_cross_grad", bad);
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (n == 0 || b->n_hist == 0)
        return COVEST_OK;
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    const int64_t R = rows_per_point(b);
    const int64_t per = batch_grad_points_per_chunk(b->n_keys, R, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_grad_chunk(b, nc_max));
    HIP_TRY(b->out.reserve((size_t)b->n_hist * (size_t)nc_max * (size_t)R * sizeof(double)));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0, tiles = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(grad_table_chunk(b, src, first, nc, &n_dead));
        const int64_t ld = nc * R; // the contraction sees R nc rows of the table and as many tail coefficients
        HIP_TRY(hipEventRecord(b->ev[2], nullptr));
        HIP_TRY(launch_batch_cross(b->counts.as<double>(), b->tails.as<double>(), b->n_hist, b->table.as<double>(),
                                   b->tl.as<double>(), ld, b->n_keys, b->out.as<double>(), ld, &tiles, nullptr));
        b->info[2] += tiles;
        if (n_dead > 0) {
            HIP_TRY(launch_batch_fix_dead(b->counts.as<double>(), b->n_hist, b->table.as<double>(), b->n_keys,
                                          b->dead_list.as<int32_t>(), n_dead, b->out.as<double>(), ld, nullptr));
            b->info[4] += b->n_hist * n_dead;
        }
        HIP_TRY(launch_batch_grad_specials(b->n_hist, nc, (int)R, b->out.as<double>(), ld, nullptr));
        HIP_TRY(hipEventRecord(b->ev[3], nullptr));
        HIP_TRY(hipMemcpy2D(out + first * R, (size_t)n * (size_t)R * sizeof(double), b->out.ptr, (size_t)ld * sizeof(double),
                            (size_t)ld * sizeof(double), (size_t)b->n_hist, hipMemcpyDeviceToHost));
        HIP_TRY(hipEventSynchronize(b->ev[3]));
        add_elapsed(b, 6, b->ev[0], b->ev[1]);
        add_elapsed(b, 7, b->ev[2], b->ev[3]);
    }
    return COVEST_OK;
}

int covest_batch_eval_pairs_grad(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out)
{
    if (!b)
        return refuse("covest_batch_eval_pairs_grad", "null batch");
    if (n < 0)
        return refuse("covest_batch_eval_pairs_grad", "n must not be negative");
    if (n > 0 && (!params || !out))
        return refuse("covest_batch_eval_pairs_grad", "null buffer");
    if (const char *bad = batch_check_index(n, hist_index, b->n_hist))
        return refuse("covest_batch_eval_pairs_grad", bad);
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (n == 0)
        return COVEST_OK;
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    HIP_TRY(b->index.reserve((size_t)n * sizeof(int64_t)));
    COVEST_TRY(stage_upload(b->index.ptr, hist_index, (size_t)n * sizeof(int64_t),
                            "covest_batch_eval_pairs_grad: upload of the index"));
    const int64_t R = rows_per_point(b);
    const int64_t per = batch_grad_points_per_chunk(b->n_keys, R, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_grad_chunk(b, nc_max));
    HIP_TRY(b->out.reserve((size_t)nc_max * (size_t)R * sizeof(double)));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(grad_table_chunk(b, src, first, nc, &n_dead));
        HIP_TRY(hipEventRecord(b->ev[2], nullptr));
        HIP_TRY(launch_batch_pairs_grad(b->counts.as<double>(), b->tails.as<double>(), b->index.as<int64_t>() + first,
                                        b->table.as<double>(), b->tl.as<double>(), nc, b->n_keys, (int)R, b->out.as<double>(),
                                        nullptr));
        HIP_TRY(hipEventRecord(b->ev[3], nullptr));
        HIP_TRY(hipMemcpy(out + first * R, b->out.ptr, (size_t)nc * (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipEventSynchronize(b->ev[3]));
        add_elapsed(b, 6, b->ev[0], b->ev[1]);
        add_elapsed(b, 7, b->ev[2], b->ev[3]);
        b->info[5] += nc;
    }
    return COVEST_OK;
}

int covest_batch_score_table(covest_batch *b, int64_t n, const double *params, double *out_rows, double *out_tail)
{
    if (!b)
        return refuse("covest_batch_score_table", "null batch");
    if (const char *bad = batch_check_points(n, 1, params, out_rows)) // (the table does not depend on the histograms)
        return refuse("covest_batch_score_table", bad);
    if (n > 0 && !out_tail)
        return refuse("covest_batch_score_table", "null buffer");
    BatchCall call(b);
    COVEST_TRY(call.status);
    if (n == 0)
        return COVEST_OK;
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    const int64_t R = rows_per_point(b);
    const int64_t per = batch_grad_points_per_chunk(b->n_keys, R, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_grad_chunk(b, nc_max));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(grad_table_chunk(b, src, first, nc, &n_dead));
        HIP_TRY(hipMemcpy(out_rows + first * R * b->n_keys, b->table.ptr,
                          (size_t)nc * (size_t)R * (size_t)b->n_keys * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_tail + first * R, b->tl.ptr, (size_t)nc * (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
        add_elapsed(b, 6, b->ev[0], b->ev[1]);
    }
    return COVEST_OK;
}

int covest_batch_info(covest_batch *b, int64_t *out)
{
    if (!b || !out)
        return refuse("covest_batch_info", "null argument");
    std::lock_guard<std::mutex> hold(b->model->lock);
    std::copy(b->info, b->info + 8, out);
    return COVEST_OK;
}

void covest_batch_destroy(covest_batch *b)
{
    if (!b)
        return;
    std::lock_guard<std::mutex> hold(b->model->lock);
    DeviceGuard dev_guard(b->model->device);
    drop_batch(b);
}

} // extern "C"
