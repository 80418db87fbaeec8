// abi_batch.cpp -- covest_batch_* of the C ABI over ll_batch.hip: a batch of histograms on one model's key set, scored
// in one pass (DESIGN.md sections 6r, 6u, 6x and, for the staging of this file, 6w).  The argument rules, the chunking of a
// point list against the table budget and the cut of launches are batch_host.h's (plain C++, checked without a device).
// A batch borrows its model; every call takes the model's lock and works on the model's device.
//
// An evaluation is open_call (the rules, the lock, fresh counters), then walk_chunks: the point list goes up once, and
// per chunk table_chunk builds the table of R rows a point (R = 1: log p; R = P + 1: with the scores; R = 1 + P +
// P (P + 1) / 2: with the curvature rows behind them), a STAGE contracts
// it with the histograms into b->out (cross_stage, pairs_stage; the score table has none) and the entry point's own
// few lines deliver the chunk.
#include "host.h"

#include <type_traits>

#include "batch_host.h"
#include "draw_host.h"

using namespace covest;

static_assert(kBatchHostTableBytes == kBatchTableBytes && kBatchHostMaxHist == kBatchMaxHist, "one budget, one cap");

// covest_batch_info's fields, in the order of batch.py INFO_FIELDS
enum BatchInfo { kPointsTabled, kTableChunks, kCrossTiles, kDeadPoints, kFixupWaves, kPairsRequests, kTableNs, kContractionNs, kInfoFields };
static_assert(kInfoFields == 8, "covest_batch_info writes out[8] (include/covest_amd.h)");

struct covest_batch {
    covest_model *model = nullptr;
    int64_t n_hist = 0, n_keys = 0;
    DevBuf counts, tails;    // H[n_hist][n_keys], tails[n_hist]
    DevBuf zero_cnt;         // the count array of the table's DevModel: n_keys zeros
    DevBuf table, tl, dead;  // one chunk: R rows [n_keys] a point, its R tail coefficients, keys with p <= 0 per point
    DevBuf points;           // a call's parameters, behind them its thresholds (repeats model)
    DevBuf out;              // a chunk's values: [n_hist][points of the chunk][R] (cross), [points][R] (pairs)
    DevBuf index, dead_list; // a pairs call's histogram numbers; the value rows of the chunk's points with dead keys
    DevBuf run_val, run_idx; // the running arg-min of covest_batch_argmin_cross
    DevBuf partial, fin;     // the gradient's and the Hessian's table: the derivative kernel's segment sums; its finishing
                             // pass's value [points], gradient [points][P] and (order 2) Hessian [points][P][P] (the tail
                             // coefficients before they are packed into tl)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // ev[0] .. ev[1]: a chunk's table; ev[2] .. ev[3]: its stage
    int64_t info[kInfoFields] = {};
    ~covest_batch()
    {
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
    }
};

namespace {

int refuse(const char *who, const char *what) { return fail(COVEST_E_INVALID, std::string(who) + ": " + what); }

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
    const int P = b->model->n_par;
    const size_t par_bytes = (size_t)n * P * sizeof(double);
    const std::vector<int32_t> t = point_thresholds(b->model, n, params);
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

// Rows a point of the table for derivatives up to `order` (0, 1, 2): batch_host.h's
int rows_per_point(const covest_batch *b, int order) { return batch_rows_per_point(b->model->n_par, order); }

// room for a chunk of nc_max points at R rows each
int reserve_chunk(covest_batch *b, int64_t nc_max, int R)
{
    if (nc_max * R > std::numeric_limits<int32_t>::max())
        return fail(COVEST_E_UNSUPPORTED, R == 1 ? "covest_batch: more than 2^31 points in a table chunk"
                                                 : "covest_batch: more than 2^31 rows in a table chunk");
    HIP_TRY(b->table.reserve((size_t)nc_max * (size_t)R * (size_t)b->n_keys * sizeof(double)));
    HIP_TRY(b->tl.reserve((size_t)nc_max * (size_t)R * sizeof(double)));
    HIP_TRY(b->dead.reserve((size_t)nc_max * sizeof(int32_t)));
    if (R > 1) { // the derivative kernel's buffers, by DerivLayout<P, order>; fin: value, gradient and (order 2) P x P
        const int P = b->model->n_par, order = batch_table_order(P, R);
        HIP_TRY(b->partial.reserve(ll_deriv_partial_bytes(table_model(b), order, nc_max)));
        HIP_TRY(b->fin.reserve((size_t)nc_max * (size_t)(1 + P + (order == 2 ? P * P : 0)) * sizeof(double)));
    }
    return COVEST_OK;
}

// The table of one chunk (points first .. first + nc of the list): rows R i .. of b->table are point i's, b->tl holds its
// R tail coefficients.  Its points with dead keys are counted in *n_dead and their VALUE rows R i listed on the device
// (dead_list: what launch_batch_fix_dead indexes by).  ev[0] .. ev[1] bracket the kernels.
int table_chunk(covest_batch *b, const PointSource &src, int64_t first, int64_t nc, int R, int64_t *n_dead)
{
    const PointSource part = points_from(src, first, b->model->n_par);
    HIP_TRY(hipEventRecord(b->ev[0], nullptr));
    if (R == 1) {
        HIP_TRY(launch_batch_table(table_model(b), part, nc, b->table.as<double>(), b->tl.as<double>(),
                                   b->dead.as<int32_t>(), false, nullptr));
    } else {
        const int P = b->model->n_par, order = batch_table_order(P, R);
        double *fin_ll = b->fin.as<double>(), *fin_grad = fin_ll + nc, *fin_hess = order == 2 ? fin_grad + nc * P : nullptr;
        HIP_TRY(launch_ll_deriv_table(table_model(b), order, part, nc, b->partial.as<double>(), b->table.as<double>(),
                                      b->dead.as<int32_t>(), fin_ll, fin_grad, fin_hess, nullptr));
        HIP_TRY(launch_batch_tail_pack(fin_ll, fin_grad, fin_hess, nc, P, R, b->tl.as<double>(), nullptr));
    }
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
    b->info[kPointsTabled] += nc;
    b->info[kTableChunks] += 1;
    b->info[kDeadPoints] += *n_dead;
    return COVEST_OK;
}

void add_elapsed(covest_batch *b, BatchInfo field, hipEvent_t from, hipEvent_t to)
{
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, from, to) == hipSuccess)
        b->info[field] += (int64_t)((double)ms * 1e6);
    else
        (void)hipGetLastError();
}

// The walk every evaluation makes over its point list, chunk by chunk of the table of R rows a point:
// `stage(first, nc, n_dead)` contracts a chunk's table into b->out, which has room for out_per_row doubles a table row,
// between ev[2] and ev[3] (nullptr: the call contracts nothing); `deliver(first, nc)` takes the chunk's result.  Called
// with the model locked and its device current.
template <class Stage, class Deliver>
int walk_chunks(covest_batch *b, int64_t n, const double *params, int R, int64_t out_per_row, Stage stage, Deliver deliver)
{
    constexpr bool contracts = !std::is_null_pointer<Stage>::value;
    PointSource src;
    COVEST_TRY(upload_points(b, n, params, src));
    const int64_t per = batch_points_per_chunk(b->n_keys, R, kBatchTableBytes), nc_max = std::min(n, per);
    COVEST_TRY(reserve_chunk(b, nc_max, R));
    HIP_TRY(b->out.reserve((size_t)out_per_row * (size_t)nc_max * (size_t)R * sizeof(double)));
    const int64_t chunks = batch_chunk_count(n, per);
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, nc, n_dead = 0;
        batch_chunk(n, per, c, &first, &nc);
        COVEST_TRY(table_chunk(b, src, first, nc, R, &n_dead));
        if constexpr (contracts) {
            HIP_TRY(hipEventRecord(b->ev[2], nullptr));
            COVEST_TRY(stage(first, nc, n_dead));
            HIP_TRY(hipEventRecord(b->ev[3], nullptr));
        }
        COVEST_TRY(deliver(first, nc));
        add_elapsed(b, kTableNs, b->ev[0], b->ev[1]); // (table_chunk's read-back of `dead` has waited for ev[1])
        if constexpr (contracts) {
            HIP_TRY(hipEventSynchronize(b->ev[3])); // (the events are the next chunk's too)
            add_elapsed(b, kContractionNs, b->ev[2], b->ev[3]);
        }
    }
    return COVEST_OK;
}

// The cross stage: every histogram against the chunk's nc R table rows, b->out[h][i R + q] with row length nc R; -inf
// where a histogram counts a dead key of a point; behind a value that is not finite, NaN derivatives.
int cross_stage(covest_batch *b, int64_t nc, int R, int64_t n_dead)
{
    const int64_t ld = nc * R; // the contraction sees R nc rows of the table and as many tail coefficients
    int64_t tiles = 0;
    HIP_TRY(launch_batch_cross(b->counts.as<double>(), b->tails.as<double>(), b->n_hist, b->table.as<double>(),
                               b->tl.as<double>(), ld, b->n_keys, b->out.as<double>(), ld, &tiles, nullptr));
    b->info[kCrossTiles] += tiles;
    if (n_dead > 0) {
        HIP_TRY(launch_batch_fix_dead(b->counts.as<double>(), b->n_hist, b->table.as<double>(), b->n_keys,
                                      b->dead_list.as<int32_t>(), n_dead, b->out.as<double>(), ld, nullptr));
        b->info[kFixupWaves] += b->n_hist * n_dead;
    }
    if (R > 1)
        HIP_TRY(launch_batch_grad_specials(b->n_hist, nc, R, b->out.as<double>(), ld, nullptr));
    return COVEST_OK;
}

// The pairs stage: histogram index[first + i] against point i of the chunk, b->out[i R + q]
int pairs_stage(covest_batch *b, int64_t first, int64_t nc, int R)
{
    HIP_TRY(launch_batch_pairs(b->counts.as<double>(), b->tails.as<double>(), b->index.as<int64_t>() + first,
                               b->table.as<double>(), b->tl.as<double>(), nc, b->n_keys, R, b->out.as<double>(), nullptr));
    b->info[kPairsRequests] += nc;
    return COVEST_OK;
}

struct BatchCall { // the model's lock, its device, fresh counters
    std::unique_lock<std::mutex> hold;
    std::optional<DeviceGuard> guard;
    int status = COVEST_OK;
    explicit BatchCall(covest_batch *b, bool counters = true) : hold(b->model->lock)
    {
        status = guard.emplace(b->model->device).status();
        if (counters)
            std::fill(b->info, b->info + kInfoFields, (int64_t)0);
    }
};

// The opening of an evaluation: a batch there is, arguments that batch_host.h's `rule` accepts, then the BatchCall.
template <class Rule>
int open_call(const char *who, covest_batch *b, Rule rule, std::optional<BatchCall> &call)
{
    if (!b)
        return refuse(who, "null batch");
    if (const char *bad = rule())
        return refuse(who, bad);
    return call.emplace(b).status;
}

// covest_batch_eval_cross, _cross_grad and _cross_hess (order 0, 1, 2): out[h][i][R] of the whole list, chunk by chunk
int eval_cross(const char *who, covest_batch *b, int64_t n, const double *params, int order, double *out)
{
    std::optional<BatchCall> call;
    COVEST_TRY(open_call(who, b, [&] { return batch_check_points(n, b->n_hist, params, out); }, call));
    if (n == 0 || b->n_hist == 0)
        return COVEST_OK;
    const int R = rows_per_point(b, order);
    return walk_chunks(
        b, n, params, R, b->n_hist, [&](int64_t, int64_t nc, int64_t n_dead) { return cross_stage(b, nc, R, n_dead); },
        [&](int64_t first, int64_t nc) -> int {
            const size_t row = (size_t)nc * (size_t)R * sizeof(double);
            HIP_TRY(hipMemcpy2D(out + first * R, (size_t)n * (size_t)R * sizeof(double), b->out.ptr, row, row,
                                (size_t)b->n_hist, hipMemcpyDeviceToHost));
            return COVEST_OK;
        });
}

// covest_batch_eval_pairs, _pairs_grad and _pairs_hess (order 0, 1, 2): out[i][R]
int eval_pairs(const char *who, covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, int order,
               double *out)
{
    std::optional<BatchCall> call;
    COVEST_TRY(open_call(who, b, [&] { return batch_check_pairs(n, b->n_hist, hist_index, params, out); }, call));
    if (n == 0)
        return COVEST_OK;
    HIP_TRY(b->index.reserve((size_t)n * sizeof(int64_t)));
    COVEST_TRY(stage_upload(b->index.ptr, hist_index, (size_t)n * sizeof(int64_t),
                            (std::string(who) + ": upload of the index").c_str()));
    const int R = rows_per_point(b, order);
    return walk_chunks(
        b, n, params, R, 1, [&](int64_t first, int64_t nc, int64_t) { return pairs_stage(b, first, nc, R); },
        [&](int64_t first, int64_t nc) -> int {
            HIP_TRY(hipMemcpy(out + first * R, b->out.ptr, (size_t)nc * (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
            return COVEST_OK;
        });
}

// covest_batch_score_table and _score_table2 (order 1, 2): the stage-less walk, the chunk's table and tail coefficients
// handed back as they are
int score_table(const char *who, covest_batch *b, int64_t n, const double *params, int order, double *out_rows,
                double *out_tail)
{
    std::optional<BatchCall> call; // (the table does not depend on the histograms: the rule of a batch of one)
    COVEST_TRY(open_call(who, b, [&] { return batch_check_points(n, 1, params, out_rows, out_tail); }, call));
    if (n == 0)
        return COVEST_OK;
    const int R = rows_per_point(b, order);
    return walk_chunks(b, n, params, R, 0, nullptr, [&](int64_t first, int64_t nc) -> int {
        HIP_TRY(hipMemcpy(out_rows + first * R * b->n_keys, b->table.ptr,
                          (size_t)nc * (size_t)R * (size_t)b->n_keys * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_tail + first * R, b->tl.ptr, (size_t)nc * (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
        return COVEST_OK;
    });
}

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

// how covest_batch_create and _draw end: the filled batch handed over, or dropped with the status of what failed
int hand_over(covest_batch *b, int rc, covest_batch **out)
{
    if (rc != COVEST_OK) {
        drop_batch(b);
        return rc;
    }
    *out = b;
    return COVEST_OK;
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
    auto fill = [&]() -> int {
        COVEST_TRY(call.status);
        COVEST_TRY(batch_prepare(b));
        if (n_hist == 0)
            return COVEST_OK;
        const size_t cells = (size_t)n_hist * (size_t)b->n_keys;
        const std::vector<double> zeros(tails ? 0 : (size_t)n_hist, 0.0);
        HIP_TRY(b->counts.reserve(cells * sizeof(double)));
        HIP_TRY(b->tails.reserve((size_t)n_hist * sizeof(double)));
        COVEST_TRY(stage_upload(b->counts.ptr, counts, cells * sizeof(double), "covest_batch_create: upload of the counts"));
        return stage_upload(b->tails.ptr, tails ? tails : zeros.data(), (size_t)n_hist * sizeof(double),
                            "covest_batch_create: upload of the tails");
    };
    return hand_over(b, fill(), out);
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
        COVEST_TRY(reserve_chunk(b, 1, 1));
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
    return hand_over(b, fill(), out);
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
    return eval_cross("covest_batch_eval_cross", b, n, params, 0, out_ll);
}

int covest_batch_eval_cross_grad(covest_batch *b, int64_t n, const double *params, double *out)
{
    return eval_cross("covest_batch_eval_cross_grad", b, n, params, 1, out);
}

int covest_batch_eval_cross_hess(covest_batch *b, int64_t n, const double *params, double *out)
{
    return eval_cross("covest_batch_eval_cross_hess", b, n, params, 2, out);
}

int covest_batch_eval_pairs(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out_ll)
{
    return eval_pairs("covest_batch_eval_pairs", b, n, hist_index, params, 0, out_ll);
}

int covest_batch_eval_pairs_grad(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out)
{
    return eval_pairs("covest_batch_eval_pairs_grad", b, n, hist_index, params, 1, out);
}

int covest_batch_eval_pairs_hess(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out)
{
    return eval_pairs("covest_batch_eval_pairs_hess", b, n, hist_index, params, 2, out);
}

int covest_batch_argmin_cross(covest_batch *b, int64_t n, const double *params, double *out_min_negll, int64_t *out_arg)
{
    std::optional<BatchCall> call;
    COVEST_TRY(open_call("covest_batch_argmin_cross", b,
                         [&] { return batch_check_points(n, b->n_hist, params, out_min_negll, out_arg); }, call));
    if (b->n_hist == 0 || n == 0)
        return COVEST_OK;
    HIP_TRY(b->run_val.reserve((size_t)b->n_hist * sizeof(double)));
    HIP_TRY(b->run_idx.reserve((size_t)b->n_hist * sizeof(int64_t)));
    HIP_TRY(launch_batch_argmin_init(b->n_hist, b->run_val.as<double>(), b->run_idx.as<int64_t>(), nullptr));
    COVEST_TRY(walk_chunks(
        b, n, params, 1, b->n_hist, [&](int64_t, int64_t nc, int64_t n_dead) { return cross_stage(b, nc, 1, n_dead); },
        [&](int64_t first, int64_t nc) -> int {
            HIP_TRY(launch_batch_argmin(b->out.as<double>(), nc, b->n_hist, nc, first, b->run_val.as<double>(),
                                        b->run_idx.as<int64_t>(), nullptr));
            return COVEST_OK;
        }));
    HIP_TRY(hipMemcpy(out_min_negll, b->run_val.ptr, (size_t)b->n_hist * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_arg, b->run_idx.ptr, (size_t)b->n_hist * sizeof(int64_t), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_batch_score_table(covest_batch *b, int64_t n, const double *params, double *out_rows, double *out_tail)
{
    return score_table("covest_batch_score_table", b, n, params, 1, out_rows, out_tail);
}

int covest_batch_score_table2(covest_batch *b, int64_t n, const double *params, double *out_rows, double *out_tail)
{
    return score_table("covest_batch_score_table2", b, n, params, 2, out_rows, out_tail);
}

int covest_batch_info(covest_batch *b, int64_t *out)
{
    if (!b || !out)
        return refuse("covest_batch_info", "null argument");
    std::lock_guard<std::mutex> hold(b->model->lock);
    std::copy(b->info, b->info + kInfoFields, out);
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
