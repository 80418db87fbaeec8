// abi_grid.cpp -- the grid handle of the C ABI (include/covest_amd.h): covest_grid_*.
#include "host.h"

using namespace covest;

namespace covest {

// Where a grid handle stages an upload, and how the copy is issued (host.h covest_grid::stage).
int grid_stage_begin(covest_grid *g, size_t bytes, StageSlot &slot)
{
    if (!g->async_uploads) { // covest_grid_create: the process's staging buffer, a blocking copy
        SharedStage &ss = shared_stage();
        slot.shared_hold = std::unique_lock<std::mutex>(ss.mu);
        HIP_TRY(ss.buf.reserve(bytes));
        slot.ptr = ss.buf.as<char>();
        return COVEST_OK;
    }
    const size_t at = (g->stage_off + 63) / 64 * 64;
    if (at + bytes > g->stage.cap) {
        // (the block is outgrown: what it holds may still be read -- copies in flight, a small grid's axes read in
        // place -- so it is set aside until the next reset, and a larger one takes over)
        if (g->stage.ptr)
            g->stage_retired.push_back(std::move(g->stage));
        HIP_TRY(g->stage.reserve(std::max<size_t>(2 * (at + bytes), 1 << 18)));
        slot.ptr = g->stage.as<char>();
        g->stage_off = bytes;
        return COVEST_OK;
    }
    slot.ptr = g->stage.as<char>() + at;
    g->stage_off = at + bytes;
    return COVEST_OK;
}

int grid_stage_commit(covest_grid *g, StageSlot &slot, void *dst, size_t bytes)
{
    if (!g->async_uploads) {
        HIP_TRY(hipMemcpy(dst, slot.ptr, bytes, hipMemcpyHostToDevice));
        slot.shared_hold = std::unique_lock<std::mutex>();
        return COVEST_OK;
    }
    HIP_TRY(hipMemcpyAsync(dst, slot.ptr, bytes, hipMemcpyHostToDevice, nullptr));
    g->upload_pending = true;
    return COVEST_OK;
}

} // namespace covest

namespace {

// The arguments of covest_grid_create / covest_grid_reset: the grid's size, the axes' values together, and the block's
// end (a negative flat_end means the whole grid).
int check_grid_args(const covest_model *m, int32_t n_axes, const double *const *axes, const int64_t *axis_len, int64_t flat_begin,
                    int64_t *flat_end, const char *who, int64_t *total_out, int64_t *n_values_out)
{
    if (!axes || !axis_len)
        return fail(COVEST_E_INVALID, std::string(who) + ": null argument");
    if (n_axes != m->n_par)
        return fail(COVEST_E_INVALID, std::string(who) + ": n_axes must equal the model's param_count");
    int64_t total = 1, n_values = 0;
    for (int d = 0; d < n_axes; ++d) {
        if (axis_len[d] < 1 || !axes[d])
            return fail(COVEST_E_INVALID, std::string(who) + ": every axis needs at least one value");
        if (total > (int64_t)1 << 40)
            return fail(COVEST_E_INVALID, std::string(who) + ": grid too large");
        total *= axis_len[d];
        n_values += axis_len[d];
    }
    if (*flat_end < 0)
        *flat_end = total;
    if (flat_begin < 0 || flat_begin > *flat_end || *flat_end > total)
        return fail(COVEST_E_INVALID, std::string(who) + ": bad flat index range");
    *total_out = total;
    *n_values_out = n_values;
    return COVEST_OK;
}

// The arena of a grid of n points whose axes hold n_values doubles and whose threshold table holds nq entries, as byte
// offsets: [queue counter (8 B, always at the start: its place does not move from grid to grid) | axes | t_table],
// staged and uploaded together, then the outputs.
struct GridArena {
    size_t ctl, axes, table;
    size_t staged_bytes; // the three above
    size_t ll, idx, word, partial_val, partial_idx, result, bytes;
    GridArena(int64_t n_values, int64_t nq, int64_t n)
    {
        const size_t n_pts = (size_t)(n > 0 ? n : 1);
        ctl = 0;
        axes = 8;
        table = axes + (size_t)n_values * sizeof(double);
        staged_bytes = (table + (size_t)nq * sizeof(int32_t) + 7) / 8 * 8;
        ll = staged_bytes;
        idx = ll + n_pts * sizeof(double);
        word = idx + n_pts * sizeof(int64_t);
        partial_val = word + n_pts * sizeof(unsigned long long);
        partial_idx = partial_val + kArgminBlocks * sizeof(double);
        result = partial_idx + kArgminBlocks * sizeof(int64_t);
        bytes = result + sizeof(ArgminResult);
    }
};

// Grows the arena, stages [counter | axes | table] and sends them on their way.  *inputs: where the kernels read the
// axes and the table -- the arena, or the staging memory itself:
// A SMALL grid of a handle that is re-configured (optimize_grid's: a few thousand points, a kilobyte of axes and
// threshold_o) reads its axes and the table WHERE THEY ARE STAGED -- page-locked host memory mapped into the
// device's address space: every workgroup reads a handful of values, and the copy engine's start-up (11 us by
// the trace of a search, a sixth of an iteration) is not paid.  The queue counter behind the axes is device
// memory all the same (atomics): cleared by a memset on the stream.  Large grids -- every point of 10^6 reads
// its axes -- keep the copy.
int stage_inputs(covest_grid *g, const GridArena &a, int32_t n_axes, const double *const *axes, const int64_t *axis_len,
                 const std::vector<int32_t> &table, int64_t n, char **inputs)
{
    const void *arena_before = g->arena.ptr;
    const bool counter_clean = g->counter_clean; // (the queue counter is 0: set by grid_configure; an evaluation clears the
                                                 // mark and sets it again once its arg-min, which resets the counter, is launched)
    HIP_TRY(g->arena.reserve(a.bytes));
    char *base = g->arena.as<char>();
    StageSlot slot;
    const int src = grid_stage_begin(g, a.staged_bytes, slot);
    if (src != COVEST_OK)
        return src;
    char *stage = slot.ptr;
    std::memset(stage, 0, a.staged_bytes);
    double *sa = reinterpret_cast<double *>(stage + a.axes);
    for (int d = 0; d < n_axes; ++d) {
        std::copy(axes[d], axes[d] + axis_len[d], sa);
        sa += axis_len[d];
    }
    if (!table.empty())
        std::memcpy(stage + a.table, table.data(), table.size() * sizeof(int32_t));
    if (g->async_uploads && n <= kArgminSmall) { // in place
        *inputs = stage;
        // (the counter's place depends on the axes' lengths: cleared unless it is where a clean one was left)
        if (!(counter_clean && g->arena.ptr == arena_before && g->sub_ctl.ptr == base + a.ctl)) {
            HIP_TRY(hipMemsetAsync(base + a.ctl, 0, 8, nullptr));
            g->upload_pending = true;
        }
        return COVEST_OK;
    }
    *inputs = base;
    return grid_stage_commit(g, slot, base, a.staged_bytes);
}

// The handle's views into the arena (axes and table: into `inputs`, see stage_inputs) and its PointSource.
void bind_views(covest_grid *g, const GridArena &a, char *inputs, int32_t n_axes, const int64_t *axis_len, int64_t flat_begin)
{
    char *base = g->arena.as<char>();
    g->axes.ptr = inputs + a.axes;
    g->sub_ctl.ptr = base + a.ctl;
    g->t_table.ptr = inputs + a.table;
    g->ll.ptr = base + a.ll;
    g->sub_index.ptr = base + a.idx;
    g->sub_word.ptr = base + a.word;
    g->partial_val.ptr = base + a.partial_val;
    g->partial_idx.ptr = base + a.partial_idx;
    g->result.ptr = base + a.result;
    PointSource &src = g->src;
    src = PointSource{};
    src.is_grid = 1;
    src.flat_begin = flat_begin;
    int64_t off = 0;
    for (int d = 0; d < kMaxParams; ++d) {
        g->len[d] = src.len[d] = d < n_axes ? axis_len[d] : 1;
        src.axis[d] = d < n_axes ? g->axes.as<double>() + off : nullptr;
        if (d < n_axes)
            off += axis_len[d];
    }
    if (g->model->n_par == 5)
        src.t_table = g->t_table.as<int32_t>();
}

// Sums of (T - 1) of a repeats grid: over the flat indices [flat_begin, flat_end) -- whole (c, e) rows plus two ragged
// ends -- and over the nq weight vectors.
struct TMinus1Sums {
    double block, q;
};

TMinus1Sums sum_t_minus_1(const std::vector<int32_t> &table, int64_t nq, int64_t flat_begin, int64_t flat_end)
{
    std::vector<double> prefix((size_t)nq + 1, 0.0);
    for (int64_t i = 0; i < nq; ++i)
        prefix[(size_t)i + 1] = prefix[(size_t)i] + (double)(table[(size_t)i] > 1 ? table[(size_t)i] - 1 : 0);
    auto upto = [&](int64_t flat) { // sum over flat indices [0, flat)
        return (double)(flat / nq) * prefix[(size_t)nq] + prefix[(size_t)(flat % nq)];
    };
    return {upto(flat_end) - upto(flat_begin), prefix[(size_t)nq]};
}

} // namespace

// Everything a grid handle holds besides its identity: called by covest_grid_create and covest_grid_reset.  Device
// memory is only ever grown, and the small inputs (axes, threshold table, the queue's counter) go up in ONE copy:
// optimize_grid re-configures a handle every iteration (21 times 0.2 ms of allocations and copies otherwise).
static int grid_configure(covest_grid *g, int32_t n_axes, const double *const *axes, const int64_t *axis_len,
                          int64_t flat_begin, int64_t flat_end, const char *who)
{
    covest_model *m = g->model;
    int64_t total = 0, n_values = 0;
    const int arc = check_grid_args(m, n_axes, axes, axis_len, flat_begin, &flat_end, who, &total, &n_values);
    if (arc != COVEST_OK)
        return arc;
    g->configured = false; // (set again at the very end: a failure below leaves views into a freed arena behind)
    g->flat_begin = flat_begin;
    g->flat_end = flat_end;
    g->evaluated = false;
    g->fix_pending = false; // (a strict pass still owed is dropped with the values it was owed for)
    g->scan_valid = false;
    g->ev_used = 0;
    g->stage_off = 0; // (a reset waited for the stream of the last evaluation: what the last reset staged has been copied)
    const int64_t n = flat_end - flat_begin;
    const int64_t n1 = n_axes == 5 ? axis_len[2] : 1, n2 = n_axes == 5 ? axis_len[3] : 1, n3 = n_axes == 5 ? axis_len[4] : 1;
    const int64_t nq = n_axes == 5 ? n1 * n2 * n3 : 0;

    // threshold_o over the (q1, q2, q) sub-grid (host, libm)
    std::vector<int32_t> table((size_t)nq);
    if (nq)
        threshold_table(m, axes[2], n1, axes[3], n2, axes[4], n3, table.data());

    const GridArena arena(n_values, nq, n);
    char *inputs = nullptr;
    const int src = stage_inputs(g, arena, n_axes, axes, axis_len, table, n, &inputs);
    if (src != COVEST_OK)
        return src;
    bind_views(g, arena, inputs, n_axes, axis_len, flat_begin);

    // the block's sum of (T - 1), and the K-factored plan
    g->sum_t_minus_1 = (double)n; // basic: T = 2 everywhere
    g->q_sum_t_minus_1 = 0.0;
    g->has_plan = false;
    if (m->n_par == 5) {
        const TMinus1Sums sums = sum_t_minus_1(table, nq, flat_begin, flat_end);
        g->sum_t_minus_1 = sums.block;
        g->q_sum_t_minus_1 = sums.q;
        const int prc = build_factored_plan(g, axes, axis_len, table);
        if (prc != COVEST_OK)
            return prc;
    }
    if (g->upload_pending) { // an evaluation on another stream than the copies' waits for this
        if (!g->upload_ev)
            HIP_TRY(hipEventCreateWithFlags(&g->upload_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(g->upload_ev, nullptr));
    }
    g->counter_clean = true;
    g->configured = true;
    return COVEST_OK;
}

static void grid_release(covest_grid *g)
{
    (void)hipDeviceSynchronize(); // (the buffers go back to the process's cache, host.h: nothing may still work on them)
    DeviceIdleScope idle;
    if (g->upload_ev) {
        (void)hipEventDestroy(g->upload_ev);
        g->upload_ev = nullptr;
    }
    g->stage.release();
    g->stage_retired.clear();
    if (g->result_host) {
        pinned_block_give(g->result_host);
        g->result_host = nullptr;
    }
    g->arena.release();
    g->plan_buf.release();
    g->axis_buf.release();
    g->axis_host.release();
    for (covest_grid::Part &part : g->long_parts)
        part.buf.release();
    g->long_parts.clear();
    g->long_q_orig.release();
    g->long_partial.release();
    for (hipEvent_t e : g->ev_begin)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : g->ev_end)
        (void)hipEventDestroy(e);
    g->ev_begin.clear();
    g->ev_end.clear();
}

extern "C" {

int covest_grid_create(covest_model *m, int32_t n_axes, const double *const *axes,
                       const int64_t *axis_len, int64_t flat_begin, int64_t flat_end,
                       covest_grid **out)
{
    if (!m || !out)
        return fail(COVEST_E_INVALID, "covest_grid_create: null argument");
    *out = nullptr;
    covest_grid *g = new (std::nothrow) covest_grid();
    if (!g)
        return fail(COVEST_E_NOMEM, "covest_grid_create: out of host memory");
    g->model = m;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc == COVEST_OK)
        rc = grid_configure(g, n_axes, axes, axis_len, flat_begin, flat_end, "covest_grid_create");
    if (rc != COVEST_OK) {
        grid_release(g);
        delete g;
        return rc;
    }
    *out = g;
    return COVEST_OK;
}

int covest_grid_reset(covest_grid *g, int32_t n_axes, const double *const *axes, const int64_t *axis_len,
                      int64_t flat_begin, int64_t flat_end)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_reset: null grid");
    covest_model *m = g->model;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    if (g->last_stream || g->evaluated)
        HIP_TRY(hipStreamSynchronize(g->last_stream)); // nothing of the last evaluation may still be in flight
    if (g->upload_pending && !g->evaluated)
        HIP_TRY(hipStreamSynchronize(nullptr)); // (a reset that was never evaluated: its copies read the staging memory)
    g->upload_pending = false;
    g->stage_retired.clear(); // (nothing of the last configuration is read any more)
    g->async_uploads = true; // (from the first reset on: a handle that is re-configured is re-configured often)
    return grid_configure(g, n_axes, axes, axis_len, flat_begin, flat_end, "covest_grid_reset");
}

void covest_grid_destroy(covest_grid *g)
{
    if (!g)
        return;
    DeviceGuard dev_guard(g->model->device);
    grid_release(g);
    delete g;
}

int covest_grid_profile(covest_grid *g, int32_t enable)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_profile: null grid");
    g->profiling = enable != 0;
    g->ev_used = 0;
    return COVEST_OK;
}

int covest_grid_kernel_ms(covest_grid *g, double *total_ms, int64_t *launches)
{
    if (!g || !total_ms || !launches)
        return fail(COVEST_E_INVALID, "covest_grid_kernel_ms: null argument");
    DeviceGuard dev_guard(g->model->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    double sum = 0.0;
    for (size_t i = 0; i < g->ev_used; ++i) {
        HIP_TRY(hipEventSynchronize(g->ev_end[i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, g->ev_begin[i], g->ev_end[i]));
        sum += (double)ms;
    }
    *total_ms = sum;
    *launches = (int64_t)g->ev_used;
    return COVEST_OK;
}

int64_t covest_grid_size(const covest_grid *g) { return g ? g->flat_end - g->flat_begin : COVEST_E_INVALID; }

// The optional hipEvent bracket around the likelihood kernel (covest_grid_profile): takes the handle's next pair of
// events, records the first on the stream and hands back the second for the caller to record behind the launch
// (nullptr: not profiling).
static int bracket_begin(covest_grid *g, hipStream_t st, hipEvent_t *end)
{
    *end = nullptr;
    if (!g->profiling)
        return COVEST_OK;
    if (g->ev_used == g->ev_begin.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        g->ev_begin.push_back(a);
        g->ev_end.push_back(b);
    }
    hipEvent_t begin = g->ev_begin[g->ev_used];
    *end = g->ev_end[g->ev_used];
    g->ev_used++;
    HIP_TRY(hipEventRecord(begin, st));
    return COVEST_OK;
}

#ifdef COVEST_DIAG
// Diagnostic builds only (env COVEST_DIAG_QUEUE): how many points the recurrence kernel handed back for the strict
// evaluation, how long the row ranges they name are, and their threshold_o.
static int report_queue(covest_grid *g, hipStream_t st, int64_t n)
{
    if (!std::getenv("COVEST_DIAG_QUEUE"))
        return COVEST_OK;
    unsigned queued = 0;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&queued, g->sub_ctl.ptr, sizeof queued, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "covest_grid_eval: %u of %lld points handed back\n", queued, (long long)n);
    if (queued == 0)
        return COVEST_OK;
    std::vector<unsigned long long> words(queued); // the row ranges named: how long they are
    HIP_TRY(hipMemcpy(words.data(), g->sub_word.ptr, (size_t)queued * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum = 0;
    long long mx = 0, mn = 1 << 30, first_sum = 0;
    for (unsigned long long w : words) {
        const long long unit = sub_units16(w) ? 16 : 1;
        const long long len = ((long long)sub_last(w) - (long long)sub_first(w) + 1) * unit;
        sum += (double)len;
        mx = std::max(mx, len);
        mn = std::min(mn, len);
        first_sum += (long long)sub_first(w) * unit;
    }
    std::fprintf(stderr, "covest_grid_eval: rows named per point: min %lld mean %.1f max %lld; mean first row %.1f\n", mn,
                 sum / queued, mx, (double)first_sum / queued);
    if (!g->src.t_table)
        return COVEST_OK;
    const int64_t n_q = g->src.len[2] * g->src.len[3] * g->src.len[4]; // the queued points' threshold_o
    std::vector<int32_t> tt((size_t)n_q);
    std::vector<int64_t> idx(queued);
    HIP_TRY(hipMemcpy(tt.data(), g->src.t_table, (size_t)n_q * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(idx.data(), g->sub_index.ptr, (size_t)queued * sizeof(int64_t), hipMemcpyDeviceToHost));
    long long tmin = 1 << 30, tmax = 0;
    double tsum = 0;
    long long hist[6] = {0, 0, 0, 0, 0, 0}; // T <= 16, 32, 64, 128, 256, more
    for (int64_t i : idx) {
        const long long T = tt[(size_t)((g->src.flat_begin + i) % n_q)];
        tmin = std::min(tmin, T);
        tmax = std::max(tmax, T);
        tsum += (double)T;
        hist[T <= 16 ? 0 : T <= 32 ? 1 : T <= 64 ? 2 : T <= 128 ? 3 : T <= 256 ? 4 : 5]++;
    }
    std::fprintf(stderr, "covest_grid_eval: threshold_o of the queued points: min %lld mean %.1f max %lld; <=16 %lld <=32 %lld <=64 %lld <=128 %lld <=256 %lld more %lld\n",
                 tmin, tsum / queued, tmax, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
    return COVEST_OK;
}
#endif

// The hand-back queue as the recurrence kernel of an evaluation fills it (counter: the first word of sub_ctl) and as a
// strict pass that was put off finds it (the second word, where the arg-min left the queue's length: argmin.hip).
static SubList grid_queue(const covest_grid *g, bool put_off)
{
    return sub_list_of(g->model, g->has_plan ? g->t_max : 2, g->sub_index.ptr, g->sub_word.ptr,
                       g->sub_ctl.as<unsigned>() + (put_off ? 1 : 0));
}

// THE STRICT RE-EVALUATION PUT OFF.  What the pass of ll_fix.hip does is correct the values of the points that were handed
// back -- 2 962 of C3's 262 144, 7 791 of C2's 10^6 -- by adding non-positive terms to them (ll_fix.hip: value = ll[pt],
// then value += h_j (safe_log(p_j) - log p_clamp) per row with p_j < p_clamp), and the arg-min can be had without it
// (argmin.hip winner_unproven).  So a plain covest_grid_eval leaves it out, and whoever reads the values, or asks what was
// launched, gets it first: the pass on the evaluation's stream, over the very queue and with the very arguments the
// evaluation would have launched it with -- the values are the same bit for bit --, then the arg-min again, so that the
// pair in HBM and its host mirror describe the final values.  Nothing is owed: nothing happens.  The caller holds the
// model's lock and has the handle's device current.  *launched (or nullptr): whether anything went onto the stream.
static int grid_complete(covest_grid *g, bool *launched = nullptr)
{
    if (launched)
        *launched = false;
    if (!g->fix_pending)
        return COVEST_OK;
    const covest_model *m = g->model;
    const int64_t n = g->flat_end - g->flat_begin;
    hipStream_t st = g->last_stream;
    LaunchRecordScope record(g->record, true);
    HIP_TRY(launch_ll_fix_list(m->dm, m->tv, g->src, g->ll.as<double>(), grid_queue(g, true), st, n));
    HIP_TRY(launch_argmin(g->ll.as<double>(), n, g->flat_begin, g->partial_val.as<double>(), g->partial_idx.as<int64_t>(),
                          g->result.as<ArgminResult>(), g->result_host, nullptr, st));
    g->fix_pending = false;
    if (launched)
        *launched = true;
    return COVEST_OK;
}

// grid_complete from an entry point that holds nothing yet
static int grid_complete_entry(covest_grid *g, bool *launched = nullptr)
{
    if (launched)
        *launched = false;
    if (!g->fix_pending)
        return COVEST_OK;
    covest_model *m = g->model;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    return grid_complete(g, launched);
}

static int grid_eval(covest_grid *g, int32_t kernel, void *stream, bool scan, double scan_start)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_eval: null grid");
    if (!g->configured)
        return fail(COVEST_E_INVALID, "covest_grid_eval: the last covest_grid_reset of this handle failed; reset it again");
    covest_model *m = g->model;
    const int kern = resolve_kernel(m, kernel, g);
    if (kern < 0)
        return kern;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    LaunchRecordScope record(g->record);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = g->flat_end - g->flat_begin;
    if (g->upload_pending && st != nullptr && g->upload_ev)
        HIP_TRY(hipStreamWaitEvent(st, g->upload_ev, 0)); // (covest_grid_reset's copies run on the null stream)
    g->fix_pending = false;   // (a strict pass still owed for the last evaluation: dropped, its values are overwritten)
    g->counter_clean = false; // (until the arg-min below is launched: a failure on the way leaves the counter as it is)
    // The strict pass is put off where a recurrence kernel hands points back and the caller asked for no scan (its records
    // are strict running minima: made on final values; covest_grid_eval_scan is optimize_grid's, grids of a few thousand
    // points whose pass is 5 us)
    const bool hands_back = kern == COVEST_KERNEL_RECUR || (kern == COVEST_KERNEL_FACTORED && g->has_short_part);
    const bool put_off = hands_back && !scan && !g->fix_eager;
    hipEvent_t bracket_end = nullptr;
    rc = bracket_begin(g, st, &bracket_end);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY((put_off ? launch_ll_unfixed : launch_ll)(m, kern, g->src, n, g->ll.as<double>(), grid_queue(g, false), st,
                                                      &g->last_kernel, g));
    g->last_kernel_id = kern;
    if (bracket_end)
        HIP_TRY(hipEventRecord(bracket_end, st));
#ifdef COVEST_DIAG
    rc = report_queue(g, st, n);
    if (rc != COVEST_OK)
        return rc;
#endif
    if (!g->result_host) { // (page-locked, mapped: argmin_stage2 stores the winner there itself)
        static_assert(sizeof(ArgminResult) <= 64 && 64 + sizeof(ScanRecords) <= kPinnedBlockBytes, "pinned block");
        g->result_host = static_cast<ArgminResult *>(pinned_block_take());
        if (!g->result_host)
            return fail(COVEST_E_NOMEM, "covest_grid_eval: no page-locked memory for the result");
    }
    g->scan_valid = scan && n >= 1 && n <= kArgminSmall;
    if (g->scan_valid)
        HIP_TRY(launch_argmin_scan(g->ll.as<double>(), n, g->flat_begin, scan_start, g->result.as<ArgminResult>(), g->result_host,
                                   g->scan_host(), g->sub_ctl.as<unsigned>(), st));
    else
        HIP_TRY(launch_argmin_proving(g->ll.as<double>(), n, g->flat_begin, g->partial_val.as<double>(),
                                      g->partial_idx.as<int64_t>(), g->result.as<ArgminResult>(), g->result_host,
                                      g->sub_ctl.as<unsigned>(), put_off ? g->sub_index.as<int64_t>() : nullptr, st));
    g->counter_clean = true;
    g->fix_pending = put_off;
    g->last_stream = st;
    g->evaluated = true;
    return COVEST_OK;
}

int covest_grid_eval(covest_grid *g, int32_t kernel, void *stream) { return grid_eval(g, kernel, stream, false, 0.0); }

int covest_grid_eval_scan(covest_grid *g, int32_t kernel, void *stream, double start_min)
{
    return grid_eval(g, kernel, stream, true, start_min);
}

int covest_grid_complete(covest_grid *g)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_complete: null grid");
    return grid_complete_entry(g);
}

int covest_grid_fix_eager(covest_grid *g, int32_t eager)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_fix_eager: null grid");
    COVEST_TRY(grid_complete_entry(g));
    g->fix_eager = eager != 0;
    return COVEST_OK;
}

int covest_grid_scan(covest_grid *g, int32_t cap, int64_t *index, double *negll, int32_t *n_records, int32_t *truncated)
{
    if (!g || !n_records || !truncated || cap < 0 || (cap > 0 && (!index || !negll)))
        return fail(COVEST_E_INVALID, "covest_grid_scan: bad argument");
    if (!g->evaluated)
        return fail(COVEST_E_INVALID, "covest_grid_scan: covest_grid_eval_scan has not run");
    DeviceGuard dev_guard(g->model->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(g->last_stream));
    *n_records = 0;
    *truncated = 1; // (a grid beyond one workgroup's reach, or a plain covest_grid_eval: no list -- read the values back)
    if (!g->scan_valid)
        return COVEST_OK;
    const ScanRecords *sr = g->scan_host(); // (the kernel's own stores to page-locked memory)
    const int32_t have = sr->n;
    *truncated = (sr->truncated || have > cap) ? 1 : 0;
    const int32_t take = std::min(have, cap);
    for (int32_t i = 0; i < take; ++i) {
        index[i] = sr->rec[i].index;
        negll[i] = sr->rec[i].negll;
    }
    *n_records = take;
    return COVEST_OK;
}

int64_t covest_grid_launch_record(const covest_grid *g, char *buf, int64_t cap)
{
    if (!g || cap < 0 || (cap > 0 && !buf))
        return fail(COVEST_E_INVALID, "covest_grid_launch_record: bad argument");
    // (a handle is never a const object: the signature is the ABI's, the strict pass still owed belongs to the record)
    COVEST_TRY(grid_complete_entry(const_cast<covest_grid *>(g)));
    return launch_record_text(g->record, buf, cap);
}

int covest_grid_argmin(covest_grid *g, double *min_negll, int64_t *argmin_flat)
{
    if (!g || !min_negll || !argmin_flat)
        return fail(COVEST_E_INVALID, "covest_grid_argmin: null argument");
    if (!g->evaluated)
        return fail(COVEST_E_INVALID, "covest_grid_argmin: covest_grid_eval has not run");
    DeviceGuard dev_guard(g->model->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(hipStreamSynchronize(g->last_stream));
    if (g->fix_pending && g->result_host->unproven != 0) {
        // a queued point's final value could change the winner (argmin.hip winner_unproven): the strict pass after all
        COVEST_TRY(grid_complete_entry(g));
        HIP_TRY(hipStreamSynchronize(g->last_stream));
    }
    const ArgminResult r = *g->result_host; // (the arg-min kernel's own store: covest_grid_eval)
    *min_negll = r.min_negll;
    *argmin_flat = r.index < 0 ? -1 : g->flat_begin + r.index;
    return COVEST_OK;
}

int covest_grid_axis_min(covest_grid *g, uint32_t keep_mask, int64_t n_cells, double *min_negll, int64_t *argmin_flat)
{
    if (!g || !min_negll || !argmin_flat)
        return fail(COVEST_E_INVALID, "covest_grid_axis_min: null argument");
    if (!g->evaluated)
        return fail(COVEST_E_INVALID, "covest_grid_axis_min: covest_grid_eval has not run");
    covest_model *m = g->model;
    if (keep_mask >> m->n_par)
        return fail(COVEST_E_INVALID, "covest_grid_axis_min: keep_mask names an axis the grid does not have");
    int64_t cells = 1;
    for (int d = 0; d < m->n_par; ++d)
        if ((keep_mask >> d) & 1)
            cells *= g->len[d];
    if (n_cells != cells)
        return fail(COVEST_E_INVALID, "covest_grid_axis_min: n_cells is not the product of the kept axes' lengths");
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    AxisMinPlan p;
    if (!axis_min_plan(g->len, m->n_par, keep_mask, g->flat_begin, g->flat_end, &p))
        return fail(COVEST_E_INVALID, "covest_grid_axis_min: the axes do not fit a plan");
    // [min -LL | index] per cell, then the same per (slice, cell) where a cell's points are walked in slices
    const size_t nc = (size_t)n_cells, n_part = p.n_slices > 1 ? nc * (size_t)p.n_slices : 0;
    HIP_TRY(g->axis_buf.reserve(16 * (nc + n_part)));
    double *out_v = g->axis_buf.as<double>();
    int64_t *out_i = reinterpret_cast<int64_t *>(out_v + nc);
    double *part_v = reinterpret_cast<double *>(out_i + nc);
    int64_t *part_i = reinterpret_cast<int64_t *>(part_v + n_part);
    hipStream_t st = g->last_stream; // (behind the evaluation it reduces)
    COVEST_TRY(grid_complete(g));
    HIP_TRY(launch_axis_min(p, g->ll.as<double>(), part_v, part_i, out_v, out_i, st));
    if (16 * nc <= ((size_t)1 << 20)) { // one copy into page-locked memory (a pageable target costs a staging per call)
        HIP_TRY(g->axis_host.reserve(16 * nc));
        HIP_TRY(hipMemcpyAsync(g->axis_host.ptr, out_v, 16 * nc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(min_negll, g->axis_host.ptr, 8 * nc);
        std::memcpy(argmin_flat, static_cast<char *>(g->axis_host.ptr) + 8 * nc, 8 * nc);
    } else {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(min_negll, out_v, 8 * nc, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(argmin_flat, out_i, 8 * nc, hipMemcpyDeviceToHost));
    }
    return COVEST_OK;
}

// (a handle is never a const object: the two signatures are the ABI's)
const double *covest_grid_ll_device(const covest_grid *g)
{
    if (!g)
        return nullptr;
    // the strict pass still owed, and the wait for it: a caller that waited for the stream before it asked stays right
    bool launched = false;
    if (grid_complete_entry(const_cast<covest_grid *>(g), &launched) != COVEST_OK)
        return nullptr;
    if (launched) {
        DeviceGuard dev_guard(g->model->device);
        if (dev_guard.status() != COVEST_OK || hipStreamSynchronize(g->last_stream) != hipSuccess)
            return nullptr;
    }
    return g->ll.as<double>();
}

const double *covest_grid_argmin_pair_device(const covest_grid *g)
{
    if (!g)
        return nullptr;
    // Who takes the pair where it lies consumes it on the stream without a visit of the host (the ranks' exchange), so
    // nobody could act on an unproven winner: the pass still owed now, and inside every evaluation of this handle from
    // here on -- a second arg-min every step would cost more than the pass.
    covest_grid *gm = const_cast<covest_grid *>(g);
    if (grid_complete_entry(gm) != COVEST_OK)
        return nullptr;
    gm->fix_eager = true;
    return g->result.as<ArgminResult>()->pair; // (address arithmetic only: nothing is read here)
}

int covest_grid_ll_host(covest_grid *g, double *out_ll)
{
    if (!g || !out_ll)
        return fail(COVEST_E_INVALID, "covest_grid_ll_host: null argument");
    if (!g->evaluated)
        return fail(COVEST_E_INVALID, "covest_grid_ll_host: covest_grid_eval has not run");
    DeviceGuard dev_guard(g->model->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    const int64_t n = g->flat_end - g->flat_begin;
    COVEST_TRY(grid_complete_entry(g));
    HIP_TRY(hipStreamSynchronize(g->last_stream));
    if (n > 0)
        HIP_TRY(hipMemcpy(out_ll, g->ll.ptr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_grid_ll_provisional_host(covest_grid *g, double *out_ll)
{
    if (!g || !out_ll)
        return fail(COVEST_E_INVALID, "covest_grid_ll_provisional_host: null argument");
    if (!g->evaluated || !g->fix_pending)
        return fail(COVEST_E_INVALID, "covest_grid_ll_provisional_host: no strict pass is owed for the last evaluation");
    DeviceGuard dev_guard(g->model->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    const int64_t n = g->flat_end - g->flat_begin;
    HIP_TRY(hipStreamSynchronize(g->last_stream));
    if (n > 0)
        HIP_TRY(hipMemcpy(out_ll, g->ll.ptr, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int64_t covest_grid_diag(covest_grid *g, int64_t *out, int64_t n)
{
    if (!g || !g->has_plan || !g->plan.diag)
        return 0;
    const int nw = g->plan.n_threads / 64;
    const int64_t total = (g->plan.ce_end - g->plan.ce_begin) * g->plan.n_qblocks * nw * 8;
    if (out && n > 0) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(out, g->plan.diag, (size_t)std::min(n, total) * sizeof(int64_t), hipMemcpyDeviceToHost);
    }
    return total;
}

int covest_grid_work(const covest_grid *g, double *pmf_terms, double *flops, const char **kernel)
{
    if (!g)
        return fail(COVEST_E_INVALID, "covest_grid_work: null grid");
    const covest_model *m = g->model;
    const double n = (double)(g->flat_end - g->flat_begin);
    const double bins = (double)m->dm.bins.n;
    const double S = (double)m->dm.n_err;
    // SURVEY 8(d) unit: pmf terms of the per-point formulation, bins * S * sum(T - 1)
    const double terms = bins * S * g->sum_t_minus_1;
    if (pmf_terms)
        *pmf_terms = terms;
    if (flops) {
        if (g->last_kernel_id == COVEST_KERNEL_FACTORED) {
            // algorithmic minimum of the factored formulation (ll_factored.hip header):
            // per (c,e): G build 2 flop per (key, o, s), contraction 2 flop per (row, q, o < T_q) -- a row is a key,
            // or the sum of a whole count-less tile (tail != 0, tiles.h); where the plan shares steps between the
            // columns of a q-tile (tiles.h) the shared sums count once --, one log (25 flop) per
            // (counted key, q), prologue exps 25 per (o, s)
            const double n_ce = (double)(g->plan.ce_end - g->plan.ce_begin);
            const double max_o = (double)(g->t_max - 1);
            const double rows = m->tail_is_zero ? bins : m->rows_contracted;
            const double logged = m->tail_is_zero ? bins : m->keys_logged;
            *flops = n_ce * (bins * S * max_o * 2.0 + rows * g->contract_flops_per_row +
                             logged * (double)g->plan.n_q * 25.0 + 25.0 * S * max_o);
        } else {
            // 4 flop per pmf term + 25 per log + 25 per exp of the prologue
            *flops = 4.0 * terms + 25.0 * bins * n + 25.0 * S * g->sum_t_minus_1;
        }
    }
    if (kernel)
        *kernel = g->last_kernel;
    return COVEST_OK;
}

} // extern "C"
