// abi_model.cpp -- the model handle of the C ABI (include/covest_amd.h): covest_model_*, covest_eval_points,
// covest_probabilities, covest_reference_overflow, and the kernel dispatch the grid entry points share.
#include "host.h"

using namespace covest;

static int check_model_desc(const covest_model_desc *d)
{
    if (d->kind != COVEST_MODEL_BASIC && d->kind != COVEST_MODEL_REPEATS)
        return fail(COVEST_E_INVALID, "covest_model_create: unknown model kind");
    if (d->n_err < 1 || d->n_err > COVEST_MAX_ERROR_CLASSES || d->n_err > d->k + 1)
        return fail(COVEST_E_INVALID, "covest_model_create: n_err must be in 1..min(k+1, 64)");
    if (d->r <= 0 || d->k <= 0)
        return fail(COVEST_E_INVALID, "covest_model_create: k and r must be positive");
    if (d->n_keys < 0 || (d->n_keys > 0 && (!d->keys || !d->counts)) || !d->comb)
        return fail(COVEST_E_INVALID, "covest_model_create: null histogram or comb");
    if (d->kind == COVEST_MODEL_REPEATS && d->n_keys == 0)
        return fail(COVEST_E_INVALID,
                    "covest_model_create: repeats model needs a non-empty histogram "
                    "(max() of an empty dict raises in covest/models.py:186)");
    return COVEST_OK;
}

// what the kernels read of a model description (device_model.h), except its bins
static void fill_dev_model(DevModel &dm, const covest_model_desc *d, int n_par)
{
    dm.kind = d->kind;
    dm.k = d->k;
    dm.r = d->r;
    dm.n_err = d->n_err;
    for (int s = 0; s < kMaxErr; ++s) {
        dm.comb[s] = s < d->n_err ? d->comb[s] : 0.0;
        dm.pow3neg[s] = std::pow(3.0, (double)-s); // 3 ** -s, covest/models.py:77
        dm.ln_comb[s] = dm.comb[s] > 0.0 ? std::log(dm.comb[s]) : -INFINITY;
    }
    for (int i = 0; i < kMaxParams; ++i) {
        dm.lo[i] = i < n_par ? d->lo[i] : std::numeric_limits<double>::quiet_NaN();
        dm.hi[i] = i < n_par ? d->hi[i] : std::numeric_limits<double>::quiet_NaN();
    }
    dm.tail = d->tail;
}

extern "C" {

int covest_model_create(const covest_model_desc *d, covest_model **out)
{
    if (!d || !out)
        return fail(COVEST_E_INVALID, "covest_model_create: null argument");
    *out = nullptr;
    const int ok = check_model_desc(d);
    if (ok != COVEST_OK)
        return ok;

    int device = 0;
    const int drc = resolve_device(d->device, "covest_model_create", &device);
    if (drc != COVEST_OK)
        return drc;

    covest_model *m = new (std::nothrow) covest_model();
    if (!m)
        return fail(COVEST_E_NOMEM, "covest_model_create: out of host memory");
    m->device = device;
    m->n_par = d->kind == COVEST_MODEL_BASIC ? 2 : 5;
    m->n_keys = d->n_keys;
    m->threshold = d->threshold;
    m->has_threshold = d->has_threshold != 0;
    DevModel &dm = m->dm;
    fill_dev_model(dm, d, m->n_par);

    // Bin views.  When tail == 0 the tail term of covest/models.py:104 is exactly
    // 0 whatever sp_j is (0 * log of a positive number, or the else-branch), so
    // bins with h_j == 0 influence nothing and are dropped from the evaluated view.
    std::vector<double> key_a, lg_a, cnt_a, key_e, lg_e, cnt_e;
    std::vector<HostBin> eval_bins;
    const bool keep_all = d->tail == 0.0; // (with a tail the evaluated view IS the full view)
    if (keep_all) {
        key_a.reserve((size_t)d->n_keys);
        lg_a.reserve((size_t)d->n_keys);
        cnt_a.reserve((size_t)d->n_keys);
    }
    int hist_max = std::numeric_limits<int>::min();
    for (int64_t b = 0; b < d->n_keys; ++b)
        hist_max = std::max(hist_max, (int)d->keys[b]);
    lgamma_ensure(hist_max); // one lock for the whole histogram
    for (int64_t b = 0; b < d->n_keys; ++b) {
        const int j = d->keys[b];
        const int je = j > 0 ? j : 0; // the product loop of the C extension is empty for j <= 0
        const double kd = (double)je;
        const double lg = lgamma_at(je);
        const double h = d->counts[b];
        if (keep_all) {
            key_a.push_back(kd);
            lg_a.push_back(lg);
            cnt_a.push_back(h);
        }
        if (d->tail != 0.0 || h != 0.0) {
            key_e.push_back(kd);
            lg_e.push_back(lg);
            cnt_e.push_back(h);
            eval_bins.push_back({j, h, (int32_t)key_e.size() - 1});
        }
    }
    m->hist_max = d->n_keys > 0 ? hist_max : 0;
    m->tail_is_zero = d->tail == 0.0;
    m->key_max = hist_max > 0 ? hist_max : 0;

    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    m->host_all_key = std::move(key_a); // (empty with a tail: the evaluated view IS the full view)
    m->host_all_lgam = std::move(lg_a);
    m->host_all_cnt = std::move(cnt_a);
    if (rc == COVEST_OK)
        rc = upload_bins(m->bins_eval, dm.bins, key_e, lg_e, cnt_e);
    if (rc == COVEST_OK && d->tail != 0.0) {
        m->all_bins = dm.bins;
        m->all_bins_ready = true;
    }
    if (rc == COVEST_OK)
        rc = build_tiles(m, std::move(eval_bins));
    if (rc != COVEST_OK) {
        covest_model_destroy(m);
        return rc;
    }
    *out = m;
    return COVEST_OK;
}

void covest_model_destroy(covest_model *m)
{
    if (!m)
        return;
    DeviceGuard dev_guard(m->device);
    (void)hipDeviceSynchronize(); // (its small buffers go back to the process's cache: nothing may still work on them)
    DeviceIdleScope idle;
    delete m; // (its buffers go with it: host.h DevBuf / HostBuf)
}

int covest_model_param_count(const covest_model *m) { return m ? m->n_par : COVEST_E_INVALID; }

int64_t covest_model_bins_evaluated(const covest_model *m) { return m ? m->dm.bins.n : COVEST_E_INVALID; }

} // extern "C"

// Where the REFERENCE overflows (documented divergence).
// c_src/covest_poissonmodule.c:19-24 forms the whole product prod_{i<=j} (l / i) in x87 long double BEFORE any
// scaling, so truncated_poisson(l, j) is +inf as soon as the running product passes LDBL_MAX -- its largest
// value is reached at i = min(j, floor(l)): l^i / i!.  A likelihood evaluation calls it for every key j of the
// histogram and every l = o * l_s, o < threshold_o (covest/models.py:92-97, :235-241); the largest l against the
// largest key decides.  The kernels return the finite value the formula defines; this reports, per point,
// whether the reference itself would have returned inf / NaN there (and optimize_grid, covest/grid.py:65-70,
// would have selected it).
static bool reference_product_overflows(long double l, int64_t j_max)
{
    if (!(l > 0.0L) || j_max < 1)
        return false;
    const long double i_top = std::min<long double>((long double)j_max, floorl(l));
    if (i_top < 1.0L)
        return false;
    const long double ln_ldbl_max = 11356.523406294143949492L;
    return i_top * logl(l) - lgammal(i_top + 1.0L) > ln_ldbl_max;
}

static bool reference_overflows_at(const DevModel &dm, int n_par, const double *par_in, int T, int64_t key_max)
{
    double par[kMaxParams] = {0, 0, 0, 0, 0};
    for (int d = 0; d < n_par; ++d)
        par[d] = clamp_one(dm, d, par_in[d]);
    const double ck = par[0] * (double)(dm.r - dm.k + 1) / (double)dm.r; // covest/models.py:71-72
    double l_max = 0.0;
    for (int sidx = 0; sidx < dm.n_err; ++sidx) { // covest/models.py:76-79, same evaluation order
        double v = ck * dm.pow3neg[sidx];
        v = v * std::pow(1.0 - par[1], (double)(dm.k - sidx));
        v = v * std::pow(par[1], (double)sidx);
        if (v > l_max)
            l_max = v;
    }
    const int o_max = n_par == 5 ? T - 1 : 1;
    return o_max >= 1 && reference_product_overflows((long double)((double)o_max * l_max), key_max);
}

namespace covest {

// Resolve COVEST_KERNEL_* for a request (g == nullptr: a point list).  Returns the
// kernel to run or a negative error.
int resolve_kernel(const covest_model *m, int32_t kernel, const covest_grid *g)
{
    const bool basic_fast = m->has_tiles && m->dm.kind == COVEST_MODEL_BASIC;
    const bool factored_ok = g && g->has_plan;
    switch (kernel) {
    case COVEST_KERNEL_AUTO:
        if (basic_fast)
            return COVEST_KERNEL_RECUR;
        // the factored kernel pays when many weight vectors share each (c, e)
        if (factored_ok && g->plan.n_q >= 32)
            return COVEST_KERNEL_FACTORED;
        // a repeats-model point list: one workgroup per (point, key segment) (list mode) instead of one wave --
        // the latency path of refinements.  Long lists are throughput work and go to K-direct (and the list
        // mode's per-point tables, 13 KB each, stay small): see covest_eval_points.
        if (!g && m->has_tiles && m->dm.kind == COVEST_MODEL_REPEATS && m->dm.n_err <= 8)
            return COVEST_KERNEL_FACTORED;
        return COVEST_KERNEL_DIRECT;
    case COVEST_KERNEL_DIRECT:
        return COVEST_KERNEL_DIRECT;
    case COVEST_KERNEL_DIRECT_REF:
        return COVEST_KERNEL_DIRECT_REF;
    case COVEST_KERNEL_RECUR:
        if (basic_fast)
            return COVEST_KERNEL_RECUR;
        return fail(COVEST_E_INVALID, "recurrence kernel needs the basic model, max_error <= 32 and keys in 1..16384");
    case COVEST_KERNEL_FACTORED:
        if (factored_ok || (!g && m->has_tiles && m->dm.kind == COVEST_MODEL_REPEATS && m->dm.n_err <= 8))
            return COVEST_KERNEL_FACTORED;
        return fail(COVEST_E_INVALID, "factored kernel needs the repeats model, keys in 1..16384 and max_error <= 32 "
                                      "(<= 8 for a point list)");
    default:
        return fail(COVEST_E_INVALID, "unknown kernel");
    }
}

// K-factored on a dense grid: the part whose weight vectors fit a workgroup's lanes writes log-likelihoods (and is
// followed by the pass that patches what it handed back); the long weight vectors go chunk by chunk of copy numbers
// into an HBM buffer of p_j, one batch of (c, e) rows at a time, and ll_finish_dense takes their logs.
// with_fix == false: the patching pass is the caller's to launch, any time before the short part's values are read (the
// long weight vectors are other points of the grid: nothing below reads or writes what the pass touches).
static hipError_t launch_factored_grid(covest_grid *g, double *out, const SubList &sub, hipStream_t st, bool with_fix)
{
    const covest_model *m = g->model;
    if (g->has_short_part) {
        record_factored_plan(g->plan, g->n_shared_tiles, false);
        hipError_t e = launch_ll_factored(m->dm, m->tv, g->plan, out, sub, st);
        if (e != hipSuccess)
            return e;
        if (with_fix)
            e = launch_ll_fix_list(m->dm, m->tv, g->src, out, sub, st, g->flat_end - g->flat_begin);
        if (e != hipSuccess)
            return e;
    }
    if (g->n_long_tiles > 0) {
        const int64_t n_cols = (int64_t)g->n_long_tiles * 16, n_rows = (int64_t)m->tv.n_items * kTileBins;
        const int64_t ce_begin = g->plan.ce_begin, ce_end = g->plan.ce_end;
        const int64_t per_ce = n_cols * n_rows * (int64_t)sizeof(double);
        const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(ce_end - ce_begin, ((int64_t)1 << 30) / per_ce));
        hipError_t e = g->long_partial.reserve((size_t)(batch * per_ce));
        if (e != hipSuccess)
            return e;
        for (const covest_grid::Part &part : g->long_parts)
            record_factored_plan(part.plan, 0, true);
        for (int64_t first = ce_begin; first < ce_end; first += batch) {
            const int64_t last = std::min(ce_end, first + batch);
            for (covest_grid::Part &part : g->long_parts) {
                FactoredPlan pl = part.plan;
                pl.ce_begin = first;
                pl.ce_end = last;
                pl.ce_first = first;
                pl.n_cols_partial = n_cols;
                pl.partial = g->long_partial.as<double>();
                e = launch_ll_factored(m->dm, m->tv, pl, out, sub, st);
                if (e != hipSuccess)
                    return e;
            }
            e = launch_ll_finish_dense(m->dm, m->tv, g->src, g->long_partial.as<double>(), first, last - first, n_cols,
                                       g->long_q_orig.as<int32_t>(), g->plan.n_q, g->flat_end, out, st);
            if (e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

SubList sub_list_of(const covest_model *m, int t_max, void *index, void *word, void *ctl)
{
    SubList l{};
    l.p_clamp = clamp_for(m, t_max);
    l.log_p_clamp = std::log(l.p_clamp);
    l.count = static_cast<unsigned *>(ctl);
    l.index = static_cast<int64_t *>(index);
    l.word = static_cast<unsigned long long *>(word);
    l.index_offset = 0;
#ifdef COVEST_DIAG // diagnostic builds only (handback.h SubList::diag_class): the shipped library has no knobs
    const char *dc = std::getenv("COVEST_DIAG_BASIC_CLASS");
    l.diag_class = dc ? std::atoi(dc) : 0;
#endif
    return l;
}

// `sub`: the queue the recurrence kernels append the points they hand back to (handback.h) -- drained right
// behind them by the fix pass; K-direct has nothing to hand back.  The queue must be empty (counter 0) on entry.
static hipError_t launch_ll_with(const covest_model *m, int kernel, const PointSource &src, int64_t n, double *out,
                                 const SubList &sub, hipStream_t st, const char **name, const covest_grid *g, bool with_fix)
{
    if (kernel == COVEST_KERNEL_FACTORED) {
        if (name)
            *name = "ll_factored";
        return launch_factored_grid(const_cast<covest_grid *>(g), out, sub, st, with_fix);
    }
    if (kernel == COVEST_KERNEL_RECUR) {
        if (name)
            *name = "ll_basic";
        hipError_t e = launch_ll_basic(m->dm, m->tv, src, n, out, sub, st);
        return e != hipSuccess || !with_fix ? e : launch_ll_fix_list(m->dm, m->tv, src, out, sub, st, n);
    }
    if (name)
        *name = kernel == COVEST_KERNEL_DIRECT_REF ? "ll_direct_ref" : "ll_direct";
    return launch_ll_direct(m->dm, src, n, out, nullptr, st, kernel == COVEST_KERNEL_DIRECT_REF);
}

hipError_t launch_ll(const covest_model *m, int kernel, const PointSource &src, int64_t n, double *out, const SubList &sub,
                     hipStream_t st, const char **name, const covest_grid *g)
{
    return launch_ll_with(m, kernel, src, n, out, sub, st, name, g, true);
}

// The same WITHOUT the pass that patches the handed-back points: the queue is left as the recurrence kernel filled it,
// the queued points' values provisional (handback.h) -- a grid handle's, whose launch_ll_fix_list comes when somebody
// reads the values (abi_grid.cpp grid_complete).
hipError_t launch_ll_unfixed(const covest_model *m, int kernel, const PointSource &src, int64_t n, double *out,
                             const SubList &sub, hipStream_t st, const char **name, const covest_grid *g)
{
    return launch_ll_with(m, kernel, src, n, out, sub, st, name, g, false);
}

} // namespace covest

constexpr int64_t kInPlaceMaxListPoints = 4; // repeats model, list mode: tables read in place (13 KB a point, 8 workgroups each)

// The queue a point-list launch hands points back through (handback.h): room for n entries, empty.  The counter is
// zeroed without waiting for it: whatever touches it afterwards -- the kernels, the blocking copies of fix_points_host
// -- is work of the same null stream and comes behind the fill, and the host never reads it.
static int reserve_point_queue(covest_model *m, int64_t n)
{
    HIP_TRY(m->ws_sub_index.reserve((size_t)n * sizeof(int64_t)));
    HIP_TRY(m->ws_sub_word.reserve((size_t)n * sizeof(unsigned long long)));
    HIP_TRY(m->ws_sub_ctl.reserve(sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(m->ws_sub_ctl.ptr, 0, sizeof(unsigned), nullptr));
    return COVEST_OK;
}

// A point list where the kernels read it and where they leave its result: stage_points.
struct StagedPoints {
    PointSource src{};
    double *out = nullptr;
    bool in_place = false; // both are the model's page-locked blocks, mapped into the device's address space
};

// Stage a whole list -- parameters, behind them the thresholds -- in the model's page-locked block, with room for
// out_bytes of results.  A SHORT list (what scipy's refinement issues: a point and its finite-difference neighbours)
// moves nothing through the copy engine: it is read, and its results written, IN PLACE in mapped host memory -- one wait
// for the stream per call; a blocking copy either side of the launch was two thirds of a basic-model evaluation's 48 us.
// A longer list goes up in ONE copy, from the page-locked block and not the caller's pageable array (HostBuf, host.h).
static int stage_points(covest_model *m, int64_t n, const double *params, size_t out_bytes, StagedPoints &sp)
{
    const int P = m->n_par;
    const std::vector<int32_t> t = point_thresholds(m, n, params);
    const size_t par_bytes = (size_t)n * P * sizeof(double), t_bytes = (t.size() * sizeof(int32_t) + 7) / 8 * 8;
    HIP_TRY(m->ws_stage.reserve(par_bytes + t_bytes));
    char *base = m->ws_stage.as<char>();
    std::memcpy(base, params, par_bytes);
    if (!t.empty())
        std::memcpy(base + par_bytes, t.data(), t.size() * sizeof(int32_t));
    sp.in_place = n <= kInPlaceMaxPoints;
    if (sp.in_place) {
        HIP_TRY(m->ws_result.reserve(out_bytes));
        sp.out = m->ws_result.as<double>();
    } else {
        HIP_TRY(m->ws_params.reserve(par_bytes + t_bytes));
        HIP_TRY(m->ws_out.reserve(out_bytes));
        HIP_TRY(hipMemcpy(m->ws_params.ptr, base, par_bytes + t_bytes, hipMemcpyHostToDevice));
        base = m->ws_params.as<char>();
        sp.out = m->ws_out.as<double>();
    }
    sp.src.is_grid = 0;
    sp.src.params = reinterpret_cast<const double *>(base);
    sp.src.t_list = P == 5 ? reinterpret_cast<const int32_t *>(base + par_bytes) : nullptr;
    return COVEST_OK;
}

// (in place: once the caller has waited for the stream)
static int read_result(const StagedPoints &sp, double *dst, size_t first, size_t count)
{
    if (sp.in_place)
        std::memcpy(dst, sp.out + first, count * sizeof(double));
    else
        HIP_TRY(hipMemcpy(dst, sp.out + first, count * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

// (parameters, threshold_o) of the points of a repeats-model list that idx names, in idx's order
static void gather_points(const double *params, const std::vector<int32_t> &t, const std::vector<int64_t> &idx,
                          std::vector<double> &sub_par, std::vector<int32_t> &sub_t)
{
    sub_par.resize(idx.size() * 5);
    sub_t.resize(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
        std::memcpy(&sub_par[k * 5], params + idx[k] * 5, 5 * sizeof(double));
        sub_t[k] = t[(size_t)idx[k]];
    }
}

// ... and up to ws_params and ws_t, for the routes that read a plain list; their values come back from ws_out, to where
// idx says.  (eval_points_list has reserved all three for the whole call.)
static int upload_points(covest_model *m, const double *params, const std::vector<int32_t> &t, const std::vector<int64_t> &idx,
                         PointSource &src)
{
    std::vector<double> sub_par;
    std::vector<int32_t> sub_t;
    gather_points(params, t, idx, sub_par, sub_t);
    HIP_TRY(hipMemcpy(m->ws_params.ptr, sub_par.data(), sub_par.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->ws_t.ptr, sub_t.data(), sub_t.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    src = PointSource{};
    src.is_grid = 0;
    src.params = m->ws_params.as<double>();
    src.t_list = m->ws_t.as<int32_t>();
    return COVEST_OK;
}

static int download_values(covest_model *m, const std::vector<int64_t> &idx, double *out_ll)
{
    std::vector<double> got(idx.size());
    HIP_TRY(hipMemcpy(got.data(), m->ws_out.ptr, got.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < idx.size(); ++k)
        out_ll[idx[k]] = got[k];
    return COVEST_OK;
}

// One point of list mode 1 from its n_seg parts {LL part, sp_j part (hi, lo), side word}: the value, the segments added
// in order and the tail term behind them, and in *word the segments' handed-back units, merged (0: none).
static double combine_segments(const double *parts, int n_seg, double tail, unsigned long long *word)
{
    double ll = 0.0, hi = 0.0, lo = 0.0;
    unsigned u_first = 0xFFFFFFFFu, u_last = 0;
    bool any_unit = false;
    for (int sg = 0; sg < n_seg; ++sg) {
        const double *o = &parts[(size_t)sg * 4];
        ll += o[0];
        unsigned long long w;
        std::memcpy(&w, &o[3], sizeof w);
        if (w != 0) {
            any_unit = true;
            u_first = std::min(u_first, sub_first(w));
            u_last = std::max(u_last, sub_last(w));
        }
        const double sum = hi + o[1], bb = sum - hi; // two-sum, as the kernels' CompSum
        lo += ((hi - (sum - bb)) + (o[1] - bb)) + o[2];
        hi = sum;
    }
    double tail_term = 0.0;
    if (tail != 0.0) { // tail * log(1 - min(1, sp)), covest/models.py:103-105
        double sp = hi + lo;
        if (!(sp < 1.0))
            sp = 1.0;
        if (sp < 1.0)
            tail_term = tail * std::log(1.0 - sp);
    }
    *word = any_unit ? sub_word(u_first, u_last, true) : 0ull;
    return ll + tail_term;
}

// threshold_o - 1 within a workgroup's lanes: one workgroup per (point, key segment), list mode 1.  The kernel stores the
// segments' parts straight into mapped host memory, 256 bytes a point, and the list's tables go up asynchronously: ONE
// wait for the stream instead of a blocking copy either side of the launch, a third of a single evaluation's 75 us.
static int list_points_fitting(covest_model *m, const double *params, const std::vector<int32_t> &t,
                               const std::vector<int64_t> &idx, const SubList &none, double *out_ll,
                               std::vector<unsigned long long> &words)
{
    std::vector<double> sub_par;
    std::vector<int32_t> sub_t;
    gather_points(params, t, idx, sub_par, sub_t);
    FactoredPlan pl;
    const int rc = build_list_plan(m, (int64_t)idx.size(), sub_par.data(), sub_t, nullptr, m->ws_plan, pl,
                                   (int64_t)idx.size() <= kInPlaceMaxListPoints);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(m->ws_result.reserve(idx.size() * (size_t)pl.n_seg * 4 * sizeof(double)));
    pl.partial = m->ws_result.as<double>();
    record_factored_plan(pl, 0, false);
    HIP_TRY(launch_ll_factored(m->dm, m->tv, pl, m->ws_out.as<double>(), none, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    for (size_t k = 0; k < idx.size(); ++k)
        out_ll[idx[k]] = combine_segments(pl.partial + k * (size_t)pl.n_seg * 4, pl.n_seg, m->dm.tail, &words[(size_t)idx[k]]);
    return COVEST_OK;
}

// threshold_o beyond that: the point is cut into chunks of kListLanes copy numbers, one workgroup each (list mode 2),
// and ll_finish_partials adds the chunks' p_j and takes the logs.
static int list_points_chunked(covest_model *m, const double *params, const std::vector<int32_t> &t,
                               const std::vector<int64_t> &idx, const SubList &none, double *out_ll)
{
    std::vector<double> item_par, point_par;
    std::vector<int32_t> item_t, item_ob, first_item(idx.size() + 1, 0), point_t;
    gather_points(params, t, idx, point_par, point_t);
    for (size_t k = 0; k < idx.size(); ++k) {
        for (int ob = 0; ob < point_t[k] - 1; ob += kListLanes) {
            item_par.insert(item_par.end(), &point_par[5 * k], &point_par[5 * k] + 5);
            item_t.push_back(point_t[k]);
            item_ob.push_back(ob);
        }
        first_item[k + 1] = (int32_t)item_t.size();
    }
    const int64_t n_items = (int64_t)item_t.size();
    const size_t n_keys = (size_t)m->tv.n_items * kTileBins; // rows of the items (tiles.h)
    FactoredPlan pl;
    const int rc = build_list_plan(m, n_items, item_par.data(), item_t, &item_ob, m->ws_plan2, pl);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(m->ws_partial.reserve((size_t)n_items * n_keys * sizeof(double)));
    // what the two kernels read besides the plan, in one copy: the items' first copy numbers | each point's first item |
    // the points' thresholds | (8-byte aligned) the points' parameters
    const size_t items_bytes = (size_t)n_items * sizeof(int32_t), first_bytes = first_item.size() * sizeof(int32_t);
    const size_t pt_bytes = point_t.size() * sizeof(int32_t);
    const size_t int_bytes = ((items_bytes + first_bytes + pt_bytes + 7) / 8) * 8;
    std::vector<char> stage(int_bytes + point_par.size() * sizeof(double));
    std::memcpy(stage.data(), item_ob.data(), items_bytes);
    std::memcpy(stage.data() + items_bytes, first_item.data(), first_bytes);
    std::memcpy(stage.data() + items_bytes + first_bytes, point_t.data(), pt_bytes);
    std::memcpy(stage.data() + int_bytes, point_par.data(), point_par.size() * sizeof(double));
    HIP_TRY(m->ws_items.reserve(stage.size()));
    const char *ib = m->ws_items.as<char>();
    HIP_TRY(hipMemcpy(m->ws_items.ptr, stage.data(), stage.size(), hipMemcpyHostToDevice));
    pl.list_mode = 2;
    pl.item_obase = reinterpret_cast<const int32_t *>(ib);
    pl.partial = m->ws_partial.as<double>();
    record_factored_plan(pl, 0, false);
    HIP_TRY(launch_ll_factored(m->dm, m->tv, pl, m->ws_out.as<double>(), none, nullptr));
    HIP_TRY(launch_ll_finish_partials(m->dm, m->tv, pl.partial, reinterpret_cast<const int32_t *>(ib + items_bytes),
                                      reinterpret_cast<const double *>(ib + int_bytes),
                                      reinterpret_cast<const int32_t *>(ib + items_bytes + first_bytes), (int64_t)idx.size(),
                                      m->ws_out.as<double>(), nullptr));
    return download_values(m, idx, out_ll);
}

// threshold_o == 1, nothing to sum over: K-direct
static int list_points_direct(covest_model *m, const double *params, const std::vector<int32_t> &t,
                              const std::vector<int64_t> &idx, const SubList &none, double *out_ll)
{
    PointSource src;
    const int rc = upload_points(m, params, t, idx, src);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(launch_ll(m, COVEST_KERNEL_DIRECT, src, (int64_t)idx.size(), m->ws_out.as<double>(), none, nullptr, nullptr));
    return download_values(m, idx, out_ll);
}

// Add the strict evaluation of the keys list mode 1 handed back (words[i] != 0, handback.h) to out_ll[i].
static int fix_points_host(covest_model *m, int64_t n, const double *params, const std::vector<int32_t> &t, double *out_ll,
                           const std::vector<unsigned long long> &words)
{
    std::vector<int64_t> again;
    for (int64_t i = 0; i < n; ++i)
        if (words[(size_t)i] != 0 && std::isfinite(out_ll[i]))
            again.push_back(i);
    if (again.empty())
        return COVEST_OK;
    const size_t na = again.size();
    std::vector<double> sub_ll(na);
    std::vector<unsigned long long> sub_w(na);
    std::vector<int64_t> sub_i(na);
    for (size_t k = 0; k < na; ++k) {
        sub_ll[k] = out_ll[again[k]];
        sub_w[k] = words[(size_t)again[k]];
        sub_i[k] = (int64_t)k;
    }
    int rc = reserve_point_queue(m, (int64_t)na);
    if (rc != COVEST_OK)
        return rc;
    PointSource src;
    rc = upload_points(m, params, t, again, src);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(hipMemcpy(m->ws_out.ptr, sub_ll.data(), na * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->ws_sub_index.ptr, sub_i.data(), na * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->ws_sub_word.ptr, sub_w.data(), na * sizeof(unsigned long long), hipMemcpyHostToDevice));
    const unsigned count = (unsigned)na; // the queue arrives full
    HIP_TRY(hipMemcpy(m->ws_sub_ctl.ptr, &count, sizeof count, hipMemcpyHostToDevice));
    HIP_TRY(launch_ll_fix_list(m->dm, m->tv, src, m->ws_out.as<double>(),
                               sub_list_of(m, kListLanes + 1, m->ws_sub_index.ptr, m->ws_sub_word.ptr, m->ws_sub_ctl.ptr),
                               nullptr, (int64_t)na));
    return download_values(m, again, out_ll);
}

// A repeats-model point list through K-factored's list mode.  A point's route depends on its own threshold_o only --
// never on what else is in the call (refinements compare values across calls).  Called with the model locked.
static int eval_points_list(covest_model *m, int64_t n, const double *params, double *out_ll)
{
    const std::vector<int32_t> t = point_thresholds(m, n, params);
    std::vector<int64_t> fits, big, rest;
    for (int64_t i = 0; i < n; ++i) {
        const int o_max = t[(size_t)i] - 1;
        (o_max < 1 ? rest : o_max <= kListLanes ? fits : big).push_back(i);
    }
    // (what upload_points and download_values use: any subset of the call fits)
    HIP_TRY(m->ws_out.reserve((size_t)n * sizeof(double)));
    HIP_TRY(m->ws_params.reserve((size_t)n * 5 * sizeof(double)));
    HIP_TRY(m->ws_t.reserve((size_t)n * sizeof(int32_t)));
    const SubList none = sub_list_of(m, kListLanes + 1, nullptr, nullptr, nullptr); // (list mode and K-direct hand nothing back)
    std::vector<unsigned long long> words((size_t)n, 0ull); // keys handed back per point (handback.h)
    int rc = fits.empty() ? COVEST_OK : list_points_fitting(m, params, t, fits, none, out_ll, words);
    if (rc == COVEST_OK && !big.empty())
        rc = list_points_chunked(m, params, t, big, none, out_ll);
    if (rc == COVEST_OK && !rest.empty())
        rc = list_points_direct(m, params, t, rest, none, out_ll);
    return rc != COVEST_OK ? rc : fix_points_host(m, n, params, t, out_ll, words);
}

// covest_eval_points_grad (order 1), covest_eval_points_hess (order 2) and covest_eval_points_opg (order kDerivOpg): the
// device leaves values | gradients | matrices (Hessians or score outer products; no last block for order 1) in one
// buffer; `who` names the entry point in the messages.
static int eval_points_deriv(covest_model *m, int order, int64_t n, const double *params, double *out_ll, double *out_grad,
                             double *out_hess, const char *who)
{
    if (!m || n < 0 || (n > 0 && (!params || !out_ll || !out_grad || (order != 1 && !out_hess))))
        return fail(COVEST_E_INVALID, std::string(who) + ": bad argument");
    if (n == 0)
        return COVEST_OK;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    LaunchRecordScope record(m->record);
    const int P = m->n_par;
    StagedPoints sp;
    rc = stage_points(m, n, params, (size_t)n * (1 + P + (order != 1 ? P * P : 0)) * sizeof(double), sp);
    if (rc != COVEST_OK)
        return rc;
    HIP_TRY(m->ws_partial.reserve(ll_deriv_partial_bytes(m->dm, order, n)));
    HIP_TRY(launch_ll_deriv(m->dm, order, sp.src, n, m->ws_partial.as<double>(), sp.out, sp.out + n, sp.out + n * (1 + P),
                            nullptr));
    if (sp.in_place)
        HIP_TRY(hipStreamSynchronize(nullptr));
    rc = read_result(sp, out_ll, 0, (size_t)n);
    if (rc == COVEST_OK)
        rc = read_result(sp, out_grad, (size_t)n, (size_t)n * P);
    if (rc == COVEST_OK && order != 1)
        rc = read_result(sp, out_hess, (size_t)n * (1 + P), (size_t)n * P * P);
    return rc;
}

extern "C" {

int covest_eval_points(covest_model *m, int64_t n, const double *params, double *out_ll,
                       int32_t kernel)
{
    if (!m || n < 0 || (n > 0 && (!params || !out_ll)))
        return fail(COVEST_E_INVALID, "covest_eval_points: bad argument");
    if (n == 0)
        return COVEST_OK;
    int kern = resolve_kernel(m, kernel, nullptr);
    if (kern < 0)
        return kern;
    if (kern == COVEST_KERNEL_FACTORED && n > kListModeMaxPoints) {
        if (kernel == COVEST_KERNEL_FACTORED)
            return fail(COVEST_E_INVALID, "factored kernel: a point list of more than 4096 points (use a grid, or K-direct)");
        kern = COVEST_KERNEL_DIRECT; // AUTO: throughput work
    }
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    LaunchRecordScope record(m->record);
    if (kern == COVEST_KERNEL_FACTORED)
        return eval_points_list(m, n, params, out_ll);
    StagedPoints sp;
    rc = stage_points(m, n, params, (size_t)n * sizeof(double), sp);
    if (rc != COVEST_OK)
        return rc;
    SubList queue = sub_list_of(m, m->n_par == 5 ? kListLanes + 1 : 2, nullptr, nullptr, nullptr); // (K-direct hands nothing back)
    if (kern == COVEST_KERNEL_RECUR) { // K-basic hands points back through the queue, and launch_ll's fix pass drains it
        rc = reserve_point_queue(m, n);
        if (rc != COVEST_OK)
            return rc;
        queue = sub_list_of(m, 2, m->ws_sub_index.ptr, m->ws_sub_word.ptr, m->ws_sub_ctl.ptr);
    }
    HIP_TRY(launch_ll(m, kern, sp.src, n, sp.out, queue, nullptr, nullptr));
    if (sp.in_place)
        HIP_TRY(hipStreamSynchronize(nullptr));
    return read_result(sp, out_ll, 0, (size_t)n);
}

int covest_eval_points_grad(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad)
{
    return eval_points_deriv(m, 1, n, params, out_ll, out_grad, nullptr, "covest_eval_points_grad");
}

int covest_eval_points_hess(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad,
                            double *out_hess)
{
    return eval_points_deriv(m, 2, n, params, out_ll, out_grad, out_hess, "covest_eval_points_hess");
}

int covest_eval_points_opg(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad,
                           double *out_opg)
{
    return eval_points_deriv(m, kDerivOpg, n, params, out_ll, out_grad, out_opg, "covest_eval_points_opg");
}

int64_t covest_model_launch_record(covest_model *m, char *buf, int64_t cap)
{
    if (!m || cap < 0 || (cap > 0 && !buf))
        return fail(COVEST_E_INVALID, "covest_model_launch_record: bad argument");
    std::lock_guard<std::mutex> guard(m->lock);
    return launch_record_text(m->record, buf, cap);
}

int covest_reference_overflow(const covest_model *m, int64_t n, const double *params, uint8_t *flags)
{
    if (!m || n < 0 || (n > 0 && (!params || !flags)))
        return fail(COVEST_E_INVALID, "covest_reference_overflow: bad argument");
    const int P = m->n_par;
    const std::vector<int32_t> t = point_thresholds(m, n, params);
    for (int64_t i = 0; i < n; ++i)
        flags[i] = reference_overflows_at(m->dm, P, params + i * P, t.empty() ? 2 : t[(size_t)i], m->key_max) ? 1 : 0;
    return COVEST_OK;
}

int covest_probabilities(covest_model *m, const double *params, int32_t clamp, double *out_p)
{
    if (!m || !params || (m->n_keys > 0 && !out_p))
        return fail(COVEST_E_INVALID, "covest_probabilities: bad argument");
    if (m->n_keys == 0)
        return COVEST_OK;
    std::lock_guard<std::mutex> guard(m->lock);
    DeviceGuard dev_guard(m->device);
    int rc = dev_guard.status();
    if (rc != COVEST_OK)
        return rc;
    const int P = m->n_par;
    HIP_TRY(m->ws_params.reserve((size_t)P * sizeof(double)));
    HIP_TRY(m->ws_out.reserve(sizeof(double)));
    HIP_TRY(m->ws_p.reserve((size_t)m->n_keys * sizeof(double)));
    HIP_TRY(hipMemcpy(m->ws_params.ptr, params, (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    PointSource src{};
    src.params = m->ws_params.as<double>();
    if (P == 5) {
        const int32_t t = clamp ? threshold_for_point(m, params)
                                : threshold_o_host(params[2], params[3], params[4], m->threshold,
                                                   m->has_threshold, m->hist_max);
        HIP_TRY(m->ws_t.reserve(sizeof(int32_t)));
        HIP_TRY(hipMemcpy(m->ws_t.ptr, &t, sizeof(int32_t), hipMemcpyHostToDevice));
        src.t_list = m->ws_t.as<int32_t>();
    }
    COVEST_TRY(ensure_all_bins(m));
    DevModel full = m->dm;
    full.bins = m->all_bins;
    if (!clamp)
        for (int i = 0; i < kMaxParams; ++i)
            full.lo[i] = full.hi[i] = std::numeric_limits<double>::quiet_NaN();
    HIP_TRY(launch_ll_direct(full, src, 1, m->ws_out.as<double>(), m->ws_p.as<double>(), nullptr));
    HIP_TRY(hipMemcpy(out_p, m->ws_p.ptr, (size_t)m->n_keys * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
