// host_common.cpp -- error state, device selection, the ln j! table and threshold_o (host arithmetic: libm,
// as CPython) of libcovest_amd.so.  Compiled with hipcc, links only the HIP runtime.  There is no CPU compute path in
// this library: every likelihood value comes out of a gfx950 kernel.
#include "factored_launch.h" // K-factored's variants, for covest_compiled_variants
#include "host.h"

using namespace covest;

namespace {
thread_local std::string g_last_error;
} // namespace

namespace covest {

// (also for the library's other translation units, reads_io.cpp: record the message covest_last_error returns)
int set_error(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    if (e == hipErrorOutOfMemory) { // an allocation that did not fit: the caller may fall back (include/covest_amd.h)
        (void)hipGetLastError();    // (the runtime keeps the error until somebody reads it)
        return COVEST_E_NOMEM;
    }
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
               ? COVEST_E_NO_DEVICE
               : COVEST_E_HIP;
}

namespace {
struct DevCache {
    std::mutex mu;
    struct Entry {
        int device;
        void *ptr;
        size_t cap;
    };
    std::vector<Entry> free_list;
    size_t bytes = 0;
    std::vector<std::pair<int, void *>> pinned; // (device, block)
};
DevCache &dev_cache()
{
    static DevCache *c = new DevCache; // (never freed: the runtime may be gone when statics are destroyed)
    return *c;
}
constexpr size_t kDevCacheEntryMax = (size_t)8 << 20, kDevCacheTotalMax = (size_t)64 << 20;
} // namespace

namespace {
thread_local int tls_device_idle = 0;
}
DeviceIdleScope::DeviceIdleScope() { ++tls_device_idle; }
DeviceIdleScope::~DeviceIdleScope() { --tls_device_idle; }
bool DeviceIdleScope::active() { return tls_device_idle > 0; }

bool dev_cache_take(size_t bytes, void **ptr, size_t *cap, int *device)
{
    if (bytes == 0 || bytes > kDevCacheEntryMax)
        return false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return false;
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> hold(c.mu);
    size_t best = c.free_list.size();
    for (size_t i = 0; i < c.free_list.size(); ++i) {
        const DevCache::Entry &e = c.free_list[i];
        // best fit, and no buffer more than four times what is asked for (a 4 MB buffer for 200 bytes would starve the
        // next large request)
        if (e.device == dev && e.cap >= bytes && e.cap <= std::max<size_t>(4 * bytes, 4096) &&
            (best == c.free_list.size() || e.cap < c.free_list[best].cap))
            best = i;
    }
    if (best == c.free_list.size())
        return false;
    *ptr = c.free_list[best].ptr;
    *cap = c.free_list[best].cap;
    *device = dev;
    c.bytes -= c.free_list[best].cap;
    c.free_list.erase(c.free_list.begin() + (std::ptrdiff_t)best);
    return true;
}

bool dev_cache_give(void *ptr, size_t cap, int dev)
{
    if (!ptr || cap == 0 || cap > kDevCacheEntryMax || dev < 0)
        return false;
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> hold(c.mu);
    if (c.bytes + cap > kDevCacheTotalMax || c.free_list.size() >= 256)
        return false;
    c.free_list.push_back({dev, ptr, cap});
    c.bytes += cap;
    return true;
}

void *pinned_block_take()
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        DevCache &c = dev_cache();
        std::lock_guard<std::mutex> hold(c.mu);
        for (size_t i = 0; i < c.pinned.size(); ++i)
            if (c.pinned[i].first == dev) {
                void *p = c.pinned[i].second;
                c.pinned.erase(c.pinned.begin() + (std::ptrdiff_t)i);
                return p;
            }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, kPinnedBlockBytes, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void pinned_block_give(void *p)
{
    if (!p)
        return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> hold(c.mu);
    if (c.pinned.size() < 64) {
        c.pinned.push_back({dev, p});
        return;
    }
    (void)hipHostFree(p);
}

SharedStage &shared_stage()
{
    static SharedStage *s = new SharedStage; // (never freed: the runtime may be gone when statics are destroyed)
    return *s;
}

int stage_upload(void *d_dst, const void *src, size_t bytes, const char *what)
{
    constexpr size_t kPiece = (size_t)8 << 20;
    SharedStage &ss = shared_stage();
    std::lock_guard<std::mutex> hold(ss.mu);
    hipError_t e = ss.buf.reserve(std::min(bytes, kPiece));
    for (size_t at = 0; e == hipSuccess && at < bytes; at += kPiece) {
        const size_t len = std::min(bytes - at, kPiece);
        std::memcpy(ss.buf.ptr, static_cast<const char *>(src) + at, len);
        e = hipMemcpy(static_cast<char *>(d_dst) + at, ss.buf.ptr, len, hipMemcpyHostToDevice);
    }
    return e == hipSuccess ? COVEST_OK : fail_hip(e, what);
}


// RepeatsModel.get_b_o / get_hist_threshold, covest/models.py:185-208, with libm
// pow as CPython's float ** int.  b_o is non-increasing in o for o >= 3 when
// 0 <= 1-q <= 1, so the first crossing is found by bisection and then confirmed
// against its left neighbours with the very same pow calls the linear scan of
// the reference would make; outside that domain the scan itself is used.
// (pw(o) = pow(1 - q, o - 3): libm's, called directly or looked up in a table of the very same calls)
template <class PowFn>
static int threshold_o_impl(double q1, double q2, double q, double thr, bool has_thr, int hist_max, PowFn pw)
{
    if (!has_thr)
        return hist_max;
    if (hist_max > 1 && q1 <= thr)
        return 1;
    if (hist_max > 2 && (1 - q1) * q2 <= thr)
        return 2;
    if (hist_max <= 3)
        return hist_max;
    const double head = (1 - q1) * (1 - q2) * q;
    const double base = 1 - q;
    const int last = hist_max - 1; // o ranges over 3..last
    auto weight = [&](int o) { return head * pw(o); };
    if (!(base >= 0.0 && base <= 1.0) || !(head == head)) {
        for (int o = 3; o <= last; ++o)
            if (weight(o) <= thr)
                return o;
        return hist_max;
    }
    if (weight(3) <= thr)
        return 3;
    if (!(weight(last) <= thr))
        return hist_max;
    int lo = 3, hi = last; // f(lo) > thr, f(hi) <= thr
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (weight(mid) <= thr)
            hi = mid;
        else
            lo = mid;
    }
    while (hi > 3 && weight(hi - 1) <= thr)
        --hi;
    return hi;
}

int threshold_o_host(double q1, double q2, double q, double thr, bool has_thr, int hist_max)
{
    const double base = 1 - q;
    return threshold_o_impl(q1, q2, q, thr, has_thr, hist_max, [&](int o) { return std::pow(base, (double)(o - 3)); });
}

// threshold_o over the (q1, q2, q) product of three axes (clamped to the model's bounds), last axis fastest: the same
// decisions as threshold_o_host point by point, but the powers of one q are computed ONCE for all its (q1, q2) -- an
// optimize_grid iteration asks for 216 thresholds of 6 different q, 1 300 calls of pow otherwise (round 4).
void threshold_table(const covest_model *m, const double *a1, int64_t n1, const double *a2, int64_t n2, const double *a3,
                     int64_t n3, int32_t *out)
{
    // pw[o] = pow(1 - q, o - 3) for the q in hand; NaN: not asked for yet (the entries a q touched are set back, not the
    // whole table: 10 000 keys and 16 values of q would be a megabyte of fills)
    std::vector<double> pw((size_t)std::max(m->hist_max, 4) + 1, std::numeric_limits<double>::quiet_NaN());
    std::vector<int> touched;
    for (int64_t c = 0; c < n3; ++c) {
        const double q = clamp_one(m->dm, 4, a3[c]);
        const double base = 1 - q;
        for (int o : touched)
            pw[(size_t)o] = std::numeric_limits<double>::quiet_NaN();
        touched.clear();
        auto pow_of = [&](int o) {
            double &v = pw[(size_t)o];
            if (v != v) {
                v = std::pow(base, (double)(o - 3));
                touched.push_back(o); // (a power that IS NaN -- q is -- is computed again each time: still the same value)
            }
            return v;
        };
        for (int64_t a = 0; a < n1; ++a) {
            const double q1 = clamp_one(m->dm, 2, a1[a]);
            for (int64_t b = 0; b < n2; ++b)
                out[(a * n2 + b) * n3 + c] = threshold_o_impl(q1, clamp_one(m->dm, 3, a2[b]), q, m->threshold, m->has_threshold,
                                                              m->hist_max, pow_of);
        }
    }
}

double clamp_one(const DevModel &dm, int d, double v)
{
    const double lo = dm.lo[d], hi = dm.hi[d];
    if (lo == lo && v < lo)
        return lo;
    if (hi == hi && v > hi)
        return hi;
    return v;
}

int threshold_for_point(const covest_model *m, const double *par)
{
    return threshold_o_host(clamp_one(m->dm, 2, par[2]), clamp_one(m->dm, 3, par[3]),
                            clamp_one(m->dm, 4, par[4]), m->threshold, m->has_threshold, m->hist_max);
}

// threshold_o of every point of a list (repeats model; the basic model has none: empty)
std::vector<int32_t> point_thresholds(const covest_model *m, int64_t n, const double *params)
{
    std::vector<int32_t> t;
    if (m->n_par == 5) {
        t.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i)
            t[(size_t)i] = threshold_for_point(m, params + i * 5);
    }
    return t;
}

// The view over EVERY key is only needed by covest_probabilities and by a batch's table: uploaded on first use.  With the
// model locked and its device current.
int ensure_all_bins(covest_model *m)
{
    if (m->all_bins_ready)
        return COVEST_OK;
    COVEST_TRY(upload_bins(m->bins_all, m->all_bins, m->host_all_key, m->host_all_lgam, m->host_all_cnt));
    m->all_bins_ready = true;
    return COVEST_OK;
}

// device < 0 = the calling thread's current device (include/covest_amd.h); checked against the device count.
int resolve_device(int device, const char *who, int *out)
{
    if (device < 0) {
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess)
            return fail_hip(e, "hipGetDevice");
    }
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess)
        return fail_hip(e, "hipGetDeviceCount");
    if (n_dev <= 0 || device >= n_dev)
        return fail(COVEST_E_NO_DEVICE, std::string(who) + ": no such HIP device");
    *out = device;
    return COVEST_OK;
}

// ln j! = lgamma(j + 1) rounded from long double, for j = 0, 1, 2, ...: a process-wide table grown on demand
// (lgammal costs ~100 ns; a 10 000-key histogram paid 1 ms of it per model handle).  A deque: growing it never moves
// the entries already there, so a caller that has made sure of the first n (lgamma_ensure, under the lock) may read
// them without it (lgamma_at) -- one lock per histogram instead of one per key.
std::mutex g_lgamma_lock;
std::deque<double> g_lgamma_table;
constexpr int64_t kLgammaTableMax = (int64_t)1 << 22; // beyond any histogram the fast paths accept: not cached

void lgamma_ensure(int64_t j_max)
{
    if (j_max > kLgammaTableMax)
        j_max = kLgammaTableMax;
    std::lock_guard<std::mutex> guard(g_lgamma_lock);
    for (size_t v = g_lgamma_table.size(); v <= (size_t)std::max<int64_t>(j_max, 0); ++v)
        g_lgamma_table.push_back((double)lgammal((long double)v + 1.0L));
}

// (after lgamma_ensure(j) or larger)
// (after lgamma_ensure(j) or larger)
double lgamma_at(int64_t j)
{
    if (j < 0)
        j = 0;
    if (j > kLgammaTableMax)
        return (double)lgammal((long double)j + 1.0L);
    return g_lgamma_table[(size_t)j];
}

double lgamma_of_factorial(int64_t j)
{
    lgamma_ensure(j);
    return lgamma_at(j);
}

// ---- the launch record (kernels.h)
namespace {
thread_local LaunchRecord *tls_record = nullptr;
} // namespace

LaunchRecordScope::LaunchRecordScope(LaunchRecord &r) : prev(tls_record)
{
    r.clear();
    tls_record = &r;
}
LaunchRecordScope::LaunchRecordScope(LaunchRecord &r, bool append) : prev(tls_record)
{
    if (!append)
        r.clear();
    tls_record = &r;
}
LaunchRecordScope::~LaunchRecordScope() { tls_record = prev; }

void record_launch(const char *name, int64_t launches)
{
    LaunchRecord *r = tls_record;
    if (!r || launches <= 0)
        return;
    for (int i = 0; i < r->n_entries; ++i)
        if (r->entries[i].name == name) { // (the names are the tables' own pointers)
            r->entries[i].launches += launches;
            return;
        }
    if (r->n_entries < (int)(sizeof r->entries / sizeof r->entries[0]))
        r->entries[r->n_entries++] = LaunchRecord::Entry{name, launches};
}

void record_factored_plan(const FactoredPlan &plan, int shared_tiles, bool long_part)
{
    LaunchRecord *r = tls_record;
    if (!r || r->n_plans >= (int)(sizeof r->plans / sizeof r->plans[0]))
        return;
    r->plans[r->n_plans++] = LaunchRecord::Plan{plan.n_threads, plan.n_buf,  plan.ld,        plan.n_qblocks,
                                                shared_tiles,   plan.n_pass, plan.list_mode, long_part,
                                                plan.col_floor};
}

// "launch <name> <count>" and "plan <key>=<value> ..." lines; the whole text's length is returned, at most cap - 1
// characters of it are written to buf, behind them a NUL
int64_t launch_record_text(const LaunchRecord &r, char *buf, int64_t cap)
{
    std::string t;
    char line[256];
    for (int i = 0; i < r.n_entries; ++i) {
        std::snprintf(line, sizeof line, "launch %s %lld\n", r.entries[i].name, (long long)r.entries[i].launches);
        t += line;
    }
    for (int i = 0; i < r.n_plans; ++i) {
        const LaunchRecord::Plan &p = r.plans[i];
        std::snprintf(line, sizeof line,
                      "plan n_threads=%d n_buf=%d ld=%d n_qblocks=%d shared_tiles=%d long=%d n_pass=%d list_mode=%d col_floor=%d\n",
                      p.n_threads, p.n_buf, p.ld, p.n_qblocks, p.shared_tiles, p.long_part ? 1 : 0, p.n_pass, p.list_mode, p.col_floor);
        t += line;
    }
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(t.size(), (size_t)(cap - 1));
        std::memcpy(buf, t.data(), n);
        buf[n] = '\0';
    }
    return (int64_t)t.size();
}

} // namespace covest

extern "C" {

int64_t covest_compiled_variants(char *buf, int64_t cap)
{
    if (cap < 0 || (cap > 0 && !buf))
        return fail(COVEST_E_INVALID, "covest_compiled_variants: bad argument");
    std::string t;
    auto add = [&](const char *const *names, int n) {
        for (int i = 0; i < n; ++i) {
            t += names[i];
            t += '\n';
        }
    };
    for (const FactoredVariant &v : kFactoredVariantTable)
        add(&v.name, 1);
    add(kFactoredFinishNames, 2);
    add(kBasicVariantNames, kBasicVariants);
    add(kFixVariantNames, kFixVariants);
    add(kArgminVariantNames, kArgminVariants);
    add(kDerivVariantNames, kDerivVariants);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(t.size(), (size_t)(cap - 1));
        std::memcpy(buf, t.data(), n);
        buf[n] = '\0';
    }
    return (int64_t)t.size();
}

int covest_abi_version(void) { return COVEST_ABI_VERSION; }

const char *covest_last_error(void) { return g_last_error.c_str(); }

int covest_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
        return fail_hip(e, "hipGetDeviceCount");
    return n;
}

int covest_threshold_o(int64_t n, const double *q123, double threshold, int32_t has_threshold,
                       int32_t hist_max, int32_t *out)
{
    if (n < 0 || (n > 0 && (!q123 || !out)))
        return fail(COVEST_E_INVALID, "covest_threshold_o: bad argument");
    for (int64_t i = 0; i < n; ++i)
        out[i] = threshold_o_host(q123[3 * i], q123[3 * i + 1], q123[3 * i + 2], threshold,
                                  has_threshold != 0, hist_max);
    return COVEST_OK;
}

} // extern "C"
