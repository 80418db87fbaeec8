// kmer_host.cpp -- the k-mer counter of the C ABI (include/covest_amd.h): covest_kmer_* over kmer_count.hip,
// kmer_wide.hip and kmer_bulk.hip.  The arithmetic of the partitioned path is kmer_plan.h's.
#include "host.h"

using namespace covest;

namespace {

// ---- the counter's table: one word a key (kmer_count.hip) or `wide` words (kmer_wide.hip); nobody else asks which ----
int64_t slots_of(const covest_kmer *c)
{
    return (int64_t)((c->wide ? c->wtable.mask : c->table.mask) + 1);
}

// an emptied table of at least min_slots slots in `slots`: described by `t` or by `wt`, whichever the keys take
int table_alloc(const covest_kmer *c, int64_t min_slots, KmerTable &t, KmerWideTable &wt, DevBuf &slots)
{
    const int lg = kmer_plan::log2_slots_for(min_slots, c->wide ? 38 : 40);
    const size_t n = (size_t)1 << lg;
    if (c->wide) {
        wt = KmerWideTable{nullptr, n - 1, lg, c->k, c->wide, 2 * c->wide}; // (1 + w words, rounded up to a power of two)
        HIP_TRY(slots.reserve(n * (size_t)wt.stride * sizeof(unsigned long long)));
        wt.words = slots.as<unsigned long long>();
        HIP_TRY(launch_kmer_wide_clear(wt, nullptr));
    } else {
        HIP_TRY(slots.reserve(n * sizeof(KmerSlot)));
        t = KmerTable{slots.as<KmerSlot>(), n - 1, lg, c->k};
        HIP_TRY(launch_kmer_fill_empty(t, nullptr));
    }
    return COVEST_OK;
}

hipError_t table_clear(const covest_kmer *c, hipStream_t st)
{
    return c->wide ? launch_kmer_wide_clear(c->wtable, st) : launch_kmer_fill_empty(c->table, st);
}

hipError_t table_rehash(const covest_kmer *c, const KmerTable &bigger, const KmerWideTable &wbigger)
{
    return c->wide ? launch_kmer_wide_rehash(c->wtable, wbigger, c->flag.as<int>(), nullptr)
                   : launch_kmer_rehash(c->table, bigger, c->flag.as<int>(), nullptr);
}

// need == 0: {max count, distinct keys} into c->stats; else the count-of-counts below `need` into c->hist
hipError_t table_scan(const covest_kmer *c, unsigned long long need)
{
    unsigned long long *stats = c->stats.as<unsigned long long>(), *hist = c->hist.as<unsigned long long>();
    if (need == 0)
        return c->wide ? launch_kmer_wide_stats(c->wtable, stats, nullptr) : launch_kmer_stats(c->table, stats, nullptr);
    return c->wide ? launch_kmer_wide_histogram(c->wtable, hist, need, nullptr)
                   : launch_kmer_histogram(c->table, hist, need, nullptr);
}

// ---- covest_kmer_count_reads_device, stage by stage -----------------------------------------------------
// One call: the reads as the layout stage left them, the plan, the device blocks, what the passes reported.
struct BulkCall {
    covest_kmer *c;
    hipStream_t st;
    const uint8_t *d_bases;
    const int64_t *d_offsets; // null: n_reads reads of read_len bases each
    int64_t n_reads, read_len, n_bases_total;
    int64_t ragged_base0 = 0, ragged_total = 0; // reads with offsets: offsets[0], and the bytes from there to the last end
    KmerBulk p{};
    size_t n_buckets = 0;
    BulkControl *ctl = nullptr;
    BulkLists *lists = nullptr;
    unsigned *first_read = nullptr; // reads of different lengths: the read of every tile's first byte (kmer_bulk.hip)
    unsigned long long room = 0, n_overflowed = 0, listed[2] = {0, 0};
};

// Reads that come with offsets but are all of one length (a sequencer's usually are) take the path of reads of one
// length: its threads need not look up which read their byte belongs to.
int resolve_layout(BulkCall &b)
{
    if (!b.d_offsets || b.n_reads <= 0)
        return COVEST_OK;
    HIP_TRY(b.c->part.ctl.reserve(sizeof(BulkControl)));
    unsigned long long *flag = &b.c->part.ctl.as<BulkControl>()->one_length;
    const unsigned long long one = 1;
    unsigned long long same = 0;
    int64_t two[2] = {0, 0}, last = 0;
    HIP_TRY(hipMemcpyAsync(flag, &one, sizeof one, hipMemcpyHostToDevice, b.st));
    HIP_TRY(launch_kmer_one_length(b.d_offsets, b.n_reads, flag, b.st));
    HIP_TRY(hipMemcpyAsync(&same, flag, sizeof same, hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(two, b.d_offsets, sizeof two, hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(&last, b.d_offsets + b.n_reads, sizeof last, hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipStreamSynchronize(b.st));
    const int64_t len0 = two[1] - two[0];
    b.ragged_base0 = two[0];
    b.ragged_total = last - two[0];
    if (b.ragged_total < 0 || b.n_reads >= ((int64_t)1 << 32))
        return fail(COVEST_E_INVALID, "covest_kmer_count_reads_device: offsets do not ascend, or 2^32 reads and more");
    b.n_bases_total = b.ragged_total;
    if (same && len0 >= b.c->k && len0 < ((int64_t)1 << 30)) {
        b.d_bases += two[0];
        b.d_offsets = nullptr;
        b.read_len = len0;
    }
    return COVEST_OK;
}

#ifdef COVEST_DIAG // diagnostic builds only: the shipped library has no knobs
void diag_overrides(const BulkCall &b, kmer_plan::Partition &plan)
{
    using namespace kmer_plan;
    const int k = b.c->k;
    const bool ragged = b.d_offsets != nullptr;
    if (const char *e = std::getenv("COVEST_KMER_M"))
        plan.m = std::max(8, std::min(std::atoi(e), std::min(k - 1, 15)));
    if (const char *e = std::getenv("COVEST_KMER_LG"))
        plan.log2_buckets = std::max(10, std::min(std::atoi(e), 26));
    plan.w = k - plan.m + 1;
    plan.sample = sample_for(plan_windows(k, ragged, b.n_reads, b.read_len, b.n_bases_total),
                             plan_bytes(ragged, b.n_reads, b.read_len, b.n_bases_total), plan.w, plan.log2_buckets);
    if (const char *e = std::getenv("COVEST_KMER_SAMPLE"))
        plan.sample = std::max(1, std::atoi(e));
}
#endif

void plan_call(BulkCall &b)
{
    kmer_plan::Partition plan = kmer_plan::plan_partition(b.c->k, b.d_offsets != nullptr, b.n_reads, b.read_len, b.n_bases_total);
#ifdef COVEST_DIAG
    diag_overrides(b, plan);
#endif
    b.p.k = b.c->k;
    b.p.m = plan.m;
    b.p.w = plan.w;
    b.p.canonical = b.c->canonical;
    b.p.log2_buckets = plan.log2_buckets;
    b.p.max_run = plan.max_run;
    b.p.sample = plan.sample;
    b.n_buckets = (size_t)1 << plan.log2_buckets;
}

// the per-bucket arrays and the control blocks (kept from call to call), the plan's pointers to them, the events
int reserve_buffers(BulkCall &b)
{
    BulkState &s = b.c->part;
    HIP_TRY(s.sampled.reserve(b.n_buckets * sizeof(unsigned)));
    HIP_TRY(s.cursor.reserve(b.n_buckets * sizeof(ulonglong2)));
    HIP_TRY(s.fill.reserve(b.n_buckets * sizeof(unsigned long long)));
    HIP_TRY(s.lists.reserve(BulkLists::bytes(b.n_buckets)));
    HIP_TRY(s.partial.reserve((b.n_buckets / 1024 + 1) * sizeof(unsigned long long)));
    HIP_TRY(s.ctl.reserve(sizeof(BulkControl)));
    HIP_TRY(s.hist.reserve((size_t)kBulkHistLen * sizeof(unsigned long long)));
    HIP_TRY(s.big.reserve((size_t)kBulkBigCap * sizeof(unsigned long long)));
    b.p.sampled = s.sampled.as<unsigned>();
    b.p.ctl = s.cursor.as<ulonglong2>();
    b.p.fill = s.fill.as<KmerBulk::fill_t>();
    b.ctl = s.ctl.as<BulkControl>();
    b.lists = s.lists.as<BulkLists>();
    b.p.ovf_count = b.ctl->ovf_count;
    b.c->bulk = false;
    for (hipEvent_t &e : s.ev)
        if (!e)
            HIP_TRY(hipEventCreate(&e));
    return COVEST_OK;
}

// pass 0: room per bucket from the sample, the buckets' places; the room in all comes back
int pass0_and_room(BulkCall &b)
{
    BulkState &s = b.c->part;
    HIP_TRY(hipEventRecord(s.ev[0], b.st));
    HIP_TRY(hipMemsetAsync(b.p.sampled, 0, b.n_buckets * sizeof(unsigned), b.st));
    HIP_TRY(hipMemsetAsync(b.ctl, 0, sizeof(BulkControl), b.st));
    if (b.d_offsets && b.n_reads > 0) { // (here, not with the other buffers: growing one waits for the device)
        HIP_TRY(s.tile_reads.reserve((size_t)kmer_plan::ragged_tiles(b.ragged_total, b.p.w) * sizeof(unsigned)));
        b.first_read = s.tile_reads.as<unsigned>();
    }
    HIP_TRY(launch_kmer_scatter(b.d_bases, b.d_offsets, b.n_reads, b.read_len, b.ragged_base0, b.ragged_total, b.first_read,
                                b.p, true, b.st));
    HIP_TRY(launch_kmer_place_buckets(b.p, s.partial.as<unsigned long long>(), &b.ctl->room, b.st));
    HIP_TRY(hipEventRecord(s.ev[1], b.st));
    HIP_TRY(hipMemcpyAsync(&b.room, &b.ctl->room, sizeof(b.room), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipStreamSynchronize(b.st));
    return COVEST_OK;
}

// do the records fit the device and the caller's limit?  Then their room, and the overflow list's
int reserve_records(BulkCall &b)
{
    BulkState &s = b.c->part;
    b.p.overflow_cap = kmer_plan::overflow_cap_for(b.room);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t have = s.recs.cap + s.ovf.cap;
    const double want = kmer_plan::records_bytes_wanted(b.room, b.p.overflow_cap);
    if (want > 0.85 * (double)(free_b + have))
        return fail(COVEST_E_NOMEM, "covest_kmer_count_reads_device: the buckets do not fit the free device memory");
    if (s.mem_limit > 0 && want > (double)s.mem_limit)
        return fail(COVEST_E_NOMEM, "covest_kmer_count_reads_device: the buckets do not fit the caller's limit "
                                    "(covest_kmer_memory_limit)");
    HIP_TRY(s.recs.reserve(std::max<size_t>((size_t)b.room, 1) * sizeof(ulonglong2)));
    HIP_TRY(s.ovf.reserve((size_t)b.p.overflow_cap * kOvfShards * sizeof(ulonglong2)));
    b.p.recs = s.recs.as<ulonglong2>();
    b.p.overflow = s.ovf.as<ulonglong2>();
    return COVEST_OK;
}

// pass 1: the records to their buckets; pass 2: the buckets counted in LDS
int scatter_and_count(BulkCall &b)
{
    BulkState &s = b.c->part;
    HIP_TRY(hipMemsetAsync(b.lists, 0, sizeof(BulkLists), b.st));
    HIP_TRY(hipMemsetAsync(b.p.fill, 0, b.n_buckets * sizeof(KmerBulk::fill_t), b.st));
    HIP_TRY(hipMemsetAsync(s.hist.ptr, 0, (size_t)kBulkHistLen * sizeof(unsigned long long), b.st));
    int n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, b.c->device) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    HIP_TRY(launch_kmer_scatter(b.d_bases, b.d_offsets, b.n_reads, b.read_len, b.ragged_base0, b.ragged_total, b.first_read,
                                b.p, false, b.st));
    HIP_TRY(hipEventRecord(s.ev[2], b.st));
    HIP_TRY(launch_kmer_bucket_count(b.p, s.hist.as<unsigned long long>(), kBulkHistLen, b.ctl->stats,
                                     s.big.as<unsigned long long>(), kBulkBigCap, &b.lists->later_n, b.lists->later_list(),
                                     b.lists->to_table, b.lists->to_table_list(b.n_buckets),
                                     kmer_plan::small_buckets(b.room, b.n_buckets), n_cu, b.st));
    HIP_TRY(hipEventRecord(s.ev[3], b.st));
    return COVEST_OK;
}

// what the passes reported, and whether the result stands
int read_back(BulkCall &b)
{
    BulkState &s = b.c->part;
    std::vector<unsigned long long> parts((size_t)kOvfShards * kOvfStride);
    HIP_TRY(hipMemcpyAsync(parts.data(), b.ctl->ovf_count, sizeof(b.ctl->ovf_count), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(s.stats, b.ctl->stats, sizeof(s.stats), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(&s.later_n, &b.lists->later_n, sizeof(unsigned), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipMemcpyAsync(b.listed, b.lists->to_table, sizeof(b.listed), hipMemcpyDeviceToHost, b.st));
    HIP_TRY(hipStreamSynchronize(b.st));
    bool part_full = false;
    for (int i = 0; i < kOvfShards; ++i) {
        b.n_overflowed += parts[(size_t)i * kOvfStride];
        part_full = part_full || parts[(size_t)i * kOvfStride] > b.p.overflow_cap;
    }
    if (part_full)
        return fail(COVEST_E_NOMEM, "covest_kmer_count_reads_device: the overflow list is full (the sample of the reads "
                                    "misjudged the buckets); use covest_kmer_add_device");
    if (s.stats[2] > kBulkBigCap)
        return fail(COVEST_E_NOMEM, "covest_kmer_count_reads_device: more than 4096 keys with counts beyond 2^20");
    return COVEST_OK;
}

// What no LDS table could hold -- the buckets that overflowed their room (all their records: a key is counted in one
// place), those with too many distinct keys -- goes to the table in HBM, sized now that the need is known.
int hand_back(BulkCall &b)
{
    covest_kmer *c = b.c;
    c->part.table_used = b.n_overflowed > 0 || b.listed[0] > 0;
    if (!c->part.table_used)
        return COVEST_OK;
    const int64_t want = kmer_plan::hand_back_slots(b.listed[1], b.n_overflowed, b.p.max_run);
    if (slots_of(c) < want) { // (nothing to keep: the counter was to be emptied)
        KmerTable bigger{};
        KmerWideTable none{};
        DevBuf slots;
        COVEST_TRY(table_alloc(c, want, bigger, none, slots));
        c->slots = std::move(slots);
        c->table = bigger;
    }
    HIP_TRY(table_clear(c, b.st));
    HIP_TRY(hipMemsetAsync(c->flag.ptr, 0, sizeof(int), b.st));
    HIP_TRY(launch_kmer_to_table(b.p, b.n_overflowed > 0, c->table, c->flag.as<int>(), b.lists->to_table,
                                 b.lists->to_table_list(b.n_buckets), b.st));
    HIP_TRY(hipStreamSynchronize(b.st));
    return kmer_check_overflow(c, "covest_kmer_count_reads_device");
}

// the passes' times, what covest_kmer_partition_info reports; the counter holds the result from here on
int finish(BulkCall &b)
{
    BulkState &s = b.c->part;
    HIP_TRY(hipEventRecord(s.ev[4], b.st));
    HIP_TRY(hipEventSynchronize(s.ev[4]));
    for (int i = 0; i < 4; ++i)
        HIP_TRY(hipEventElapsedTime(&s.ms[i], s.ev[i], s.ev[i + 1]));
    s.info[0] = (int64_t)b.n_buckets;
    s.info[1] = b.p.m;
    s.info[2] = b.p.sample;
    s.info[3] = (int64_t)b.room;
    s.info[4] = (int64_t)b.n_overflowed;
    s.to_table_n = b.listed[0];
    b.c->bulk = true;
    return COVEST_OK;
}

} // namespace

namespace covest {

// The adds' way into the table of either key width (abi_update.cpp).  d_weights null: every occurrence counts once;
// else a weight a read (covest_kmer_add_weighted*)
hipError_t table_count(const covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                       int64_t read_len, const uint32_t *d_weights, hipStream_t st)
{
    int *flag = c->flag.as<int>();
    return c->wide ? launch_kmer_wide_count(d_bases, d_offsets, n_reads, read_len, c->canonical, c->wtable, flag, st, d_weights)
                   : launch_kmer_count(d_bases, d_offsets, n_reads, read_len, c->k, c->canonical, c->table, flag, st,
                                       d_weights);
}

int KmerHostCall::open(const uint8_t *bases, const int64_t *offsets, int64_t n_reads)
{
    COVEST_TRY(dev_.status());
    const size_t n_pos = (size_t)(offsets[n_reads] - offsets[0]), n = (size_t)n_reads;
    HIP_TRY(c->ws_bases.reserve(std::max<size_t>(n_pos, 1)));
    HIP_TRY(c->ws_offsets.reserve((n + 1) * sizeof(int64_t)));
    if (n_pos)
        HIP_TRY(hipMemcpy(c->ws_bases.ptr, bases + offsets[0], n_pos, hipMemcpyHostToDevice));
    std::vector<int64_t> rel(n + 1);
    for (size_t i = 0; i <= n; ++i)
        rel[i] = offsets[i] - offsets[0];
    HIP_TRY(hipMemcpy(c->ws_offsets.ptr, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return COVEST_OK;
}

// the two sticky words (host.h), the overflow first: an overflow set before an underflow is still reported
int kmer_check_overflow(covest_kmer *c, const char *who)
{
    int flag[kKmerStickyWords] = {0, 0};
    HIP_TRY(hipMemcpy(flag, c->flag.ptr, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag[kKmerOverflowWord])
        return fail(COVEST_E_NOMEM, "k-mer table overflow: call covest_kmer_reserve with more slots");
    if (flag[kKmerUnderflowWord])
        return fail(COVEST_E_INVALID, kmer_underflow_text(who));
    return COVEST_OK;
}

int KmerHostCall::close(const char *reader)
{
    HIP_TRY(hipDeviceSynchronize());
    int flag[kKmerStickyWords] = {0, 0};
    HIP_TRY(hipMemcpy(flag, c->flag.ptr, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag[kKmerOverflowWord])
        return fail(COVEST_E_NOMEM, std::string(reader) + ": k-mer table overflow, the counts are partial: "
                                                          "covest_kmer_clear and recount with more slots");
    return !flag[kKmerUnderflowWord] ? COVEST_OK : fail(COVEST_E_INVALID, kmer_underflow_text(reader));
}

std::string kmer_underflow_text(const char *who)
{
    return std::string(who) + ": k-mer table underflow, a removal took out more than the table held and the counts are "
                              "unspecified: covest_kmer_clear and recount";
}

// a weight a read: there with the reads, and where a uint32 can lie
int kmer_check_weights(const char *who, const uint32_t *weights, int64_t n_reads)
{
    if (n_reads > 0 && !weights)
        return fail(COVEST_E_INVALID, std::string(who) + ": null weights");
    if (reinterpret_cast<uintptr_t>(weights) % alignof(uint32_t) != 0)
        return fail(COVEST_E_INVALID, std::string(who) + ": the weights must be aligned to 4 bytes");
    return COVEST_OK;
}

// covest_kmer_reserve's rehash (into a table of more slots) and covest_kmer_compact's (abi_remove.cpp: into one of as
// many): a fresh table of at least min_slots slots takes the counter's place; the keys HELD travel, by table_add, keys whose count
// a removal brought to 0 stay behind (kmer_table.h).  The counter's lock is held and its device is current.
int kmer_rehash_locked(covest_kmer *c, int64_t min_slots, const char *who)
{
    // An overflow of an earlier covest_kmer_add_device (asynchronous: it never looks at the flag itself) is STICKY
    // until covest_kmer_clear: its batch is partly counted, and a rehash of a table with k-mers missing must not make
    // the next covest_kmer_histogram look clean; an underflow of a removal likewise.  So: everything in flight on this
    // device first (the adds may run on a caller's non-blocking stream, the rehash runs on the null stream), then the
    // flags.
    HIP_TRY(hipDeviceSynchronize());
    COVEST_TRY(kmer_check_overflow(c, who));
    KmerTable bigger{};
    KmerWideTable wbigger{};
    DevBuf slots;
    int rc = table_alloc(c, min_slots, bigger, wbigger, slots);
    hipError_t e = hipSuccess;
    if (rc == COVEST_OK) { // (the flags are known to be clean here: whatever they hold afterwards is the rehash's)
        e = table_rehash(c, bigger, wbigger);
        if (e == hipSuccess)
            e = hipDeviceSynchronize();
        if (e != hipSuccess)
            rc = fail_hip(e, (std::string(who) + ": rehash").c_str());
    }
    if (rc != COVEST_OK)
        return rc; // (the new table goes with `slots`)
    c->slots = std::move(slots);
    c->table = bigger;
    c->wtable = wbigger;
    return kmer_check_overflow(c, who);
}

} // namespace covest

extern "C" {

int covest_kmer_create(int32_t k, int32_t canonical, int64_t min_slots, int32_t device, covest_kmer **out)
{
    if (!out)
        return fail(COVEST_E_INVALID, "covest_kmer_create: null argument");
    *out = nullptr;
    if (k < 1 || k > 255)
        return fail(COVEST_E_INVALID, "covest_kmer_create: k must be in 1..255 (keys of up to eight 64-bit words)");
    {
        const int drc = resolve_device(device, "covest_kmer_create", &device);
        if (drc != COVEST_OK)
            return drc;
    }
    covest_kmer *c = new (std::nothrow) covest_kmer();
    if (!c)
        return fail(COVEST_E_NOMEM, "covest_kmer_create: out of host memory");
    c->device = device;
    c->k = k;
    c->canonical = canonical != 0;
    c->wide = kmer_plan::kmer_wide_words(k);
    DeviceGuard dev_guard(device);
    hipError_t e = hipSuccess;
    int rc = dev_guard.status();
    if (rc == COVEST_OK)
        rc = table_alloc(c, min_slots, c->table, c->wtable, c->slots);
    if (rc == COVEST_OK) {
        e = c->flag.reserve(kKmerStickyWords * sizeof(int));
        if (e == hipSuccess)
            e = hipMemset(c->flag.ptr, 0, kKmerStickyWords * sizeof(int));
        if (e == hipSuccess)
            e = c->stats.reserve(kKmerStatsWords * sizeof(unsigned long long));
        if (e != hipSuccess)
            rc = fail_hip(e, "covest_kmer_create: allocation");
    }
    if (rc != COVEST_OK) {
        covest_kmer_destroy(c);
        return rc;
    }
    *out = c;
    return COVEST_OK;
}

void covest_kmer_destroy(covest_kmer *c)
{
    if (!c)
        return;
    DeviceGuard dev_guard(c->device);
    for (hipEvent_t &e : c->part.ev)
        if (e) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
    (void)hipDeviceSynchronize();
    delete c; // (its buffers go with it: host.h DevBuf)
}

int64_t covest_kmer_slots(const covest_kmer *c)
{
    return c ? slots_of(c) : COVEST_E_INVALID;
}

int covest_kmer_clear(covest_kmer *c, void *stream)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_clear: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    HIP_TRY(table_clear(c, static_cast<hipStream_t>(stream)));
    HIP_TRY(hipMemsetAsync(c->flag.ptr, 0, kKmerStickyWords * sizeof(int), static_cast<hipStream_t>(stream)));
    // what the partitioned path kept for its next call -- the buckets' records are gigabytes -- goes with the counts,
    // whether its last call succeeded or not (a call that failed after its reserve left `bulk` false and the records
    // allocated: the table path the caller falls back to needs that memory).  covest_kmer_count_reads_device has
    // returned, and hipFree waits for the device: nothing of it is in flight
    if (c->part.recs.ptr || c->part.ovf.ptr)
        (void)hipDeviceSynchronize();
    c->part.recs.release();
    c->part.ovf.release();
    c->bulk = false;
    return COVEST_OK;
}

int covest_kmer_memory_limit(covest_kmer *c, int64_t max_bytes)
{
    if (!c || max_bytes < 0)
        return fail(COVEST_E_INVALID, "covest_kmer_memory_limit: bad argument");
    std::lock_guard<std::mutex> guard(c->lock);
    c->part.mem_limit = max_bytes;
    return COVEST_OK;
}

int covest_kmer_reserve(covest_kmer *c, int64_t min_slots)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_reserve: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    if (slots_of(c) >= min_slots)
        return COVEST_OK;
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    return kmer_rehash_locked(c, min_slots, "covest_kmer_reserve");
}

int covest_kmer_histogram(covest_kmer *c, int64_t *out, int64_t out_len, int64_t *needed_len,
                          int64_t *distinct)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_histogram: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    HIP_TRY(hipDeviceSynchronize());
    int rc = kmer_check_overflow(c, "covest_kmer_histogram");
    if (rc != COVEST_OK)
        return rc;
    unsigned long long stats[kKmerStatsWords] = {0, 0, 0}; // (max count, keys held; the slots occupied: abi_remove.cpp)
    const bool table_in_use = !c->bulk || c->part.table_used; // (a partitioned count may leave nothing in the table)
    if (table_in_use) {
        HIP_TRY(hipMemset(c->stats.ptr, 0, sizeof(stats)));
        HIP_TRY(table_scan(c, 0));
        HIP_TRY(hipMemcpy(stats, c->stats.ptr, sizeof(stats), hipMemcpyDeviceToHost));
    }
    // (after covest_kmer_count_reads_device the table holds only what the partitioned path handed back; the rest of
    // the keys were counted in LDS, and what is left of them is their count-of-counts)
    std::vector<unsigned long long> big;
    if (c->bulk) {
        stats[0] = std::max(stats[0], c->part.stats[0]);
        stats[1] += c->part.stats[1];
        if (c->part.stats[2] > 0) {
            big.resize((size_t)c->part.stats[2]);
            HIP_TRY(hipMemcpy(big.data(), c->part.big.ptr, big.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        }
    }
    const int64_t need = (int64_t)stats[0] + 1; // index 0 .. max count (bin/kmer_hist.py:64)
    if (needed_len)
        *needed_len = need;
    if (distinct)
        *distinct = (int64_t)stats[1];
    if (!out)
        return COVEST_OK;
    if (out_len < need)
        return fail(COVEST_E_INVALID, "covest_kmer_histogram: output shorter than max count + 1");
    HIP_TRY(c->hist.reserve((size_t)need * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(c->hist.ptr, 0, (size_t)need * sizeof(unsigned long long)));
    if (table_in_use)
        HIP_TRY(table_scan(c, (unsigned long long)need));
    HIP_TRY(hipMemcpy(out, c->hist.ptr, (size_t)need * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (c->bulk) {
        const size_t n_dense = (size_t)std::min<unsigned long long>((unsigned long long)need, kBulkHistLen);
        std::vector<unsigned long long> dense(n_dense);
        HIP_TRY(hipMemcpy(dense.data(), c->part.hist.ptr, n_dense * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_dense; ++i)
            out[i] += (int64_t)dense[i];
        for (unsigned long long v : big)
            if ((int64_t)v < need)
                out[v] += 1;
    }
    return COVEST_OK;
}

// The whole counting loop of bin/kmer_hist.py:77-89 for reads resident in HBM, by the partitioned path
// (kmer_bulk.hip).  See include/covest_amd.h.
int covest_kmer_count_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                   int64_t read_len, int64_t n_bases_total, void *stream)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !d_bases) || (!d_offsets && read_len < 0))
        return fail(COVEST_E_INVALID, "covest_kmer_count_reads_device: bad argument");
    if (c->wide || c->k < 19 || c->k > 31)
        return fail(COVEST_E_UNSUPPORTED, "covest_kmer_count_reads_device: the partitioned path takes k = 19 .. 31 "
                                          "(use covest_kmer_add_device)");
    if (!d_offsets && (read_len < c->k || read_len >= ((int64_t)1 << 30)))
        return fail(COVEST_E_UNSUPPORTED, "covest_kmer_count_reads_device: reads shorter than k, or of 2^30 bases and more "
                                          "(use covest_kmer_add_device)");
    std::lock_guard<std::mutex> guard(c->lock);
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    BulkCall b{c, static_cast<hipStream_t>(stream), d_bases, d_offsets, n_reads, read_len, n_bases_total};
    COVEST_TRY(resolve_layout(b));
    plan_call(b);
    COVEST_TRY(reserve_buffers(b));
    COVEST_TRY(pass0_and_room(b));
    COVEST_TRY(reserve_records(b));
    COVEST_TRY(scatter_and_count(b));
    COVEST_TRY(read_back(b));
    COVEST_TRY(hand_back(b));
    return finish(b);
}

int covest_kmer_partition_info(const covest_kmer *c, int64_t out[8])
{
    if (!c || !out)
        return fail(COVEST_E_INVALID, "covest_kmer_partition_info: bad argument");
    if (!c->bulk)
        return fail(COVEST_E_INVALID, "covest_kmer_partition_info: the counter holds no covest_kmer_count_reads_device result");
    for (int i = 0; i < 5; ++i)
        out[i] = c->part.info[i];
    out[5] = (int64_t)c->part.later_n;
    out[6] = (int64_t)c->part.to_table_n;
    out[7] = (int64_t)c->part.stats[3];
    return COVEST_OK;
}

int covest_kmer_partition_ms(const covest_kmer *c, double out[4])
{
    if (!c || !out)
        return fail(COVEST_E_INVALID, "covest_kmer_partition_ms: bad argument");
    if (!c->bulk)
        return fail(COVEST_E_INVALID, "covest_kmer_partition_ms: the counter holds no covest_kmer_count_reads_device result");
    for (int i = 0; i < 4; ++i)
        out[i] = (double)c->part.ms[i];
    return COVEST_OK;
}

int covest_kmer_scatter_rate(int32_t device, int64_t slots, int64_t ops, double *ops_per_s)
{
    if (slots < 1 || ops < 1 || !ops_per_s)
        return fail(COVEST_E_INVALID, "covest_kmer_scatter_rate: bad argument");
    DeviceCall call(device, "covest_kmer_scatter_rate");
    COVEST_TRY(call.status());
    DevBuf words;
    HIP_TRY(words.reserve(((size_t)slots + 1) * sizeof(unsigned long long)));
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipMemset(words.ptr, 0, ((size_t)slots + 1) * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipEventCreate(&a);
    if (e == hipSuccess)
        e = hipEventCreate(&b);
    unsigned long long *w = words.as<unsigned long long>();
    if (e == hipSuccess) // (once untimed: the pages are touched, the clocks are up)
        e = launch_kmer_scatter_rate(w, (unsigned long long)slots, std::min<int64_t>(ops, 1 << 24), w + slots, nullptr);
    if (e == hipSuccess)
        e = hipEventRecord(a, nullptr);
    if (e == hipSuccess)
        e = launch_kmer_scatter_rate(w, (unsigned long long)slots, ops, w + slots, nullptr);
    if (e == hipSuccess)
        e = hipEventRecord(b, nullptr);
    if (e == hipSuccess)
        e = hipEventSynchronize(b);
    float ms = 0.0f;
    if (e == hipSuccess)
        e = hipEventElapsedTime(&ms, a, b);
    if (a)
        (void)hipEventDestroy(a);
    if (b)
        (void)hipEventDestroy(b);
    if (e != hipSuccess)
        return fail_hip(e, "covest_kmer_scatter_rate");
    const double done = (double)(((ops + 63) / 64) * 64);
    *ops_per_s = done / ((double)ms * 1e-3);
    return COVEST_OK;
}

} // extern "C"
