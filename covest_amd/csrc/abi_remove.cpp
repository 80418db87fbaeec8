// abi_remove.cpp -- covest_kmer_remove*, covest_kmer_occupancy and covest_kmer_compact of the C ABI over kmer_remove.hip
// and the scans of kmer_count.hip: counts taken back out of the one-word table.  Arguments,
// lock, device guard, staging and weight checks are those of the four add forms (kmer_host.cpp).
#include "host.h"

using namespace covest;

namespace {

// covest_kmer_remove_device (d_weights null) and covest_kmer_remove_weighted_device with the counter's lock held (the
// host forms hold it for their whole call: host.h KmerHostCall)
int remove_device_locked(const char *who, covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                         int64_t read_len, const uint32_t *d_weights, void *stream)
{
    COVEST_TRY(fail_if(check_table_holds_keys(who, c->wide, c->bulk)));
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(launch_kmer_remove(d_bases, d_offsets, n_reads, read_len, c->k, c->canonical, c->table,
                               c->flag.as<int>() + kKmerUnderflowWord, static_cast<hipStream_t>(stream), d_weights));
    return COVEST_OK;
}

// a host form behind its staging: the removal, the wait, and the underflow it may have met itself
int remove_host_locked(const char *who, covest_kmer *c, int64_t n_reads, const uint32_t *d_weights)
{
    COVEST_TRY(remove_device_locked(who, c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0, d_weights,
                                    nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return kmer_check_overflow(c, who);
}

} // namespace

extern "C" {

int covest_kmer_remove_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, void *stream)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !d_bases) || (!d_offsets && read_len < 0))
        return fail(COVEST_E_INVALID, "covest_kmer_remove_device: bad argument");
    std::lock_guard<std::mutex> guard(c->lock);
    return remove_device_locked("covest_kmer_remove_device", c, d_bases, d_offsets, n_reads, read_len, nullptr, stream);
}

int covest_kmer_remove_weighted_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                       int64_t read_len, const uint32_t *d_weights, void *stream)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !d_bases) || (!d_offsets && read_len < 0))
        return fail(COVEST_E_INVALID, "covest_kmer_remove_weighted_device: bad argument");
    COVEST_TRY(kmer_check_weights("covest_kmer_remove_weighted_device", d_weights, n_reads));
    std::lock_guard<std::mutex> guard(c->lock);
    return remove_device_locked("covest_kmer_remove_weighted_device", c, d_bases, d_offsets, n_reads, read_len, d_weights,
                                stream);
}

int covest_kmer_remove(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_remove: bad argument");
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_remove", c->wide, false))); // (bulk: with the lock held)
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases))
        return fail(COVEST_E_INVALID, "covest_kmer_remove: bad offsets");
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    return remove_host_locked("covest_kmer_remove", c, n_reads, nullptr);
}

int covest_kmer_remove_weighted(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                                const uint32_t *weights)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_remove_weighted: bad argument");
    COVEST_TRY(kmer_check_weights("covest_kmer_remove_weighted", weights, n_reads));
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_remove_weighted", c->wide, false)));
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases))
        return fail(COVEST_E_INVALID, "covest_kmer_remove_weighted: bad offsets");
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    HIP_TRY(c->ws_weights.reserve((size_t)n_reads * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(c->ws_weights.ptr, weights, (size_t)n_reads * sizeof(uint32_t), hipMemcpyHostToDevice));
    return remove_host_locked("covest_kmer_remove_weighted", c, n_reads, c->ws_weights.as<uint32_t>());
}

int covest_kmer_occupancy(covest_kmer *c, int64_t out[2])
{
    if (!c || !out)
        return fail(COVEST_E_INVALID, "covest_kmer_occupancy: null argument");
    std::lock_guard<std::mutex> guard(c->lock);
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_occupancy", c->wide, c->bulk)));
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(hipDeviceSynchronize()); // the adds may run on a caller's non-blocking stream, the scan on the null stream
    unsigned long long stats[kKmerStatsWords] = {0, 0, 0};
    HIP_TRY(hipMemset(c->stats.ptr, 0, sizeof(stats)));
    HIP_TRY(launch_kmer_stats(c->table, c->stats.as<unsigned long long>(), nullptr));
    HIP_TRY(hipMemcpy(stats, c->stats.ptr, sizeof(stats), hipMemcpyDeviceToHost));
    out[0] = (int64_t)stats[1];
    out[1] = (int64_t)stats[2];
    return COVEST_OK;
}

int covest_kmer_compact(covest_kmer *c)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_compact: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_compact", c->wide, c->bulk)));
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    return kmer_rehash_locked(c, (int64_t)(c->table.mask + 1), "covest_kmer_compact");
}

} // extern "C"
