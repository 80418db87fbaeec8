// abi_remove.cpp -- covest_kmer_occupancy and covest_kmer_compact of the C ABI over the scans of kmer_count.hip: what a
// removal leaves in the one-word table, measured and let go.  The removals themselves:
// abi_update.cpp.
#include "host.h"

using namespace covest;

extern "C" {

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
