// abi_lookup.cpp -- covest_kmer_lookup_reads* of the C ABI over kmer_lookup.hip: per-read k-mer abundances, summaries
// and scores against the counter's table.  Nothing here, or below it, writes to the table.
#include "host.h"
#include "kmer_lookup.h"

using namespace covest;

namespace {

int lookup_locked(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads, int64_t read_len,
                  uint32_t cutoff, const double *d_weights, int32_t n_weights, uint32_t *d_abundance, uint32_t *d_summary,
                  double *d_score, void *stream)
{
    const std::string name("covest_kmer_lookup_reads_device");
    COVEST_TRY(fail_if(check_table_reads_sizes(name, d_offsets != nullptr, n_reads, read_len)));
    if (d_score && (!d_weights || n_weights < 1))
        return fail(COVEST_E_INVALID, name + ": a score needs a table of at least one weight");
    if ((uintptr_t)d_abundance % alignof(uint32_t) || (uintptr_t)d_summary % (4 * sizeof(uint32_t)) ||
        (uintptr_t)d_score % alignof(double) || (uintptr_t)d_weights % alignof(double))
        return fail(COVEST_E_INVALID, name + ": an output is not naturally aligned (summary: rows of 16 bytes)");
    COVEST_TRY(fail_if(check_table_holds_keys(name, c->wide, c->bulk)));
    if (n_reads == 0)
        return COVEST_OK;
    if (!d_bases)
        return fail(COVEST_E_INVALID, name + ": null bases");
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(launch_kmer_lookup(d_bases, d_offsets, n_reads, read_len, c->canonical, c->table, cutoff, d_weights, n_weights,
                               d_abundance, d_summary, d_score, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_kmer_lookup_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                    int64_t read_len, uint32_t cutoff, const double *d_weights, int32_t n_weights,
                                    uint32_t *d_abundance, uint32_t *d_summary, double *d_score, void *stream)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads_device: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    return lookup_locked(c, d_bases, d_offsets, n_reads, read_len, cutoff, d_weights, n_weights, d_abundance, d_summary,
                         d_score, stream);
}

int covest_kmer_lookup_reads(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                             uint32_t cutoff, const double *weights, int32_t n_weights, uint32_t *abundance,
                             uint32_t *summary, double *score)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: bad argument");
    if (score && (!weights || n_weights < 1))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: a score needs a table of at least one weight");
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_lookup_reads", c->wide, false))); // (bulk: the device form's)
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: bad offsets");
    const size_t n_pos = (size_t)n_bytes, n = (size_t)n_reads;
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    DevBuf d_weights, d_abundance, d_summary, d_score; // (go with the call; the copies back have waited for the kernel)
    if (score) {
        HIP_TRY(d_weights.reserve((size_t)n_weights * sizeof(double)));
        HIP_TRY(hipMemcpy(d_weights.ptr, weights, (size_t)n_weights * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(d_score.reserve(n * sizeof(double)));
    }
    if (abundance)
        HIP_TRY(d_abundance.reserve(std::max<size_t>(n_pos, 1) * sizeof(uint32_t)));
    if (summary)
        HIP_TRY(d_summary.reserve(n * 4 * sizeof(uint32_t)));
    COVEST_TRY(lookup_locked(c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0, cutoff,
                             score ? d_weights.as<double>() : nullptr, score ? n_weights : 0,
                             abundance ? d_abundance.as<uint32_t>() : nullptr, summary ? d_summary.as<uint32_t>() : nullptr,
                             score ? d_score.as<double>() : nullptr, nullptr));
    COVEST_TRY(call.close("covest_kmer_lookup_reads"));
    if (abundance && n_pos)
        HIP_TRY(hipMemcpy(abundance, d_abundance.ptr, n_pos * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (summary)
        HIP_TRY(hipMemcpy(summary, d_summary.ptr, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (score)
        HIP_TRY(hipMemcpy(score, d_score.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
