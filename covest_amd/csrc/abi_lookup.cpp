// abi_lookup.cpp -- covest_kmer_lookup_reads* of the C ABI over kmer_lookup.hip: per-read k-mer abundances, summaries
// and scores against the counter's table.  Nothing here, or below it, writes to the table.
#include "host.h"
#include "kmer_lookup.h"

using namespace covest;

namespace {

// The checks both forms share (the counter's lock is held).
int check_lookup(const char *who, const covest_kmer *c, int64_t n_reads, int64_t read_len, bool has_offsets,
                 const void *weights, int32_t n_weights, const void *abundance, const void *summary, const void *score)
{
    const std::string name(who);
    if (n_reads < 0 || (!has_offsets && (read_len < 0 || read_len >= ((int64_t)1 << 32))))
        return fail(COVEST_E_INVALID, name + ": negative size, or no offsets and no read_len below 2^32");
    if (score && (!weights || n_weights < 1))
        return fail(COVEST_E_INVALID, name + ": a score needs a table of at least one weight");
    if ((uintptr_t)abundance % alignof(uint32_t) || (uintptr_t)summary % (4 * sizeof(uint32_t)) ||
        (uintptr_t)score % alignof(double) || (uintptr_t)weights % alignof(double))
        return fail(COVEST_E_INVALID, name + ": an output is not naturally aligned (summary: rows of 16 bytes)");
    if (c->wide)
        return fail(COVEST_E_UNSUPPORTED, name + ": k must be at most 31 (keys of one word)");
    if (c->bulk)
        return fail(COVEST_E_INVALID, name + ": the counter holds a covest_kmer_count_reads_device result "
                                             "(its keys are not in the table); covest_kmer_clear first");
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
    COVEST_TRY(check_lookup("covest_kmer_lookup_reads_device", c, n_reads, read_len, d_offsets != nullptr, d_weights,
                            n_weights, d_abundance, d_summary, d_score));
    if (n_reads == 0)
        return COVEST_OK;
    if (!d_bases)
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads_device: null bases");
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    HIP_TRY(launch_kmer_lookup(d_bases, d_offsets, n_reads, read_len, c->canonical, c->table, cutoff, d_weights, n_weights,
                               d_abundance, d_summary, d_score, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_kmer_lookup_reads(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                             uint32_t cutoff, const double *weights, int32_t n_weights, uint32_t *abundance,
                             uint32_t *summary, double *score)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: bad argument");
    if (score && (!weights || n_weights < 1))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: a score needs a table of at least one weight");
    if (c->wide)
        return fail(COVEST_E_UNSUPPORTED, "covest_kmer_lookup_reads: k must be at most 31 (keys of one word)");
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases))
        return fail(COVEST_E_INVALID, "covest_kmer_lookup_reads: bad offsets");
    DeviceGuard dev_guard(c->device);
    if (dev_guard.status() != COVEST_OK)
        return dev_guard.status();
    const size_t n_pos = (size_t)n_bytes, n = (size_t)n_reads;
    DevBuf d_weights, d_abundance, d_summary, d_score; // (go with the call; the copies back have waited for the kernel)
    COVEST_TRY(stage_reads_in_counter(c, bases, offsets, n_reads));
    if (score) {
        HIP_TRY(d_weights.reserve((size_t)n_weights * sizeof(double)));
        HIP_TRY(hipMemcpy(d_weights.ptr, weights, (size_t)n_weights * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(d_score.reserve(n * sizeof(double)));
    }
    if (abundance)
        HIP_TRY(d_abundance.reserve(std::max<size_t>(n_pos, 1) * sizeof(uint32_t)));
    if (summary)
        HIP_TRY(d_summary.reserve(n * 4 * sizeof(uint32_t)));
    COVEST_TRY(covest_kmer_lookup_reads_device(c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0, cutoff,
                                               score ? d_weights.as<double>() : nullptr, score ? n_weights : 0,
                                               abundance ? d_abundance.as<uint32_t>() : nullptr,
                                               summary ? d_summary.as<uint32_t>() : nullptr,
                                               score ? d_score.as<double>() : nullptr, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    COVEST_TRY(kmer_check_partial(c, "covest_kmer_lookup_reads"));
    if (abundance && n_pos)
        HIP_TRY(hipMemcpy(abundance, d_abundance.ptr, n_pos * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (summary)
        HIP_TRY(hipMemcpy(summary, d_summary.ptr, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (score)
        HIP_TRY(hipMemcpy(score, d_score.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
