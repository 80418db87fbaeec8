// abi_correct.cpp -- covest_kmer_correct_reads* of the C ABI over kmer_correct.hip: isolated substitutions of reads
// corrected from the counter's table.  Nothing here, or below it, writes to the table.
#include "host.h"
#include "kmer_correct.h"

using namespace covest;

namespace {

int correct_locked(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads, int64_t read_len,
                   uint32_t cutoff, uint8_t *d_out, uint32_t *d_fix, void *stream)
{
    const std::string name("covest_kmer_correct_reads_device");
    COVEST_TRY(fail_if(check_table_reads_sizes(name, d_offsets != nullptr, n_reads, read_len)));
    if ((uintptr_t)d_fix % (4 * sizeof(uint32_t)))
        return fail(COVEST_E_INVALID, name + ": fix is not aligned to its rows of 16 bytes");
    COVEST_TRY(fail_if(check_table_holds_keys(name, c->wide, c->bulk)));
    if (n_reads == 0)
        return COVEST_OK;
    if (!d_bases || !d_out)
        return fail(COVEST_E_INVALID, name + ": null bases or null out");
    if (!d_offsets && d_out != d_bases) { // (with offsets the extent of the reads is on the device: not seen from here)
        const uintptr_t a = (uintptr_t)d_bases, b = (uintptr_t)d_out, n_bytes = (uintptr_t)n_reads * (uintptr_t)read_len;
        if (a < b + n_bytes && b < a + n_bytes)
            return fail(COVEST_E_INVALID, name + ": out overlaps the bases without being the bases (in place: out == bases)");
    }
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(launch_kmer_correct(d_bases, d_offsets, n_reads, read_len, c->canonical, c->table, cutoff, d_out, d_fix,
                                static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_kmer_correct_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                     int64_t read_len, uint32_t cutoff, uint8_t *d_out, uint32_t *d_fix, void *stream)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_correct_reads_device: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    return correct_locked(c, d_bases, d_offsets, n_reads, read_len, cutoff, d_out, d_fix, stream);
}

int covest_kmer_correct_reads(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                              uint32_t cutoff, uint8_t *out, uint32_t *fix)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_correct_reads: bad argument");
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_correct_reads", c->wide, false))); // (bulk: the device form's)
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases) || !out)
        return fail(COVEST_E_INVALID, "covest_kmer_correct_reads: bad offsets, or null bases or null out");
    const size_t n_pos = (size_t)n_bytes, n = (size_t)n_reads;
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    DevBuf d_fix; // (goes with the call; the copies back have waited for the kernel)
    if (fix)
        HIP_TRY(d_fix.reserve(n * 4 * sizeof(uint32_t)));
    // in place on the staged copy of the bases: only the corrected bytes are stored (the copy back is under the lock too)
    COVEST_TRY(correct_locked(c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0, cutoff,
                              c->ws_bases.as<uint8_t>(), fix ? d_fix.as<uint32_t>() : nullptr, nullptr));
    COVEST_TRY(call.close("covest_kmer_correct_reads"));
    if (n_pos)
        HIP_TRY(hipMemcpy(out, c->ws_bases.ptr, n_pos, hipMemcpyDeviceToHost));
    if (fix)
        HIP_TRY(hipMemcpy(fix, d_fix.ptr, n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
