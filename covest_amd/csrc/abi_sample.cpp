// abi_sample.cpp -- covest_sample_reads* of the C ABI over sample_reads.hip: the counterpart of the reference's
// covest/data.py:57-63 sample_reads.  No handle: the device form launches on the caller's stream
// and returns; the host form owns its device buffers for the call.
#include "call_scratch.h"
#include "host.h"
#include "sample.h"

using namespace covest;

namespace {

// The checks both forms share; *thr = floor((1 / factor) * 2^32) (2^32 at factor 1: every read is kept).
int check_sample_args(const char *who, const void *offsets, int64_t n_reads, int64_t read_len, int64_t first_read,
                      double factor, const void *out_offsets, uint64_t *thr)
{
    const std::string name(who);
    if (!(factor >= 1.0) || !std::isfinite(factor)) // (NaN fails the first)
        return fail(COVEST_E_INVALID, name + ": factor must be a finite number, at least 1");
    if (n_reads < 0 || first_read < 0)
        return fail(COVEST_E_INVALID, name + ": n_reads and first_read must not be negative");
    if (!offsets && read_len < 0)
        return fail(COVEST_E_INVALID, name + ": without offsets read_len must not be negative");
    const int64_t i64_max = std::numeric_limits<int64_t>::max();
    if (first_read > i64_max - n_reads || (!offsets && read_len > 0 && n_reads > i64_max / read_len))
        return fail(COVEST_E_INVALID, name + ": more reads than 64-bit offsets reach");
    if (n_reads > 0 && offsets && !out_offsets)
        return fail(COVEST_E_INVALID, name + ": reads of their own lengths need an array for the output offsets");
    *thr = (uint64_t)std::floor((1.0 / factor) * 4294967296.0);
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_sample_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                               int64_t read_len, int64_t first_read, double factor, uint64_t seed, uint8_t *d_out_bases,
                               int64_t *d_out_offsets, int64_t *d_kept_index, int64_t *d_counts, void *stream)
{
    uint64_t thr = 0;
    COVEST_TRY(check_sample_args("covest_sample_reads_device", d_offsets, n_reads, read_len, first_read, factor,
                                 d_out_offsets, &thr));
    if (!d_counts)
        return fail(COVEST_E_INVALID, "covest_sample_reads_device: d_counts is null");
    DeviceCall call(device, "covest_sample_reads_device");
    COVEST_TRY(call.status());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_reads == 0) { // nothing launched: the counts, and the one output offset there is, by a memset on the stream
        HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), st));
        if (d_out_offsets)
            HIP_TRY(hipMemsetAsync(d_out_offsets, 0, sizeof(int64_t), st));
        return COVEST_OK;
    }
    CallScratch *scratch = nullptr; // (call_scratch.h: the call returns before its kernels have run)
    COVEST_TRY(call_scratch_take(call.device(), sample_scratch_bytes(n_reads), "scratch of covest_sample_reads_device", &scratch));
    const hipError_t e = launch_sample_reads(d_bases, d_offsets, n_reads, read_len, first_read, thr, seed, d_out_bases,
                                             d_out_offsets, d_kept_index, d_counts, scratch->buf.ptr, st);
    call_scratch_give(scratch, st); // (whatever was launched before a failure still works on the block)
    HIP_TRY(e);
    return COVEST_OK;
}

int covest_sample_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                        int64_t first_read, double factor, uint64_t seed, uint8_t *out_bases, int64_t *out_offsets,
                        int64_t *kept_index, int64_t *n_kept, int64_t *bases_kept)
{
    uint64_t thr = 0;
    COVEST_TRY(check_sample_args("covest_sample_reads", offsets, n_reads, read_len, first_read, factor, out_offsets, &thr));
    if (!n_kept || !bases_kept)
        return fail(COVEST_E_INVALID, "covest_sample_reads: n_kept and bases_kept must not be null");
    if (offsets) {
        if (offsets[0] < 0)
            return fail(COVEST_E_INVALID, "covest_sample_reads: negative offset");
        for (int64_t i = 0; i < n_reads; ++i)
            if (offsets[i + 1] < offsets[i])
                return fail(COVEST_E_INVALID, "covest_sample_reads: offsets descend at read " + std::to_string(i));
    }
    const int64_t end_byte = offsets ? offsets[n_reads] : n_reads * read_len; // (the bases are copied from byte 0)
    if (n_reads > 0 && end_byte > 0 && (!bases || !out_bases))
        return fail(COVEST_E_INVALID, "covest_sample_reads: null buffer");
    *n_kept = *bases_kept = 0;
    if (n_reads == 0) {
        if (out_offsets)
            out_offsets[0] = 0;
        return COVEST_OK;
    }
    DeviceCall call(device, "covest_sample_reads");
    COVEST_TRY(call.status());
    const size_t n_bytes = (size_t)end_byte, index_bytes = (size_t)n_reads * sizeof(int64_t);
    // (go with the call, on every path; the copies back have waited for the kernels)
    DevBuf d_bases, d_offsets, d_out_bases, d_out_offsets, d_kept, d_counts, d_scratch;
    HIP_TRY(d_bases.reserve(std::max<size_t>(n_bytes, 16)));
    HIP_TRY(d_out_bases.reserve(std::max<size_t>(n_bytes, 16)));
    if (offsets)
        HIP_TRY(d_offsets.reserve(index_bytes + sizeof(int64_t)));
    if (out_offsets)
        HIP_TRY(d_out_offsets.reserve(index_bytes + sizeof(int64_t)));
    if (kept_index)
        HIP_TRY(d_kept.reserve(index_bytes));
    HIP_TRY(d_counts.reserve(2 * sizeof(int64_t)));
    HIP_TRY(d_scratch.reserve(sample_scratch_bytes(n_reads)));
    if (n_bytes)
        HIP_TRY(hipMemcpy(d_bases.ptr, bases, n_bytes, hipMemcpyHostToDevice));
    if (offsets)
        HIP_TRY(hipMemcpy(d_offsets.ptr, offsets, index_bytes + sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(launch_sample_reads(d_bases.as<uint8_t>(), offsets ? d_offsets.as<int64_t>() : nullptr, n_reads,
                                read_len, first_read, thr, seed, d_out_bases.as<uint8_t>(),
                                out_offsets ? d_out_offsets.as<int64_t>() : nullptr,
                                kept_index ? d_kept.as<int64_t>() : nullptr, d_counts.as<int64_t>(), d_scratch.ptr,
                                nullptr));
    int64_t counts[2] = {0, 0};
    HIP_TRY(hipMemcpy(counts, d_counts.ptr, sizeof(counts), hipMemcpyDeviceToHost));
    if (counts[1] > 0)
        HIP_TRY(hipMemcpy(out_bases, d_out_bases.ptr, (size_t)counts[1], hipMemcpyDeviceToHost));
    if (out_offsets)
        HIP_TRY(hipMemcpy(out_offsets, d_out_offsets.ptr, (size_t)(counts[0] + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (kept_index && counts[0] > 0)
        HIP_TRY(hipMemcpy(kept_index, d_kept.ptr, (size_t)counts[0] * sizeof(int64_t), hipMemcpyDeviceToHost));
    *n_kept = counts[0];
    *bases_kept = counts[1];
    return COVEST_OK;
}

} // extern "C"
