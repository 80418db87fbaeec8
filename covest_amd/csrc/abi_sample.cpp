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
    COVEST_TRY(fail_if(check_reads_args(name, offsets != nullptr, n_reads, read_len, first_read, out_offsets != nullptr)));
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
    COVEST_TRY(fail_if(check_ascending_offsets("covest_sample_reads", offsets, n_reads)));
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
    ReadsStage stage; // (goes with the call, on every path, as the two below; the copies back have waited for the kernels)
    DevBuf d_counts, d_scratch;
    COVEST_TRY(stage.upload(bases, offsets, n_reads, (size_t)end_byte, out_offsets != nullptr, kept_index != nullptr));
    HIP_TRY(d_counts.reserve(2 * sizeof(int64_t)));
    HIP_TRY(d_scratch.reserve(sample_scratch_bytes(n_reads)));
    HIP_TRY(launch_sample_reads(stage.d_bases.as<uint8_t>(), stage.d_offsets.as<int64_t>(), n_reads, read_len, first_read,
                                thr, seed, stage.d_out_bases.as<uint8_t>(), stage.d_out_offsets.as<int64_t>(),
                                stage.d_index.as<int64_t>(), d_counts.as<int64_t>(), d_scratch.ptr, nullptr));
    int64_t counts[2] = {0, 0};
    HIP_TRY(hipMemcpy(counts, d_counts.ptr, sizeof(counts), hipMemcpyDeviceToHost));
    COVEST_TRY(stage.download(out_bases, (size_t)counts[1], out_offsets, (size_t)(counts[0] + 1), kept_index, (size_t)counts[0]));
    *n_kept = counts[0];
    *bases_kept = counts[1];
    return COVEST_OK;
}

} // extern "C"
