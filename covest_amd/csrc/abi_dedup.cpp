// abi_dedup.cpp -- covest_dedup_reads* of the C ABI over dedup_reads.hip: duplicate reads removed, the first copy kept
// (DESIGN.md section 6al).  No handle: the device form launches on the caller's stream and returns; the host form owns
// its device buffers for the call.
#include "call_scratch.h"
#include "dedup.h"
#include "host.h"

using namespace covest;

namespace {

// The checks both forms share.
int check_dedup_args(const char *who, const void *offsets, int64_t n_reads, int64_t read_len, int64_t first_read,
                     int32_t fp_bits, const void *out_offsets)
{
    const std::string name(who);
    if (fp_bits < 1 || fp_bits > 63)
        return fail(COVEST_E_INVALID, name + ": fp_bits must be within 1 .. 63");
    return fail_if(check_reads_args(name, offsets != nullptr, n_reads, read_len, first_read, out_offsets != nullptr));
}

} // namespace

extern "C" {

int covest_dedup_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, int64_t first_read, int32_t reverse_complement, int32_t fp_bits,
                              uint64_t seed, uint8_t *d_out_bases, int64_t *d_out_offsets, int64_t *d_kept_index,
                              int32_t *d_copies, int64_t *d_counts, void *stream)
{
    COVEST_TRY(check_dedup_args("covest_dedup_reads_device", d_offsets, n_reads, read_len, first_read, fp_bits, d_out_offsets));
    if (!d_counts)
        return fail(COVEST_E_INVALID, "covest_dedup_reads_device: d_counts is null");
    DeviceCall call(device, "covest_dedup_reads_device");
    COVEST_TRY(call.status());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_reads == 0) { // nothing launched: the counts, and the one output offset there is, by a memset on the stream
        HIP_TRY(hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), st));
        if (d_out_offsets)
            HIP_TRY(hipMemsetAsync(d_out_offsets, 0, sizeof(int64_t), st));
        return COVEST_OK;
    }
    CallScratch *scratch = nullptr; // (call_scratch.h: the call returns before its kernels have run)
    COVEST_TRY(call_scratch_take(call.device(), dedup_scratch_bytes(n_reads), "scratch of covest_dedup_reads_device", &scratch));
    const hipError_t e = launch_dedup_reads(d_bases, d_offsets, n_reads, read_len, first_read, reverse_complement, fp_bits, seed,
                                            d_out_bases, d_out_offsets, d_kept_index, d_copies, d_counts, scratch->buf.ptr, st);
    call_scratch_give(scratch, st); // (whatever was launched before a failure still works on the block)
    HIP_TRY(e);
    return COVEST_OK;
}

int covest_dedup_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                       int64_t first_read, int32_t reverse_complement, int32_t fp_bits, uint64_t seed, uint8_t *out_bases,
                       int64_t *out_offsets, int64_t *kept_index, int32_t *copies, int64_t *n_kept, int64_t *bases_kept,
                       int64_t *n_collided)
{
    COVEST_TRY(check_dedup_args("covest_dedup_reads", offsets, n_reads, read_len, first_read, fp_bits, out_offsets));
    if (!n_kept || !bases_kept || !n_collided)
        return fail(COVEST_E_INVALID, "covest_dedup_reads: n_kept, bases_kept and n_collided must not be null");
    COVEST_TRY(fail_if(check_ascending_offsets("covest_dedup_reads", offsets, n_reads)));
    const int64_t end_byte = offsets ? offsets[n_reads] : n_reads * read_len; // (the bases are copied from byte 0)
    if (n_reads > 0 && end_byte > 0 && (!bases || !out_bases))
        return fail(COVEST_E_INVALID, "covest_dedup_reads: null buffer");
    *n_kept = *bases_kept = *n_collided = 0;
    if (n_reads == 0) {
        if (out_offsets)
            out_offsets[0] = 0;
        return COVEST_OK;
    }
    DeviceCall call(device, "covest_dedup_reads");
    COVEST_TRY(call.status());
    ReadsStage stage; // (goes with the call, on every path, as the three below; the copies back have waited for the kernels)
    DevBuf d_counts, d_copies, d_scratch;
    COVEST_TRY(stage.upload(bases, offsets, n_reads, (size_t)end_byte, out_offsets != nullptr, kept_index != nullptr));
    HIP_TRY(d_counts.reserve(3 * sizeof(int64_t)));
    if (copies)
        HIP_TRY(d_copies.reserve((size_t)n_reads * sizeof(int32_t)));
    HIP_TRY(d_scratch.reserve(dedup_scratch_bytes(n_reads)));
    HIP_TRY(launch_dedup_reads(stage.d_bases.as<uint8_t>(), stage.d_offsets.as<int64_t>(), n_reads, read_len, first_read,
                               reverse_complement, fp_bits, seed, stage.d_out_bases.as<uint8_t>(),
                               stage.d_out_offsets.as<int64_t>(), stage.d_index.as<int64_t>(), d_copies.as<int32_t>(),
                               d_counts.as<int64_t>(), d_scratch.ptr, nullptr));
    int64_t counts[3] = {0, 0, 0};
    HIP_TRY(hipMemcpy(counts, d_counts.ptr, sizeof(counts), hipMemcpyDeviceToHost));
    COVEST_TRY(stage.download(out_bases, (size_t)counts[1], out_offsets, (size_t)(counts[0] + 1), kept_index, (size_t)counts[0]));
    if (copies && counts[0])
        HIP_TRY(hipMemcpy(copies, d_copies.ptr, (size_t)counts[0] * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_kept = counts[0];
    *bases_kept = counts[1];
    *n_collided = counts[2];
    return COVEST_OK;
}

} // extern "C"
