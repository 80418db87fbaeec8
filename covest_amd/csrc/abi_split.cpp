// abi_split.cpp -- covest_split_reads* of the C ABI over split_reads.hip: the stable G-way split of the packed reads
// behind the delete-a-group jackknife.  No handle: the device form launches on the caller's
// stream and returns; the host form owns its device buffers for the call.
#include "call_scratch.h"
#include "host.h"
#include "split.h"

using namespace covest;

namespace {

// The checks both forms share.
int check_split_args(const char *who, const void *offsets, int64_t n_reads, int64_t read_len, int64_t first_read,
                     int32_t groups, const void *out_offsets, const void *group_first)
{
    const std::string name(who);
    if (groups < 1 || groups > kSplitMaxGroups)
        return fail(COVEST_E_INVALID, name + ": groups must be within 1 .. " + std::to_string(kSplitMaxGroups));
    COVEST_TRY(fail_if(check_reads_args(name, offsets != nullptr, n_reads, read_len, first_read, out_offsets != nullptr)));
    if (!group_first)
        return fail(COVEST_E_INVALID, name + ": group_first is null");
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_split_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, int64_t first_read, int32_t groups, uint64_t seed, uint8_t *d_out_bases,
                              int64_t *d_out_offsets, int64_t *d_read_index, int64_t *d_group_first, void *stream)
{
    COVEST_TRY(check_split_args("covest_split_reads_device", d_offsets, n_reads, read_len, first_read, groups,
                                d_out_offsets, d_group_first));
    DeviceCall call(device, "covest_split_reads_device");
    COVEST_TRY(call.status());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_reads == 0) { // nothing launched: the groups' starts, and the one output offset there is, by a memset on the stream
        HIP_TRY(hipMemsetAsync(d_group_first, 0, (size_t)(groups + 1) * sizeof(int64_t), st));
        if (d_out_offsets)
            HIP_TRY(hipMemsetAsync(d_out_offsets, 0, sizeof(int64_t), st));
        return COVEST_OK;
    }
    CallScratch *scratch = nullptr; // (call_scratch.h: the call returns before its kernels have run)
    COVEST_TRY(call_scratch_take(call.device(), split_scratch_bytes(n_reads, groups), "scratch of covest_split_reads_device",
                                 &scratch));
    const hipError_t e = launch_split_reads(d_bases, d_offsets, n_reads, read_len, first_read, groups, seed, d_out_bases,
                                            d_out_offsets, d_read_index, d_group_first, scratch->buf.ptr, st);
    call_scratch_give(scratch, st); // (whatever was launched before a failure still works on the block)
    HIP_TRY(e);
    return COVEST_OK;
}

int covest_split_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                       int64_t first_read, int32_t groups, uint64_t seed, uint8_t *out_bases, int64_t *out_offsets,
                       int64_t *read_index, int64_t *group_first)
{
    COVEST_TRY(check_split_args("covest_split_reads", offsets, n_reads, read_len, first_read, groups, out_offsets,
                                group_first));
    COVEST_TRY(fail_if(check_ascending_offsets("covest_split_reads", offsets, n_reads)));
    const int64_t end_byte = offsets ? offsets[n_reads] : n_reads * read_len; // (the bases are copied from byte 0)
    if (n_reads > 0 && end_byte > 0 && (!bases || !out_bases))
        return fail(COVEST_E_INVALID, "covest_split_reads: null buffer");
    if (n_reads == 0) {
        std::fill(group_first, group_first + groups + 1, (int64_t)0);
        if (out_offsets)
            out_offsets[0] = 0;
        return COVEST_OK;
    }
    DeviceCall call(device, "covest_split_reads");
    COVEST_TRY(call.status());
    const size_t first_bytes = (size_t)(groups + 1) * sizeof(int64_t);
    ReadsStage stage; // (goes with the call, on every path, as the two below; the copies back have waited for the kernels)
    DevBuf d_first, d_scratch;
    COVEST_TRY(stage.upload(bases, offsets, n_reads, (size_t)end_byte, out_offsets != nullptr, read_index != nullptr));
    HIP_TRY(d_first.reserve(first_bytes));
    HIP_TRY(d_scratch.reserve(split_scratch_bytes(n_reads, groups)));
    HIP_TRY(launch_split_reads(stage.d_bases.as<uint8_t>(), stage.d_offsets.as<int64_t>(), n_reads, read_len, first_read,
                               groups, seed, stage.d_out_bases.as<uint8_t>(), stage.d_out_offsets.as<int64_t>(),
                               stage.d_index.as<int64_t>(), d_first.as<int64_t>(), d_scratch.ptr, nullptr));
    HIP_TRY(hipMemcpy(group_first, d_first.ptr, first_bytes, hipMemcpyDeviceToHost));
    // a ragged input's bytes in all are offsets[n_reads] - offsets[0]: the reads need not start at byte 0
    const size_t out_bytes = offsets ? (size_t)(offsets[n_reads] - offsets[0]) : (size_t)end_byte;
    return stage.download(out_bases, out_bytes, out_offsets, (size_t)n_reads + 1, read_index, (size_t)n_reads);
}

} // extern "C"
