// call_scratch.h -- device memory of the entry points over packed reads that take no handle (abi_sample.cpp,
// abi_split.cpp; the block partials of covest_rows_moments_device, abi_influence.cpp): the scratch of the device forms,
// and the staging of the host forms (ReadsStage, at the end).
// A device form launches on the caller's stream and returns.  Such a call returns before its kernels have run, so what they work on cannot go with the call: a
// block is handed to ONE call at a time and to the next only once the event recorded behind that call's last launch has
// come to pass.  Blocks stay with the process (as the device cache's do); calls that overlap on several streams get a
// block each.
#pragma once
#include "host.h"

namespace covest {

struct CallScratch {
    DevBuf buf;
    hipEvent_t done = nullptr;
    int device = -1;
    bool in_use = false;
};
struct CallScratchPool {
    std::mutex mu;
    std::deque<CallScratch> blocks; // (a deque: growing it moves no block a call holds)
};
inline CallScratchPool &call_scratch_pool()
{
    static CallScratchPool *pool = new CallScratchPool; // (never destroyed: no HIP call after the runtime has gone)
    return *pool;
}

// `what` names the scratch in the message of a failure
inline int call_scratch_take(int device, size_t bytes, const char *what, CallScratch **out)
{
    CallScratchPool &pool = call_scratch_pool();
    CallScratch *got = nullptr;
    {
        std::lock_guard<std::mutex> hold(pool.mu);
        for (CallScratch &s : pool.blocks)
            if (!s.in_use && s.device == device && hipEventQuery(s.done) == hipSuccess) {
                got = &s;
                break;
            }
        (void)hipGetLastError(); // (hipErrorNotReady of a query is no failure of this call)
        if (!got) {
            pool.blocks.emplace_back();
            got = &pool.blocks.back();
            got->device = device;
        }
        got->in_use = true;
    }
    hipError_t e = hipSuccess;
    if (!got->done)
        e = hipEventCreateWithFlags(&got->done, hipEventDisableTiming);
    if (e == hipSuccess) {
        // a block much larger than this call needs goes back to the device (the one 4 * 10^9-base call of a process
        // must not keep its scratch for ever)
        if (got->buf.cap > ((size_t)64 << 20) && got->buf.cap / 4 > bytes)
            got->buf.release();
        e = got->buf.reserve(bytes);
    }
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> hold(pool.mu);
        got->in_use = false;
        return fail_hip(e, what);
    }
    *out = got;
    return COVEST_OK;
}

inline void call_scratch_give(CallScratch *s, hipStream_t stream)
{
    (void)hipEventRecord(s->done, stream);
    std::lock_guard<std::mutex> hold(call_scratch_pool().mu);
    s->in_use = false;
}

// What a host form owns on the device for the call: the reads as they came, the reads as they go back, and ONE index
// per read that goes back with them (the sampler's kept_index, the split's read_index).  It goes with the call, on
// every path; the copies back wait for the kernels.
struct ReadsStage {
    DevBuf d_bases, d_offsets, d_out_bases, d_out_offsets, d_index;

    // Room for n_reads reads of n_bytes bases in all, counted from byte 0 of `bases` (offsets, out_offsets, index: only
    // where wanted), and the reads on the device.
    int upload(const uint8_t *bases, const int64_t *offsets, int64_t n_reads, size_t n_bytes, bool out_offsets, bool index)
    {
        const size_t index_bytes = (size_t)n_reads * sizeof(int64_t);
        HIP_TRY(d_bases.reserve(std::max<size_t>(n_bytes, 16)));
        HIP_TRY(d_out_bases.reserve(std::max<size_t>(n_bytes, 16)));
        if (offsets)
            HIP_TRY(d_offsets.reserve(index_bytes + sizeof(int64_t)));
        if (out_offsets)
            HIP_TRY(d_out_offsets.reserve(index_bytes + sizeof(int64_t)));
        if (index)
            HIP_TRY(d_index.reserve(index_bytes));
        if (n_bytes)
            HIP_TRY(hipMemcpy(d_bases.ptr, bases, n_bytes, hipMemcpyHostToDevice));
        if (offsets)
            HIP_TRY(hipMemcpy(d_offsets.ptr, offsets, index_bytes + sizeof(int64_t), hipMemcpyHostToDevice));
        return COVEST_OK;
    }
    // The first n_bases output bases, n_offsets output offsets and n_index indices back (a count of 0, or an array that
    // was not wanted: nothing).
    int download(uint8_t *out_bases, size_t n_bases, int64_t *out_offsets, size_t n_offsets, int64_t *index, size_t n_index)
    {
        if (n_bases)
            HIP_TRY(hipMemcpy(out_bases, d_out_bases.ptr, n_bases, hipMemcpyDeviceToHost));
        if (out_offsets && n_offsets)
            HIP_TRY(hipMemcpy(out_offsets, d_out_offsets.ptr, n_offsets * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (index && n_index)
            HIP_TRY(hipMemcpy(index, d_index.ptr, n_index * sizeof(int64_t), hipMemcpyDeviceToHost));
        return COVEST_OK;
    }
};

} // namespace covest
