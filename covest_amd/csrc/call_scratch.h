// call_scratch.h -- device scratch of the entry points that launch on the caller's stream and return (abi_sample.cpp,
// abi_split.cpp).  Such a call returns before its kernels have run, so what they work on cannot go with the call: a
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

} // namespace covest
