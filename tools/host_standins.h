// host_standins.h -- what the GPU-less harnesses (tools/plan_bytes.cpp, tools/tiles_bytes.cpp) put in the place of HIP
// and of host_common.cpp: malloc and memcpy, a log of every HIP call (name, byte count, destination as an offset into
// the allocation it lies in), and look-alikes of the pure helpers (the same on both sides of a comparison, so that two
// builds of the code under test see the same values).  Included by exactly one translation unit of a harness.
#pragma once
#include "host.h"

static bool g_timing; // a timing loop: nothing is logged or remembered
static std::vector<std::pair<char *, size_t>> g_allocs;
static std::string g_hip_log, g_last_error;

static size_t alloc_size(const void *p)
{
    for (auto &a : g_allocs)
        if (a.first == p)
            return a.second;
    return 0;
}
static std::string place_of(const void *p) // "a<ordinal of the allocation>+<offset>"
{
    const char *c = (const char *)p;
    for (size_t i = 0; i < g_allocs.size(); ++i)
        if (c >= g_allocs[i].first && c < g_allocs[i].first + g_allocs[i].second)
            return "a" + std::to_string(i) + "+" + std::to_string(c - g_allocs[i].first);
    return p ? "elsewhere" : "null";
}
static void log_call(const char *name, size_t bytes, const void *dst)
{
    if (!g_timing)
        g_hip_log += std::string(name) + " " + std::to_string(bytes) + " " + place_of(dst) + "\n";
}
static void *logged_alloc(const char *name, size_t n)
{
    void *p = calloc(1, n ? n : 1);
    if (!g_timing) {
        g_allocs.push_back({(char *)p, n});
        log_call(name, n, p);
    }
    return p;
}

extern "C" {
hipError_t hipDeviceSynchronize() { log_call("hipDeviceSynchronize", 0, nullptr); return hipSuccess; }
hipError_t hipFree(void *p) { log_call("hipFree", 0, p); return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipHostFree(void *p) { log_call("hipHostFree", 0, p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = logged_alloc("hipHostMalloc", n); return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = logged_alloc("hipMalloc", n); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { log_call("hipMemcpy", n, d); memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { log_call("hipMemcpyAsync", n, d); memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { log_call("hipMemsetAsync", n, d); memset(d, v, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { log_call("hipStreamSynchronize", 0, nullptr); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { log_call("hipStreamWaitEvent", 0, nullptr); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)calloc(1, 8); log_call("hipEventCreate", 0, nullptr); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)calloc(1, 8); log_call("hipEventCreateWithFlags", 0, nullptr); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { log_call("hipEventRecord", 0, nullptr); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { log_call("hipEventDestroy", 0, nullptr); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
}

namespace covest {
int set_error(int code, const std::string &msg)
{
    g_last_error = msg;
    fprintf(stderr, "error %d %s\n", code, msg.c_str());
    return code;
}
int fail_hip(hipError_t, const char *w) { fprintf(stderr, "hip error %s\n", w); return -1; }
bool dev_cache_take(size_t, void **, size_t *, int *) { return false; }
bool dev_cache_give(void *, size_t, int) { return true; }
DeviceIdleScope::DeviceIdleScope() {}
DeviceIdleScope::~DeviceIdleScope() {}
bool DeviceIdleScope::active() { return true; }
SharedStage &shared_stage() { static SharedStage s; return s; }
double clamp_one(const DevModel &dm, int d, double v) { return std::min(std::max(v, dm.lo[d]), dm.hi[d]); }
void lgamma_ensure(int64_t) {}
double lgamma_at(int64_t j) { return std::lgamma((double)j + 1.0); }
double lgamma_of_factorial(int64_t j) { return std::lgamma((double)j + 1.0); }
} // namespace covest

#ifdef STANDIN_GRID_STAGE // a harness that does not link abi_grid.cpp: one block, refilled with 0x5a outside timing loops
namespace covest {
static std::vector<char> g_stage;
int grid_stage_begin(covest_grid *, size_t bytes, StageSlot &slot)
{
    if (g_stage.size() < bytes || !g_timing)
        g_stage.assign(bytes, 0x5a);
    slot.ptr = g_stage.data();
    return 0;
}
int grid_stage_commit(covest_grid *, StageSlot &slot, void *dst, size_t bytes) { memcpy(dst, slot.ptr, bytes); return 0; }
} // namespace covest
#endif
