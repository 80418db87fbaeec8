// abi_bootstrap.cpp -- covest_bootstrap_weights* of the C ABI over bootstrap_weights.hip: the multiplicities of the
// Poisson bootstrap over reads.  No handle: the device form launches on the caller's stream and
// returns; the host form owns its device buffer for the call.  (The weighted adds they feed: kmer_host.cpp.)
#include "bootstrap_weights.h"
#include "host.h"

using namespace covest;

namespace {

// The checks both forms share.
int check_weights_args(const char *who, int64_t n_reads, int64_t first_read, const void *out)
{
    const std::string name(who);
    if (n_reads < 0 || first_read < 0)
        return fail(COVEST_E_INVALID, name + ": n_reads and first_read must not be negative");
    COVEST_TRY(fail_if(check_reads_reach(name, first_read, n_reads, 0)));
    if (n_reads > 0 && !out)
        return fail(COVEST_E_INVALID, name + ": null output");
    if (reinterpret_cast<uintptr_t>(out) % alignof(uint32_t) != 0)
        return fail(COVEST_E_INVALID, name + ": the output must be aligned to 4 bytes");
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_bootstrap_weights_device(int32_t device, int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate,
                                    uint32_t *d_out, void *stream)
{
    COVEST_TRY(check_weights_args("covest_bootstrap_weights_device", n_reads, first_read, d_out));
    if (n_reads == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_bootstrap_weights_device");
    COVEST_TRY(call.status());
    HIP_TRY(launch_bootstrap_weights(n_reads, first_read, seed, replicate, d_out, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_bootstrap_weights(int32_t device, int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate,
                             uint32_t *out)
{
    COVEST_TRY(check_weights_args("covest_bootstrap_weights", n_reads, first_read, out));
    if (n_reads == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_bootstrap_weights");
    COVEST_TRY(call.status());
    DevBuf d_out; // (goes with the call, on every path; the copy back has waited for the kernel)
    HIP_TRY(d_out.reserve((size_t)n_reads * sizeof(uint32_t)));
    HIP_TRY(launch_bootstrap_weights(n_reads, first_read, seed, replicate, d_out.as<uint32_t>(), nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, (size_t)n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
