// bootstrap_weights.hip -- K-weights: how often each read is drawn in one replicate of the Poisson bootstrap over reads
// (covest_bootstrap_weights*).
//
// Read r (64-bit: index in the call + first_read) of replicate b takes word 0 of Philox block (lo32(r), hi32(r), b, 9)
// (sim_philox.h kStreamBootstrap) and counts the thirteen thresholds of the Poisson(1) distribution function at or below
// it (poisson1_multiplicity).  A lane a read, one 4-byte store a lane, coalesced: the ten Philox rounds are the cost.
// Launches are cut as sample_reads.hip cuts its own (kmer_plan::lane_blocks_per_launch).  Nothing is written outside
// out[0 .. n_reads).
#include <hip/hip_runtime.h>

#include "bootstrap_weights.h"
#include "kmer_plan.h"
#include "sim_philox.h"

namespace covest {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void bootstrap_weights_kernel(const long long n_reads, const unsigned long long first_read,
                                                                     const uint32_t replicate, const uint32_t key0,
                                                                     const uint32_t key1, const long long block0,
                                                                     uint32_t *__restrict__ out)
{
    const long long idx = (block0 + (long long)blockIdx.x) * kThreads + threadIdx.x;
    if (idx >= n_reads)
        return;
    out[idx] = bootstrap_weight(first_read + (unsigned long long)idx, replicate, PhiloxKey{key0, key1});
}

} // namespace

hipError_t launch_bootstrap_weights(int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate, uint32_t *out,
                                    hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    const int64_t n_blocks = (n_reads + kThreads - 1) / kThreads;
    const PhiloxKey key = philox_key(seed);
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, n_blocks));
        hipLaunchKernelGGL(bootstrap_weights_kernel, grid, dim3(kThreads), 0, stream, (long long)n_reads,
                           (unsigned long long)first_read, replicate, key.k0, key.k1, (long long)b0, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace covest
