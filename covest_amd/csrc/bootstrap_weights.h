// bootstrap_weights.h -- the launcher of bootstrap_weights.hip (abi_bootstrap.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace covest {

// out[n_reads] (device): the multiplicity of reads first_read .. first_read + n_reads - 1 in `replicate` under `seed`
// (sim_philox.h bootstrap_weight).  Asynchronous on `stream`; nothing outside out[0 .. n_reads) is written.
hipError_t launch_bootstrap_weights(int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate, uint32_t *out,
                                    hipStream_t stream);

} // namespace covest
