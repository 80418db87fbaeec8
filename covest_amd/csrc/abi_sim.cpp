// abi_sim.cpp -- covest_random_genome*, covest_simulate_reads* of the C ABI over sim_reads.hip: the counterpart of the
// reference's tools/simulator/generate_sequence.py and read_simulator.py:60-88.  No handle: the
// device forms launch on the caller's stream and return; the host forms own their device buffers for the call.
#include "host.h"

using namespace covest;

namespace {

// The checks both forms of covest_simulate_reads share; *thr = floor(error_rate * 2^32) (2^32 at error_rate 1).
int check_reads_args(const char *who, const void *genome, int64_t genome_len, int32_t read_len, int64_t first_read,
                     int64_t n_reads, double error_rate, const void *bases, uint64_t *thr)
{
    const std::string name(who);
    if (read_len < 1)
        return fail(COVEST_E_INVALID, name + ": read_len must be at least 1");
    if (genome_len <= read_len) // randrange(genome_size - read_length) of an empty range raises (read_simulator.py:75)
        return fail(COVEST_E_INVALID, name + ": the genome must be longer than a read");
    if (n_reads < 0 || first_read < 0)
        return fail(COVEST_E_INVALID, name + ": n_reads and first_read must not be negative");
    if (!(error_rate >= 0.0 && error_rate <= 1.0)) // (NaN fails both)
        return fail(COVEST_E_INVALID, name + ": error_rate must be in [0, 1]");
    COVEST_TRY(fail_if(check_reads_reach(name, first_read, n_reads, read_len)));
    if (n_reads > 0 && (!genome || !bases))
        return fail(COVEST_E_INVALID, name + ": null buffer");
    *thr = (uint64_t)std::floor(error_rate * 4294967296.0);
    return COVEST_OK;
}

bool is_acgt(uint8_t b)
{
    switch (b) {
    case 'a': case 'c': case 'g': case 't':
    case 'A': case 'C': case 'G': case 'T':
        return true;
    default:
        return false;
    }
}

} // namespace

extern "C" {

int covest_random_genome_device(int32_t device, int64_t n, uint64_t seed, uint8_t *d_out, void *stream)
{
    if (n < 0 || (n > 0 && !d_out))
        return fail(COVEST_E_INVALID, "covest_random_genome_device: bad argument");
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_random_genome_device");
    COVEST_TRY(call.status());
    HIP_TRY(launch_random_genome(n, seed, d_out, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_simulate_reads_device(int32_t device, const uint8_t *d_genome, int64_t genome_len, int32_t read_len,
                                 int64_t first_read, int64_t n_reads, double error_rate, uint64_t seed,
                                 int32_t both_strands, uint8_t *d_bases, int64_t *d_origin, void *stream)
{
    uint64_t thr = 0;
    COVEST_TRY(check_reads_args("covest_simulate_reads_device", d_genome, genome_len, read_len, first_read, n_reads,
                                error_rate, d_bases, &thr));
    if (n_reads == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_simulate_reads_device");
    COVEST_TRY(call.status());
    HIP_TRY(launch_sim_reads(d_genome, genome_len, read_len, first_read, n_reads, thr, seed, both_strands != 0, d_bases,
                             d_origin, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_random_genome(int32_t device, int64_t n, uint64_t seed, uint8_t *out)
{
    if (n < 0 || (n > 0 && !out))
        return fail(COVEST_E_INVALID, "covest_random_genome: bad argument");
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_random_genome");
    COVEST_TRY(call.status());
    DevBuf d_out; // (goes with the call; hipMemcpy below has waited for the kernel by then)
    HIP_TRY(d_out.reserve((size_t)n));
    HIP_TRY(launch_random_genome(n, seed, d_out.as<uint8_t>(), nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, (size_t)n, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_simulate_reads(int32_t device, const uint8_t *genome, int64_t genome_len, int32_t read_len, int64_t first_read,
                          int64_t n_reads, double error_rate, uint64_t seed, int32_t both_strands, uint8_t *bases,
                          int64_t *origin)
{
    uint64_t thr = 0;
    COVEST_TRY(check_reads_args("covest_simulate_reads", genome, genome_len, read_len, first_read, n_reads, error_rate,
                                bases, &thr));
    if (genome)
        for (int64_t i = 0; i < genome_len; ++i)
            if (!is_acgt(genome[i])) // (-s, the IUPAC substitution of read_simulator.py:34-57, is not built)
                return fail(COVEST_E_INVALID, "covest_simulate_reads: genome byte outside acgtACGT at " + std::to_string(i));
    if (n_reads == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_simulate_reads");
    COVEST_TRY(call.status());
    const size_t n_bytes = (size_t)n_reads * (size_t)read_len, origin_bytes = (size_t)n_reads * sizeof(int64_t);
    DevBuf d_genome, d_bases, d_origin; // (go with the call, on every path; the last copy has waited for the kernel)
    HIP_TRY(d_genome.reserve((size_t)genome_len));
    HIP_TRY(d_bases.reserve(n_bytes));
    if (origin)
        HIP_TRY(d_origin.reserve(origin_bytes));
    COVEST_TRY(stage_upload(d_genome.ptr, genome, (size_t)genome_len, "covest_simulate_reads: upload of the genome"));
    HIP_TRY(launch_sim_reads(d_genome.as<uint8_t>(), genome_len, read_len, first_read, n_reads, thr, seed, both_strands != 0,
                             d_bases.as<uint8_t>(), origin ? d_origin.as<int64_t>() : nullptr, nullptr));
    HIP_TRY(hipMemcpy(bases, d_bases.ptr, n_bytes, hipMemcpyDeviceToHost));
    if (origin)
        HIP_TRY(hipMemcpy(origin, d_origin.ptr, origin_bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
