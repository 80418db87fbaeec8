// abi_repeat.cpp -- covest_repeat_plan, covest_repeat_genome* of the C ABI over sim_repeats.hip: genomes whose k-mers
// have a prescribed copy-number distribution.  The plan is host arithmetic and needs no device;
// the device form launches on the caller's stream and returns; the host form owns its device buffers for the call.
#include "host.h"

#include <stdexcept>
#include "sim_philox.h"

using namespace covest;

namespace {

constexpr int32_t kMaxCopiesLimit = 1 << 20;
constexpr int64_t kMaxPlanUnits = (int64_t)1 << 40; // 16 bytes a unit on the host while the list is sorted: 16 TiB

bool in_unit_interval(double v) { return v >= 0.0 && v <= 1.0; } // (NaN fails both)

// t_o = min(2^32, floor(cdf_o * 2^32)) for o = 1 .. max_copies - 1, the cdf formed by basic IEEE operations in the
// order include/covest_amd.h states (no pow): RepeatsModel.get_b_o of the reference as a distribution
std::vector<uint64_t> copy_thresholds(double q1, double q2, double q, int32_t max_copies)
{
    std::vector<uint64_t> t;
    t.reserve((size_t)max_copies);
    double cdf = q1, b = 0.0;
    for (int32_t o = 1; o < max_copies; ++o) {
        if (o == 2) {
            cdf = cdf + (1.0 - q1) * q2;
        } else if (o == 3) {
            b = ((1.0 - q1) * (1.0 - q2)) * q;
            cdf = cdf + b;
        } else if (o > 3) {
            b = b * (1.0 - q);
            cdf = cdf + b;
        }
        const double scaled = std::floor(cdf * 4294967296.0);
        t.push_back(scaled >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)scaled);
    }
    return t;
}

// The checks both forms of covest_repeat_genome share; *thr = floor(divergence * 2^32) (2^32 at divergence 1).
int check_genome_args(const char *who, const void *plan, int64_t n_units, int32_t unit_len, int64_t n, double divergence,
                      const void *out, uint64_t *thr)
{
    const std::string name(who);
    if (unit_len < 1)
        return fail(COVEST_E_INVALID, name + ": unit_len must be at least 1");
    if (n < 0 || n_units < 0)
        return fail(COVEST_E_INVALID, name + ": n and n_units must not be negative");
    if (n_units < n / unit_len + (n % unit_len != 0 ? 1 : 0))
        return fail(COVEST_E_INVALID, name + ": n is more than n_units * unit_len");
    if (!in_unit_interval(divergence))
        return fail(COVEST_E_INVALID, name + ": divergence must be in [0, 1]");
    if (n > 0 && (!plan || !out))
        return fail(COVEST_E_INVALID, name + ": null buffer");
    *thr = (uint64_t)std::floor(divergence * 4294967296.0);
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_repeat_plan(int64_t n_units, double q1, double q2, double q, int32_t max_copies, uint64_t seed,
                       int32_t both_orientations, int64_t *plan, int64_t *n_families)
{
    if (!in_unit_interval(q1) || !in_unit_interval(q2) || !in_unit_interval(q))
        return fail(COVEST_E_INVALID, "covest_repeat_plan: q1, q2 and q must be in [0, 1]");
    if (max_copies < 1 || max_copies > kMaxCopiesLimit)
        return fail(COVEST_E_INVALID, "covest_repeat_plan: max_copies must be in 1 .. 2^20");
    if (n_units < 0)
        return fail(COVEST_E_INVALID, "covest_repeat_plan: n_units must not be negative");
    if (n_units > 0 && (!plan || !n_families))
        return fail(COVEST_E_INVALID, "covest_repeat_plan: null output");
    if (n_units == 0) {
        if (n_families)
            *n_families = 0;
        return COVEST_OK;
    }
    if (n_units > kMaxPlanUnits) // (before std::vector is asked: beyond its max_size it throws length_error, not bad_alloc)
        return fail(COVEST_E_NOMEM, "covest_repeat_plan: more than 2^40 units");
    const PhiloxKey key = philox_key(seed);
    struct Entry {
        uint64_t key;
        int64_t rec; // family << 1 | forward
    };
    std::vector<Entry> list;
    try {
        const std::vector<uint64_t> t = copy_thresholds(q1, q2, q, max_copies);
        list.reserve((size_t)n_units);
        uint64_t f = 0;
        while ((int64_t)list.size() < n_units) {
            uint32_t w[4];
            philox_block(f, 0u, kStreamCopies, key, w);
            // o_f = 1 + the number of thresholds <= u (they ascend: the cdf only grows)
            const int64_t copies = 1 + (std::upper_bound(t.begin(), t.end(), (uint64_t)w[0]) - t.begin());
            for (int64_t c = 0; c < copies && (int64_t)list.size() < n_units; ++c) {
                const uint64_t j = (uint64_t)list.size();
                philox_block(j, 0u, kStreamShuffle, key, w);
                const int64_t forward = (w[2] & 1u) | (both_orientations ? 0u : 1u);
                list.push_back({(uint64_t)w[0] | ((uint64_t)w[1] << 32), (int64_t)(f << 1) | forward});
            }
            ++f;
        }
        *n_families = (int64_t)f;
        // (entries are in order of j, so a stable sort by the key alone breaks ties by j)
        std::stable_sort(list.begin(), list.end(), [](const Entry &a, const Entry &b) { return a.key < b.key; });
    } catch (const std::exception &) { // (bad_alloc, length_error: nothing may leave an extern "C" function)
        return fail(COVEST_E_NOMEM, "covest_repeat_plan: the unit list does not fit the host's memory");
    }
    for (int64_t slot = 0; slot < n_units; ++slot)
        plan[slot] = list[(size_t)slot].rec;
    return COVEST_OK;
}

int covest_repeat_genome_device(int32_t device, const int64_t *d_plan, int64_t n_units, int32_t unit_len, int64_t n,
                                double divergence, uint64_t seed, uint8_t *d_out, void *stream)
{
    uint64_t thr = 0;
    COVEST_TRY(check_genome_args("covest_repeat_genome_device", d_plan, n_units, unit_len, n, divergence, d_out, &thr));
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_repeat_genome_device");
    COVEST_TRY(call.status());
    HIP_TRY(launch_repeat_genome(d_plan, unit_len, n, thr, seed, d_out, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_repeat_genome(int32_t device, const int64_t *plan, int64_t n_units, int32_t unit_len, int64_t n,
                         double divergence, uint64_t seed, uint8_t *out)
{
    uint64_t thr = 0;
    COVEST_TRY(check_genome_args("covest_repeat_genome", plan, n_units, unit_len, n, divergence, out, &thr));
    if (plan) {
        // the largest family id whose last base, (f + 1) * unit_len - 1, still fits 63 bits
        const int64_t f_max = std::numeric_limits<int64_t>::max() / unit_len - 1;
        for (int64_t u = 0; u < n_units; ++u) {
            if (plan[u] < 0)
                return fail(COVEST_E_INVALID, "covest_repeat_genome: negative plan entry at " + std::to_string(u));
            if ((plan[u] >> 1) > f_max)
                return fail(COVEST_E_INVALID, "covest_repeat_genome: family id times unit_len leaves 63 bits at " + std::to_string(u));
        }
    }
    if (n == 0)
        return COVEST_OK;
    DeviceCall call(device, "covest_repeat_genome");
    COVEST_TRY(call.status());
    const size_t n_used = (size_t)((n - 1) / unit_len + 1), plan_bytes = n_used * sizeof(int64_t); // the units the kernel reads
    DevBuf d_plan, d_out; // (go with the call, on every path; the last copy has waited for the kernel)
    HIP_TRY(d_plan.reserve(plan_bytes));
    HIP_TRY(d_out.reserve((size_t)n));
    COVEST_TRY(stage_upload(d_plan.ptr, plan, plan_bytes, "covest_repeat_genome: upload of the plan"));
    HIP_TRY(launch_repeat_genome(d_plan.as<int64_t>(), unit_len, n, thr, seed, d_out.as<uint8_t>(), nullptr));
    HIP_TRY(hipMemcpy(out, d_out.ptr, (size_t)n, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
