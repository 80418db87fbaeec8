// abi_influence.cpp -- covest_kmer_read_influence* and covest_rows_moments* of the C ABI over kmer_influence.hip: the
// delete-one-read change of a table-valued sum over the distinct k-mers, per read, and the moments of such rows
// (DESIGN.md section 6ai).  Nothing here, or below it, writes to the k-mer table.
#include "call_scratch.h"
#include "host.h"
#include "kmer_influence.h"

using namespace covest;

namespace {

int too_many_windows(const char *who, int64_t read, int64_t windows)
{
    return fail(COVEST_E_UNSUPPORTED, std::string(who) + ": read " + std::to_string(read) + " has " + std::to_string(windows) +
                                          " windows, more than " + std::to_string(kInfluenceMaxWindows) +
                                          " (the compare is quadratic in them)");
}

int influence_locked(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads, int64_t read_len,
                     const double *d_table, int64_t n_rows, int32_t n_cols, double *d_rows, void *stream)
{
    const std::string name("covest_kmer_read_influence_device");
    COVEST_TRY(fail_if(check_table_reads_sizes(name, d_offsets != nullptr, n_reads, read_len)));
    if (n_rows < 1 || n_cols < 1 || n_cols > kInfluenceMaxCols)
        return fail(COVEST_E_INVALID, name + ": the table needs at least one row and 1 .. " +
                                          std::to_string(kInfluenceMaxCols) + " columns");
    if (n_rows > std::numeric_limits<int64_t>::max() / (int64_t)(n_cols * sizeof(double)))
        return fail(COVEST_E_INVALID, name + ": a table beyond 64-bit sizes");
    if (!d_table || (n_reads > 0 && !d_rows))
        return fail(COVEST_E_INVALID, name + ": null table or rows");
    if ((uintptr_t)d_table % alignof(double) || (uintptr_t)d_rows % alignof(double))
        return fail(COVEST_E_INVALID, name + ": the table or the rows are not aligned to 8 bytes");
    COVEST_TRY(fail_if(check_table_holds_keys(name, c->wide, c->bulk)));
    if (n_reads == 0)
        return COVEST_OK;
    if (!d_bases)
        return fail(COVEST_E_INVALID, name + ": null bases");
    // reads of one length: the host sees the windows (with offsets the kernel answers NaN for such a read)
    if (!d_offsets && read_len - c->table.k + 1 > kInfluenceMaxWindows)
        return too_many_windows(name.c_str(), 0, read_len - c->table.k + 1);
    DeviceGuard dev_guard(c->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(launch_kmer_read_influence(d_bases, d_offsets, n_reads, read_len, c->canonical, c->table, d_table, n_rows,
                                       n_cols, d_rows, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int check_moments(const char *who, const void *rows, int64_t n, int32_t q, const void *centre, const void *sum,
                  const void *cross)
{
    const std::string name(who);
    if (n < 0 || n > ((int64_t)1 << 40))
        return fail(COVEST_E_INVALID, name + ": n must be within 0 .. 2^40");
    if (q < 1 || q > kMomentsMaxQ)
        return fail(COVEST_E_INVALID, name + ": q must be within 1 .. " + std::to_string(kMomentsMaxQ));
    if (!centre || !sum || !cross || (n > 0 && !rows))
        return fail(COVEST_E_INVALID, name + ": null argument");
    if ((uintptr_t)rows % alignof(double) || (uintptr_t)centre % alignof(double) || (uintptr_t)sum % alignof(double) ||
        (uintptr_t)cross % alignof(double))
        return fail(COVEST_E_INVALID, name + ": an array is not aligned to 8 bytes");
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_kmer_read_influence_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                      int64_t read_len, const double *d_table, int64_t n_rows, int32_t n_cols,
                                      double *d_rows, void *stream)
{
    if (!c)
        return fail(COVEST_E_INVALID, "covest_kmer_read_influence_device: null counter");
    std::lock_guard<std::mutex> guard(c->lock);
    return influence_locked(c, d_bases, d_offsets, n_reads, read_len, d_table, n_rows, n_cols, d_rows, stream);
}

int covest_kmer_read_influence(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                               const double *table, int64_t n_rows, int32_t n_cols, double *rows)
{
    if (!c || n_reads < 0 || (n_reads > 0 && !offsets))
        return fail(COVEST_E_INVALID, "covest_kmer_read_influence: bad argument");
    if (n_rows < 1 || n_cols < 1 || n_cols > kInfluenceMaxCols || !table || (n_reads > 0 && !rows))
        return fail(COVEST_E_INVALID, "covest_kmer_read_influence: the table needs at least one row and 1 .. " +
                                          std::to_string(kInfluenceMaxCols) + " columns, and the rows a place");
    if (n_rows > std::numeric_limits<int64_t>::max() / (int64_t)(n_cols * sizeof(double)))
        return fail(COVEST_E_INVALID, "covest_kmer_read_influence: a table beyond 64-bit sizes");
    COVEST_TRY(fail_if(check_table_holds_keys("covest_kmer_read_influence", c->wide, false))); // (bulk: the device form's)
    if (n_reads == 0)
        return COVEST_OK;
    const int64_t n_bytes = offsets[n_reads] - offsets[0];
    if (n_bytes < 0 || (n_bytes > 0 && !bases))
        return fail(COVEST_E_INVALID, "covest_kmer_read_influence: bad offsets");
    for (int64_t i = 0; i < n_reads; ++i) {
        if (offsets[i + 1] < offsets[i])
            return fail(COVEST_E_INVALID, "covest_kmer_read_influence: bad offsets");
        const int64_t windows = offsets[i + 1] - offsets[i] - c->table.k + 1;
        if (windows > kInfluenceMaxWindows)
            return too_many_windows("covest_kmer_read_influence", i, windows);
    }
    const size_t table_bytes = (size_t)n_rows * (size_t)n_cols * sizeof(double);
    const size_t rows_bytes = (size_t)n_reads * (size_t)(n_cols + 1) * sizeof(double);
    KmerHostCall call(c);
    COVEST_TRY(call.open(bases, offsets, n_reads));
    DevBuf d_table, d_rows; // (go with the call; the copy back has waited for the kernel)
    HIP_TRY(d_table.reserve(table_bytes));
    HIP_TRY(hipMemcpy(d_table.ptr, table, table_bytes, hipMemcpyHostToDevice));
    HIP_TRY(d_rows.reserve(rows_bytes));
    COVEST_TRY(influence_locked(c, c->ws_bases.as<uint8_t>(), c->ws_offsets.as<int64_t>(), n_reads, 0, d_table.as<double>(),
                                n_rows, n_cols, d_rows.as<double>(), nullptr));
    COVEST_TRY(call.close("covest_kmer_read_influence"));
    HIP_TRY(hipMemcpy(rows, d_rows.ptr, rows_bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

int covest_rows_moments_device(const double *d_rows, int64_t n, int32_t q, const double *d_centre, double *d_sum,
                               double *d_cross, void *stream)
{
    COVEST_TRY(check_moments("covest_rows_moments_device", d_rows, n, q, d_centre, d_sum, d_cross));
    DeviceCall call(-1, "covest_rows_moments_device"); // (the calling thread's current device: the arrays live there)
    COVEST_TRY(call.status());
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallScratch *scratch = nullptr; // (call_scratch.h: the call returns before its kernels have run)
    COVEST_TRY(call_scratch_take(call.device(), moments_scratch_bytes(n, q), "scratch of covest_rows_moments_device", &scratch));
    const hipError_t e = launch_rows_moments(d_rows, n, q, d_centre, d_sum, d_cross, scratch->buf.ptr, st);
    call_scratch_give(scratch, st); // (whatever was launched before a failure still works on the block)
    HIP_TRY(e);
    return COVEST_OK;
}

int covest_rows_moments(const double *rows, int64_t n, int32_t q, const double *centre, double *sum, double *cross)
{
    COVEST_TRY(check_moments("covest_rows_moments", rows, n, q, centre, sum, cross));
    DeviceCall call(-1, "covest_rows_moments");
    COVEST_TRY(call.status());
    const size_t rows_bytes = (size_t)n * (size_t)q * sizeof(double), q_bytes = (size_t)q * sizeof(double);
    const size_t cross_bytes = (size_t)(q * (q + 1) / 2) * sizeof(double);
    DevBuf d_rows, d_centre, d_sum, d_cross, d_scratch; // (go with the call; the copies back wait for the kernels)
    HIP_TRY(d_rows.reserve(std::max<size_t>(rows_bytes, 16)));
    HIP_TRY(d_centre.reserve(q_bytes));
    HIP_TRY(d_sum.reserve(q_bytes));
    HIP_TRY(d_cross.reserve(cross_bytes));
    HIP_TRY(d_scratch.reserve(moments_scratch_bytes(n, q)));
    if (rows_bytes)
        HIP_TRY(hipMemcpy(d_rows.ptr, rows, rows_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_centre.ptr, centre, q_bytes, hipMemcpyHostToDevice));
    HIP_TRY(launch_rows_moments(d_rows.as<double>(), n, q, d_centre.as<double>(), d_sum.as<double>(), d_cross.as<double>(),
                                d_scratch.ptr, nullptr));
    HIP_TRY(hipMemcpy(sum, d_sum.ptr, q_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cross, d_cross.ptr, cross_bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
