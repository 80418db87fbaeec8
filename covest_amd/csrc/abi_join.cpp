// abi_join.cpp -- covest_kmer_join_histogram* of the C ABI over kmer_join.hip: two counters' tables joined on their keys
// into the matrix of clipped counts.  Nothing here, or below it, writes to either table.
#include "host.h"
#include "kmer_join.h"

using namespace covest;

namespace {

// what both forms refuse before a lock is taken: the handles themselves
int check_handles(const std::string &name, const covest_kmer *a, const covest_kmer *b)
{
    if (!a || !b)
        return fail(COVEST_E_INVALID, name + ": null counter");
    if (a == b)
        return fail(COVEST_E_INVALID, name + ": the same counter twice (a join needs two tables)");
    return COVEST_OK;
}

// ... and with both locks held: the counters against each other, the matrix, the output (`align`: what it must be
// aligned to), and last, as the other readers of the table, that both tables hold their keys
int check_join(const std::string &name, const covest_kmer *a, const covest_kmer *b, int64_t n_rows, int64_t n_cols,
               const int64_t *out, size_t align)
{
    COVEST_TRY(fail_if(check_table_holds_keys(name, a->wide || b->wide, false)));
    if (a->k != b->k || a->canonical != b->canonical || a->device != b->device)
        return fail(COVEST_E_INVALID, name + ": the counters differ in k, in the canonical flag or in their device");
    if (!kmer_join::cells_ok(n_rows, n_cols))
        return fail(COVEST_E_INVALID, name + ": n_rows and n_cols must be at least 1 and n_rows * n_cols at most 2^22");
    if (!out || (uintptr_t)out % align)
        return fail(COVEST_E_INVALID, name + ": the output is null or not aligned to 8 bytes");
    return fail_if(check_table_holds_keys(name, 0, a->bulk || b->bulk));
}

int read_flag(const covest_kmer *c, int *flag) // flag[kKmerStickyWords]: the overflow word and the underflow word
{
    HIP_TRY(hipMemcpy(flag, c->flag.ptr, kKmerStickyWords * sizeof(int), hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // namespace

extern "C" {

int covest_kmer_join_histogram_device(covest_kmer *a, covest_kmer *b, int64_t n_rows, int64_t n_cols, int64_t *d_out,
                                      void *stream)
{
    const std::string name("covest_kmer_join_histogram_device");
    COVEST_TRY(check_handles(name, a, b));
    std::scoped_lock guard(a->lock, b->lock); // (std::lock's order: join(a, b) and join(b, a) cannot wait for each other)
    COVEST_TRY(check_join(name, a, b, n_rows, n_cols, d_out, alignof(int64_t)));
    DeviceGuard dev_guard(a->device);
    COVEST_TRY(dev_guard.status());
    HIP_TRY(launch_kmer_join(a->table, b->table, n_rows, n_cols, d_out, static_cast<hipStream_t>(stream)));
    return COVEST_OK;
}

int covest_kmer_join_histogram(covest_kmer *a, covest_kmer *b, int64_t n_rows, int64_t n_cols, int64_t *out)
{
    const std::string name("covest_kmer_join_histogram");
    COVEST_TRY(check_handles(name, a, b));
    std::scoped_lock guard(a->lock, b->lock);
    COVEST_TRY(check_join(name, a, b, n_rows, n_cols, out, 1)); // (host memory: memcpy's, any alignment)
    DeviceGuard dev_guard(a->device);
    COVEST_TRY(dev_guard.status());
    const size_t bytes = (size_t)(n_rows * n_cols) * sizeof(int64_t);
    DevBuf d_out; // (goes with the call; the copy back has waited for the kernel)
    HIP_TRY(d_out.reserve(bytes));
    HIP_TRY(hipDeviceSynchronize()); // the adds may run on a caller's non-blocking stream, the join on the null stream
    HIP_TRY(launch_kmer_join(a->table, b->table, n_rows, n_cols, d_out.as<int64_t>(), nullptr));
    HIP_TRY(hipDeviceSynchronize());
    int flag_a[kKmerStickyWords] = {0, 0}, flag_b[kKmerStickyWords] = {0, 0};
    COVEST_TRY(read_flag(a, flag_a));
    COVEST_TRY(read_flag(b, flag_b));
    if (flag_a[kKmerOverflowWord] || flag_b[kKmerOverflowWord])
        return fail(COVEST_E_NOMEM, name + ": k-mer table overflow, the counts are partial: covest_kmer_clear and recount "
                                           "with more slots");
    if (flag_a[kKmerUnderflowWord] || flag_b[kKmerUnderflowWord])
        return fail(COVEST_E_INVALID, kmer_underflow_text(name.c_str()));
    HIP_TRY(hipMemcpy(out, d_out.ptr, bytes, hipMemcpyDeviceToHost));
    return COVEST_OK;
}

} // extern "C"
