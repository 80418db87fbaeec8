// kmer_remove.hip -- K-kmer's counts taken back out of the one-word table (k <= 31) on gfx950: for every window of
// every read, what kmer_count.hip added is subtracted again.
//
// Shape: the add's, because it is the same code -- kmer_update.h's walk over the reads and over the launches, with the
// subtraction (TableSub, table_sub there) as its operation.
//
// A window: find the slot that carries the key by table_add's decisions WITHOUT storing (kmer_table.h table_locate: a
// removal creates no key), then one returning 64-bit atomic add of -sub on the slot's count.  The key stays: "held" and
// "occupied" in kmer_table.h.  The kernels of this file run behind the adds whose counts they take back -- same stream,
// or ordered after them by the caller -- so the walk reads slots with plain 16-byte loads, as the readers do; the count
// it loads is not looked at, the atomic's return is.
//
// Underflow: a key that occupies no slot, or a count that was smaller than what is subtracted (the count has then
// wrapped), sets the counter's sticky underflow word with a plain vector store of 1 -- a word of its own beside the
// overflow word, so neither erases the other.  After it the counts are unspecified.
//
// Bound: as the add, the rate at which the memory side retires scattered 8-byte operations -- one 16-byte load and one
// 8-byte atomic a window, both in the same line.  The atomic RETURNS (the add's does not): the wave-a-read loop keeps one
// in flight per lane and looks at its value only after the next window's key and walk, so no lane waits for an atomic
// with nothing else to do; a thread of the numbered form has one window and looks at once.  Fewer than 16 outstanding a
// wave either way (MI355X_MICROARCH.md, float-atomic row: issue stalls begin there).  Plain vector code; no assembly.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kmer_update.h"

namespace covest {

namespace {

using namespace kmer;

__global__ __launch_bounds__(256) void kmer_remove_kernel(const unsigned char *__restrict__ bases,
                                                          const int64_t *__restrict__ offsets, int64_t n_reads,
                                                          int64_t fixed_len, int k, int canonical, const KmerTable t,
                                                          int *underflow)
{
    update_read<false>(bases, offsets, n_reads, fixed_len, k, canonical, t, TableSub{underflow}, nullptr);
}

__global__ __launch_bounds__(256) void kmer_remove_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                   const int64_t *__restrict__ offsets, int64_t n_reads,
                                                                   int64_t fixed_len, int k, int canonical,
                                                                   const KmerTable t, int *underflow,
                                                                   const uint32_t *__restrict__ weights)
{
    update_read<true>(bases, offsets, n_reads, fixed_len, k, canonical, t, TableSub{underflow}, weights);
}

__global__ __launch_bounds__(256) void kmer_remove_fixed_kernel(const unsigned char *__restrict__ bases, int64_t n_reads,
                                                                int64_t len, int k, int canonical, const KmerTable t,
                                                                int *underflow)
{
    update_numbered_window<false>(bases, n_reads, len, k, canonical, t, TableSub{underflow}, nullptr);
}

__global__ __launch_bounds__(256) void kmer_remove_fixed_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                         int64_t n_reads, int64_t len, int k, int canonical,
                                                                         const KmerTable t, int *underflow,
                                                                         const uint32_t *__restrict__ weights)
{
    update_numbered_window<true>(bases, n_reads, len, k, canonical, t, TableSub{underflow}, weights);
}

} // namespace

hipError_t launch_kmer_remove(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len, int k,
                              int canonical, const KmerTable &t, int *underflow, hipStream_t stream, const uint32_t *weights)
{
    return kmer::launch_update(kmer_remove_kernel, kmer_remove_weighted_kernel, kmer_remove_fixed_kernel,
                               kmer_remove_fixed_weighted_kernel, bases, offsets, n_reads, fixed_len, k, canonical, t, underflow,
                               stream, weights);
}

} // namespace covest
