// kmer_count.hip -- K-kmer: the k-mer abundance histogram of bin/kmer_hist.py on gfx950
// (BASELINE.json config 5).
//
// Reference restated (paths in the reference checkout):
//   single_hash / hash_kmer / rehash  bin/kmer_hist.py:14-31   a=0 c=1 g=2 t=3, 2 bits per base
//   compute_counts                    :34-41   exact counts keyed by the 2k-bit integer
//   compute_histogram                 :57-64   count-of-counts
// `canonical` (min of the code and its reverse complement's) is the jellyfish -C convention that
// config 5 asks for; the reference itself is forward-strand only.
//
// Shape: one wave64 per read; lane s owns the window starting at base s (then s+64, ...), builds
// its 2k-bit code from k byte loads (neighbouring lanes overlap: L1-resident) and inserts it into
// an open-addressing table in HBM: 16-byte slots {key u64 (CAS on first touch), count u64 (atomic add)}.
// Bound: HBM random atomics -- one 8-byte read/CAS and one 8-byte add per k-mer, both in the same line, 64
// different cache lines per wave instruction (MI355X_MICROARCH.md, Global atomics: the scattered shape runs
// ~17x below the 1.3 TB/s contiguous-atomic rate); the arithmetic is noise.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "kmer_update.h"

namespace covest {

namespace {

using namespace kmer;

// The four adding kernels: kmer_update.h's walk with the add as its operation.  A wave a read,
// plain and weighted (every occurrence is added weights[read] times in its one atomic add); reads of ONE length, the
// windows numbered through, plain and weighted.
__global__ __launch_bounds__(256) void kmer_count_kernel(const unsigned char *__restrict__ bases,
                                                         const int64_t *__restrict__ offsets,
                                                         int64_t n_reads, int64_t fixed_len, int k,
                                                         int canonical, const KmerTable t, int *overflow)
{
    update_read<false>(bases, offsets, n_reads, fixed_len, k, canonical, t, TableAdd{overflow}, nullptr);
}

__global__ __launch_bounds__(256) void kmer_count_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                  const int64_t *__restrict__ offsets, int64_t n_reads,
                                                                  int64_t fixed_len, int k, int canonical,
                                                                  const KmerTable t, int *overflow,
                                                                  const uint32_t *__restrict__ weights)
{
    update_read<true>(bases, offsets, n_reads, fixed_len, k, canonical, t, TableAdd{overflow}, weights);
}

__global__ __launch_bounds__(256) void kmer_count_fixed_kernel(const unsigned char *__restrict__ bases, int64_t n_reads,
                                                               int64_t len, int k, int canonical, const KmerTable t,
                                                               int *overflow)
{
    update_numbered_window<false>(bases, n_reads, len, k, canonical, t, TableAdd{overflow}, nullptr);
}

__global__ __launch_bounds__(256) void kmer_count_fixed_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                        int64_t n_reads, int64_t len, int k, int canonical,
                                                                        const KmerTable t, int *overflow,
                                                                        const uint32_t *__restrict__ weights)
{
    update_numbered_window<true>(bases, n_reads, len, k, canonical, t, TableAdd{overflow}, weights);
}

// Re-insert every HELD key of `src` (kmer_table.h) into the `dst` table -- a larger one, or one of the same size
// (covest_kmer_compact): a key whose count a removal brought to 0 does not travel.
__global__ __launch_bounds__(256) void kmer_rehash_kernel(const KmerTable src, const KmerTable dst, int *overflow)
{
    const unsigned long long n = src.mask + 1;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const KmerSlot e = src.slots[i];
        if (slot_held(e.key, e.count))
            table_add(dst, e.key, revcomp_code(e.key, dst.k), e.count, overflow);
    }
}

__global__ __launch_bounds__(256) void kmer_fill_empty_kernel(KmerSlot *slots, unsigned long long n)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x)
        slots[i] = KmerSlot{kEmptyKey, 0ull}; // one 16-byte store per lane: coalesced streaming write
}

// stats[0] = max count, stats[1] = distinct keys: the keys HELD (kmer_table.h), stats[2] = the slots occupied
__global__ __launch_bounds__(256) void kmer_stats_kernel(const KmerTable t, unsigned long long *stats)
{
    const unsigned long long n = t.mask + 1;
    unsigned long long distinct = 0, mx = 0, occupied = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const KmerSlot e = t.slots[i];
        if (slot_occupied(e.key)) {
            ++occupied;
            distinct += slot_held(e.key, e.count) ? 1ull : 0ull;
            mx = e.count > mx ? e.count : mx; // (a count of 0 raises no maximum)
        }
    }
    wave_fold_distinct_max(distinct, mx);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        occupied += __shfl_xor(occupied, off, kWave);
    // The three words share a line, and every atomic on it queues behind the others: a workgroup folds its four waves in
    // LDS first and sends three atomics, where a wave each sending its own would be twelve (the parent's kernel sent eight).
    __shared__ unsigned long long part[3][256 / kWave];
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        part[0][wave] = mx;
        part[1][wave] = distinct;
        part[2][wave] = occupied;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; ++w) {
            mx = part[0][w] > mx ? part[0][w] : mx;
            distinct += part[1][w];
            occupied += part[2][w];
        }
        atomicMax(&stats[0], mx);
        atomicAdd(&stats[1], distinct);
        atomicAdd(&stats[2], occupied);
    }
}

// compute_histogram: hist[c] = number of keys with count c, c < hist_len.  Low counts go through
// LDS-private bins (one flush of atomics per workgroup), the rare high ones straight to HBM.
constexpr int kLdsBins = 4096;
__global__ __launch_bounds__(256) void kmer_histogram_kernel(const KmerTable t, unsigned long long *hist,
                                                             unsigned long long hist_len)
{
    __shared__ unsigned bins[kLdsBins];
    for (int i = threadIdx.x; i < kLdsBins; i += blockDim.x)
        bins[i] = 0u;
    __syncthreads();
    const unsigned long long n = t.mask + 1;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const KmerSlot e = t.slots[i];
        if (slot_held(e.key, e.count)) { // (a key of count 0 is not counted: hist[0] stays 0)
            const unsigned long long c = e.count;
            if (c < (unsigned long long)kLdsBins)
                atomicAdd(&bins[c], 1u);
            else if (c < hist_len)
                atomicAdd(&hist[c], 1ull);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kLdsBins; i += blockDim.x)
        if (bins[i] != 0u && (unsigned long long)i < hist_len)
            atomicAdd(&hist[i], (unsigned long long)bins[i]);
}

} // namespace

hipError_t launch_kmer_fill_empty(const KmerTable &t, hipStream_t stream)
{
    const unsigned long long n = t.mask + 1;
    hipLaunchKernelGGL(kmer_fill_empty_kernel, dim3(grid_for(n)), dim3(256), 0, stream, t.slots, n);
    return hipGetLastError();
}

// weights == nullptr: the unweighted kernels; else a weight a read (kmer_update.h launch_update)
hipError_t launch_kmer_count(const unsigned char *bases, const int64_t *offsets, int64_t n_reads,
                             int64_t fixed_len, int k, int canonical, const KmerTable &t, int *overflow,
                             hipStream_t stream, const uint32_t *weights)
{
    return kmer::launch_update(kmer_count_kernel, kmer_count_weighted_kernel, kmer_count_fixed_kernel,
                               kmer_count_fixed_weighted_kernel, bases, offsets, n_reads, fixed_len, k, canonical, t, overflow,
                               stream, weights);
}

hipError_t launch_kmer_rehash(const KmerTable &src, const KmerTable &dst, int *overflow, hipStream_t stream)
{
    hipLaunchKernelGGL(kmer_rehash_kernel, dim3(grid_for(src.mask + 1)), dim3(256), 0, stream, src, dst, overflow);
    return hipGetLastError();
}

hipError_t launch_kmer_stats(const KmerTable &t, unsigned long long *stats, hipStream_t stream)
{
    hipLaunchKernelGGL(kmer_stats_kernel, dim3(grid_for(t.mask + 1)), dim3(256), 0, stream, t, stats);
    return hipGetLastError();
}

hipError_t launch_kmer_histogram(const KmerTable &t, unsigned long long *hist, unsigned long long hist_len,
                                 hipStream_t stream)
{
    hipLaunchKernelGGL(kmer_histogram_kernel, dim3(grid_for(t.mask + 1)), dim3(256), 0, stream, t, hist, hist_len);
    return hipGetLastError();
}

} // namespace covest
