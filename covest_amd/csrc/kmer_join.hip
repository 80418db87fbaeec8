// kmer_join.hip -- two k-mer tables of kmer_count.hip joined on their keys: out[i][j] = the number of keys held by at
// least one of A and B whose count in A, clipped, is i and whose count in B, clipped, is j (kmer_join.h; DESIGN.md
// section 6am).  Read-only on both tables.
//
// Two sweeps, both grid-stride over slots as kmer_histogram_kernel's:
//   1. over A's slots: a held key probes B -- table_find with the key and the reverse complement derived from it, as
//      kmer_rehash_kernel derives it -- and counts into cell (clip a, clip b);
//   2. over B's slots: a held key probes A and counts into row 0 only when A holds none.
// A key of both tables is met in both sweeps and counted in the first alone; a key of one table is met once: no key is
// counted twice and none is missed.  Held is kmer_table.h's: a slot whose count a removal (kmer_remove.hip) brought to 0
// is passed over in both sweeps, and table_find answers 0 for it, so a key held by neither table is in no cell and cell
// (0, 0) stays 0.  Each table is walked and probed with its own log2_slots (first_slot, slot_of);
// has_first_slot is a function of k and of the probed table's size.
//
// The cells i < kLdsRows, j < kLdsCols are counted in workgroup-private bins in LDS and flushed once per workgroup; the
// others go straight to HBM.  Integer atomics: the result is the same on every run.  Folding the equal cells of a wave
// into one add of their number before the bins are touched was built and measured 6 % slower: a lane
// adds one.
//
// Bound: one 16-byte streaming load a slot of each table and, a held key, one scattered 16-byte load of the other
// table (table_find's first slot), against the histogram scan's streaming load alone.
#include "kmer_join.h"

#include "kmer_table.h"

namespace covest {

namespace {

using namespace kmer;

// the key of a slot counted into its cell: in the bins where the cell has one, else straight to HBM
__device__ __forceinline__ void count_cell(unsigned *bins, unsigned long long *out, uint32_t i, uint32_t j, uint32_t n_cols)
{
    if (kmer_join::in_lds(i, j))
        atomicAdd(&bins[kmer_join::lds_index(i, j)], 1u);
    else
        atomicAdd(&out[kmer_join::flat_index(i, j, n_cols)], 1ull);
}

__global__ __launch_bounds__(256) void kmer_join_kernel(const KmerTable a, const KmerTable b, unsigned long long *out,
                                                        uint32_t n_rows, uint32_t n_cols)
{
    __shared__ unsigned bins[kmer_join::kLdsBins];
    for (int i = threadIdx.x; i < kmer_join::kLdsBins; i += blockDim.x)
        bins[i] = 0u;
    __syncthreads();
    const unsigned long long first = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long n_a = a.mask + 1, n_b = b.mask + 1;
    for (unsigned long long s = first; s < n_a; s += stride) {
        const ulonglong2 e = slot_load(a, s);
        if (slot_held(e.x, e.y))
            count_cell(bins, out, kmer_join::clip(e.y, n_rows),
                       kmer_join::clip(table_find(b, e.x, revcomp_code(e.x, b.k)), n_cols), n_cols);
    }
    for (unsigned long long s = first; s < n_b; s += stride) {
        const ulonglong2 e = slot_load(b, s);
        if (slot_held(e.x, e.y) && table_find(a, e.x, revcomp_code(e.x, a.k)) == 0ull)
            count_cell(bins, out, 0u, kmer_join::clip(e.y, n_cols), n_cols);
    }
    __syncthreads();
    for (int at = threadIdx.x; at < kmer_join::kLdsBins; at += blockDim.x) {
        const uint32_t i = (uint32_t)at / kmer_join::kLdsCols, j = (uint32_t)at % kmer_join::kLdsCols;
        if (bins[at] != 0u && i < n_rows && j < n_cols) // (a bin outside the matrix is never added to: the clips)
            atomicAdd(&out[kmer_join::flat_index(i, j, n_cols)], (unsigned long long)bins[at]);
    }
}

} // namespace

hipError_t launch_kmer_join(const KmerTable &a, const KmerTable &b, int64_t n_rows, int64_t n_cols, int64_t *out,
                            hipStream_t stream)
{
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)(n_rows * n_cols) * sizeof(int64_t), stream);
    if (e != hipSuccess)
        return e;
    const unsigned long long n = a.mask > b.mask ? a.mask + 1 : b.mask + 1;
    hipLaunchKernelGGL(kmer_join_kernel, dim3(grid_for(n)), dim3(256), 0, stream, a, b,
                       reinterpret_cast<unsigned long long *>(out), (uint32_t)n_rows, (uint32_t)n_cols);
    return hipGetLastError();
}

} // namespace covest
