// kmer_remove.hip -- K-kmer's counts taken back out of the one-word table (k <= 31) on gfx950: for every window of
// every read, what kmer_count.hip added is subtracted again.
//
// Shape: kmer_count.hip's, read for read -- the same read view (wave_read.h: a wave64 a read, lane s the windows s,
// s + 64, ...), the same key of a window (window_key), the same launch walk (kmer_plan::for_each_wave_launch; reads of one
// length: the windows numbered through, a thread a window), the same weight of a launch's first read (weights_at,
// window_weights_at).  A read of weight 0 returns before it touches the bases; a read shorter than k removes the one key
// "hash of what there is", an empty read k-mer 0: exactly what the add adds for them.
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
#include "wave_read.h"

namespace covest {

namespace {

using namespace kmer;

constexpr unsigned long long kNothingBefore = ~0ull; // a "count before" that is never too small

// `sub` taken from the count of `key`: the count before, or 0 where no slot carries the key (then smaller than any sub:
// underflow by the same compare)
__device__ __forceinline__ unsigned long long table_sub(const KmerTable &t, unsigned long long key, unsigned long long rc,
                                                        unsigned long long sub)
{
    unsigned long long seen;
    const unsigned long long h = table_locate(t, key, rc, seen);
    if (h == kNoSlot)
        return 0ull;
    return atomicAdd(&t.slots[h].count, 0ull - sub); // returning: global_atomic_add_x2 ... sc0
}

__device__ __forceinline__ unsigned long long remove_window(const unsigned char *__restrict__ seq, int64_t s, int64_t len,
                                                            int k, int canonical, const KmerTable &t, unsigned long long sub)
{
    unsigned long long h, rc;
    window_key(seq, s, len, k, canonical, h, rc);
    return table_sub(t, h, rc, sub);
}

// A wave a read: count_read of kmer_count.hip with the subtraction in place of the add.
template <bool kWeighted>
__device__ __forceinline__ void remove_read(const unsigned char *__restrict__ bases, const int64_t *__restrict__ offsets,
                                            int64_t n_reads, int64_t fixed_len, int k, int canonical, const KmerTable &t,
                                            int *underflow, const uint32_t *__restrict__ weights)
{
    WaveRead w;
    if (!wave_read(bases, offsets, n_reads, fixed_len, k, w))
        return;
    unsigned long long sub = 1ull;
    if (kWeighted) {
        sub = weights[w.r];
        if (sub == 0)
            return;
    }
    if (w.len < k) {
        if (w.lane == 0) {
            unsigned long long h = 0, rc = 0;
            for (int i = 0; i < (int)w.len; ++i) {
                const unsigned long long c = base_code(w.seq[i]);
                h = (h << 2) | c;
            }
            rc = revcomp_code(h, k);
            canonical_pair(h, rc, canonical);
            if (table_sub(t, h, rc, sub) < sub)
                *underflow = 1;
        }
        return;
    }
    unsigned long long before = kNothingBefore; // of the window before this one: looked at behind the next walk
    bool under = false;
    for (int64_t s = w.lane; s < w.len - k + 1; s += kWave) {
        const unsigned long long now = remove_window(w.seq, s, w.len, k, canonical, t, sub);
        under = under || before < sub;
        before = now;
    }
    if (under || before < sub)
        *underflow = 1;
}

__global__ __launch_bounds__(256) void kmer_remove_kernel(const unsigned char *__restrict__ bases,
                                                          const int64_t *__restrict__ offsets, int64_t n_reads,
                                                          int64_t fixed_len, int k, int canonical, const KmerTable t,
                                                          int *underflow)
{
    remove_read<false>(bases, offsets, n_reads, fixed_len, k, canonical, t, underflow, nullptr);
}

__global__ __launch_bounds__(256) void kmer_remove_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                   const int64_t *__restrict__ offsets, int64_t n_reads,
                                                                   int64_t fixed_len, int k, int canonical,
                                                                   const KmerTable t, int *underflow,
                                                                   const uint32_t *__restrict__ weights)
{
    remove_read<true>(bases, offsets, n_reads, fixed_len, k, canonical, t, underflow, weights);
}

// Reads of ONE length, the windows numbered through (count_numbered_window of kmer_count.hip).
template <bool kWeighted>
__device__ __forceinline__ void remove_numbered_window(const unsigned char *__restrict__ bases, int64_t n_reads, int64_t len,
                                                       int k, int canonical, const KmerTable &t, int *underflow,
                                                       const uint32_t *__restrict__ weights)
{
    const int64_t n_windows = len - k + 1; // (the host sends reads shorter than k to kmer_remove_kernel)
    const int64_t total = n_reads * n_windows;
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total)
        return;
    const int64_t r = w / n_windows;
    unsigned long long sub = 1ull;
    if (kWeighted) {
        sub = weights[r];
        if (sub == 0)
            return;
    }
    if (remove_window(bases + r * len, w - r * n_windows, len, k, canonical, t, sub) < sub)
        *underflow = 1;
}

__global__ __launch_bounds__(256) void kmer_remove_fixed_kernel(const unsigned char *__restrict__ bases, int64_t n_reads,
                                                                int64_t len, int k, int canonical, const KmerTable t,
                                                                int *underflow)
{
    remove_numbered_window<false>(bases, n_reads, len, k, canonical, t, underflow, nullptr);
}

__global__ __launch_bounds__(256) void kmer_remove_fixed_weighted_kernel(const unsigned char *__restrict__ bases,
                                                                         int64_t n_reads, int64_t len, int k, int canonical,
                                                                         const KmerTable t, int *underflow,
                                                                         const uint32_t *__restrict__ weights)
{
    remove_numbered_window<true>(bases, n_reads, len, k, canonical, t, underflow, weights);
}

} // namespace

// launch_kmer_count's walk over the launches, kernel for kernel
hipError_t launch_kmer_remove(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len, int k,
                              int canonical, const KmerTable &t, int *underflow, hipStream_t stream, const uint32_t *weights)
{
    if (n_reads <= 0)
        return hipSuccess;
    if (!offsets && fixed_len >= k) {
        const int64_t n_windows = fixed_len - k + 1;
        const int64_t reads_per_launch = kmer_plan::window_reads_per_launch(n_windows);
        for (int64_t first = 0; first < n_reads; first += reads_per_launch) {
            const int64_t n = kmer_plan::reads_of_launch(first, n_reads, reads_per_launch);
            const int64_t total = n * n_windows;
            const dim3 grid((unsigned)((total + 255) / 256));
            if (weights)
                hipLaunchKernelGGL(kmer_remove_fixed_weighted_kernel, grid, dim3(256), 0, stream, bases + first * fixed_len, n,
                                   fixed_len, k, canonical, t, underflow, weights + kmer_plan::window_weights_at(first));
            else
                hipLaunchKernelGGL(kmer_remove_fixed_kernel, grid, dim3(256), 0, stream, bases + first * fixed_len, n,
                                   fixed_len, k, canonical, t, underflow);
        }
        return hipGetLastError();
    }
    kmer_plan::for_each_wave_launch(n_reads, fixed_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        const dim3 grid((unsigned)l.blocks), block(kWaveReadsPerBlock * kWave);
        const int64_t *offs = offsets ? offsets + l.first : nullptr;
        if (weights)
            hipLaunchKernelGGL(kmer_remove_weighted_kernel, grid, block, 0, stream, bases + l.byte_at, offs, l.n, fixed_len, k,
                               canonical, t, underflow, weights + kmer_plan::weights_at(l));
        else
            hipLaunchKernelGGL(kmer_remove_kernel, grid, block, 0, stream, bases + l.byte_at, offs, l.n, fixed_len, k,
                               canonical, t, underflow);
    });
    return hipGetLastError();
}

} // namespace covest
