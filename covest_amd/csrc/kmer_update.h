// kmer_update.h -- one walk over packed reads for everything that CHANGES the one-word k-mer table (k <= 31), and one
// walk over its launches.  kmer_count.hip adds by it, kmer_remove.hip takes back out by it; the
// wide table (kmer_wide.hip, keys of its own) shares the wave-a-read half of the launches.
//
// The walk: a wave64 a read (wave_read.h: lane s the windows s, s + 64, ...), or, for reads of ONE length, the windows of
// all reads numbered through and a thread a window.  A read of weight 0 returns before it touches the bases; a read
// shorter than k gives the one key "hash of what there is", an empty read k-mer 0 (bin/kmer_hist.py:36-37).
//
// An operation is what is done with a window's key.  It carries the pointer to its sticky word and has two calls:
//   window(t, key, rc, n, carry)   the key n times into, or out of, the table; what it must still look at goes to `carry`
//   settle(n, carry)               once, behind the last window of the lane: what `carry` holds is looked at
// Every branch of the walk -- the short read, the window loop, the numbered window -- makes the same two calls.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_read.h"

namespace covest {
namespace kmer {

// The add: table_add, nothing carried.  Sticky word: the counter's overflow word.
struct TableAdd {
    int *overflow;
    struct Carry {};
    __device__ __forceinline__ void window(const KmerTable &t, unsigned long long key, unsigned long long rc,
                                           unsigned long long n, Carry &) const
    {
        table_add(t, key, rc, n, overflow);
    }
    __device__ __forceinline__ void settle(unsigned long long, const Carry &) const {}
};

// `sub` taken from the count of `key`: the count before, or 0 where no slot carries the key (then smaller than any sub:
// underflow by the same compare)
__device__ __forceinline__ unsigned long long table_sub(const KmerTable &t, unsigned long long key, unsigned long long rc,
                                                        unsigned long long sub)
{
    unsigned long long seen;
    const unsigned long long h = table_locate(t, key, rc, seen);
    if (h == kNoSlot)
        return 0ull;
    // (`minus` named ahead of the call, and `under` ahead of `before` in TableSub::Carry, change which registers the compiler
    // picks and nothing else: with them the removal kernels are the code they were before this header, byte for byte
    // (DESIGN.md section 6ao).  Neither is needed for a right result.)
    const unsigned long long minus = 0ull - sub;
    return atomicAdd(&t.slots[h].count, minus); // returning: global_atomic_add_x2 ... sc0
}

// The subtraction (kmer_remove.hip says why the atomic returns).  Carried: the count before the last window's
// subtraction, compared only behind the NEXT window's key and walk, and whether an earlier one was too small.  Sticky
// word: the counter's underflow word.
struct TableSub {
    int *underflow;
    struct Carry {
        bool under = false;
        unsigned long long before = ~0ull; // a "count before" that is never too small
    };
    __device__ __forceinline__ void window(const KmerTable &t, unsigned long long key, unsigned long long rc,
                                           unsigned long long n, Carry &c) const
    {
        const unsigned long long now = table_sub(t, key, rc, n);
        c.under = c.under || c.before < n;
        c.before = now;
    }
    __device__ __forceinline__ void settle(unsigned long long n, const Carry &c) const
    {
        if (c.under || c.before < n)
            *underflow = 1;
    }
};

// One window of a read: its 2k-bit code (hash_kmer / rehash, bin/kmer_hist.py:18-31), the reverse complement's, the
// canonical choice, the operation.  `n`: 1, or the read's weight.
template <class Op>
__device__ __forceinline__ void update_window(const unsigned char *__restrict__ seq, int64_t s, int64_t len, int k,
                                              int canonical, const KmerTable &t, Op op, unsigned long long n,
                                              typename Op::Carry &carry)
{
    unsigned long long h, rc;
    window_key(seq, s, len, k, canonical, h, rc);
    op.window(t, h, rc, n, carry);
}

// A wave a read.  kWeighted: every occurrence counts weights[read] times in its one atomic; the weight is wave-uniform.
// The unweighted instantiation has the constant 1 and does not look at `weights`.
template <bool kWeighted, class Op>
__device__ __forceinline__ void update_read(const unsigned char *__restrict__ bases, const int64_t *__restrict__ offsets,
                                            int64_t n_reads, int64_t fixed_len, int k, int canonical, const KmerTable &t,
                                            Op op, const uint32_t *__restrict__ weights)
{
    WaveRead w;
    if (!wave_read(bases, offsets, n_reads, fixed_len, k, w))
        return;
    unsigned long long n = 1ull;
    if (kWeighted) {
        n = weights[w.r];
        if (n == 0)
            return;
    }
    typename Op::Carry carry;
    if (w.len < k) {
        if (w.lane == 0) {
            unsigned long long h = 0, rc = 0;
            for (int i = 0; i < (int)w.len; ++i) {
                const unsigned long long c = base_code(w.seq[i]);
                h = (h << 2) | c;
            }
            rc = revcomp_code(h, k);
            canonical_pair(h, rc, canonical);
            op.window(t, h, rc, n, carry);
            op.settle(n, carry);
        }
        return;
    }
    for (int64_t s = w.lane; s < w.len - k + 1; s += kWave) // (len >= k: w.n_windows without its clamp, which costs 0.5 %)
        update_window(w.seq, s, w.len, k, canonical, t, op, n, carry);
    op.settle(n, carry);
}

// Reads of ONE length (what a sequencing run's FASTQ holds, and config 5's synthetic reads): the windows of all reads
// are numbered through -- read = index / windows per read -- and a wave takes 64 consecutive ones, so that no lane
// idles in a read's last 64-window round (100-base reads have 80 windows: 64 + 16 lanes, 37 % of the slots empty).
// kWeighted: the lane takes its read's weight, and a weight of 0 returns before the bases are read.
template <bool kWeighted, class Op>
__device__ __forceinline__ void update_numbered_window(const unsigned char *__restrict__ bases, int64_t n_reads, int64_t len,
                                                       int k, int canonical, const KmerTable &t, Op op,
                                                       const uint32_t *__restrict__ weights)
{
    const int64_t n_windows = len - k + 1; // (the host sends reads shorter than k to the wave-a-read kernel)
    const int64_t total = n_reads * n_windows;
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total)
        return;
    const int64_t r = w / n_windows;
    unsigned long long n = 1ull;
    if (kWeighted) {
        n = weights[r];
        if (n == 0)
            return;
    }
    typename Op::Carry carry;
    update_window(bases + r * len, w - r * n_windows, len, k, canonical, t, op, n, carry);
    op.settle(n, carry);
}

// ---- the launches ------------------------------------------------------------------------------------------------------
// A wave a read (kmer_plan::for_each_wave_launch): the kernel `wave(bases, offsets, n, fixed_len, mid...)`, or with
// weights `wave_weighted(..., mid..., weights)` -- a weight a read, which goes with the launch's first read
// (kmer_plan.h weights_at).  `mid`: what the kernel takes between the reads and the weights.  (The weighted kernel is
// named first, as in the branch below: a kernel that is a template is emitted where it is first named, and the wide
// table's code object keeps the order it had.)
template <class WaveWeighted, class Wave, class... Mid>
void launch_wave_reads(WaveWeighted wave_weighted, Wave wave, const unsigned char *bases, const int64_t *offsets,
                       int64_t n_reads, int64_t fixed_len, const uint32_t *weights, hipStream_t stream, Mid... mid)
{
    kmer_plan::for_each_wave_launch(n_reads, fixed_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        const dim3 grid((unsigned)l.blocks), block(kWaveReadsPerBlock * kWave);
        const int64_t *offs = offsets ? offsets + l.first : nullptr;
        if (weights)
            hipLaunchKernelGGL(wave_weighted, grid, block, 0, stream, bases + l.byte_at, offs, l.n, fixed_len, mid...,
                               weights + kmer_plan::weights_at(l));
        else
            hipLaunchKernelGGL(wave, grid, block, 0, stream, bases + l.byte_at, offs, l.n, fixed_len, mid...);
    });
}

// An update of the one-word table by its four kernels.  Reads of one length that have a window: 64 consecutive windows
// per wave (the numbered kernels), at most 2^23 workgroups of 256 windows per launch, cut at whole reads
// (kmer_plan::window_reads_per_launch; the weights: window_weights_at); every other read set a wave a read.  weights ==
// nullptr: the unweighted kernels.  `sticky`: the word the operation sets (TableAdd, TableSub).
template <class Wave, class WaveWeighted, class Numbered, class NumberedWeighted>
hipError_t launch_update(Wave wave, WaveWeighted wave_weighted, Numbered numbered, NumberedWeighted numbered_weighted,
                         const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len, int k,
                         int canonical, const KmerTable &t, int *sticky, hipStream_t stream, const uint32_t *weights)
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
                hipLaunchKernelGGL(numbered_weighted, grid, dim3(256), 0, stream, bases + first * fixed_len, n, fixed_len, k,
                                   canonical, t, sticky, weights + kmer_plan::window_weights_at(first));
            else
                hipLaunchKernelGGL(numbered, grid, dim3(256), 0, stream, bases + first * fixed_len, n, fixed_len, k, canonical,
                                   t, sticky);
        }
        return hipGetLastError();
    }
    launch_wave_reads(wave_weighted, wave, bases, offsets, n_reads, fixed_len, weights, stream, k, canonical, t, sticky);
    return hipGetLastError();
}

} // namespace kmer
} // namespace covest
