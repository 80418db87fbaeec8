// dedup_reads.hip -- K-dedup: duplicate reads removed on the device, the first copy kept, the kept reads compacted in
// input order into the packed layout the k-mer counter takes (covest_dedup_reads*).
//
// The result is a function of the input (dedup.h states it): candidates are decided by a fingerprint of the whole read
// (read_fingerprint.h), a table keyed by it keeps the LOWEST read index of every key, and a read is dropped only after
// its bytes have been compared with that read's.  Three memsets and the launches on the caller's stream, none of which
// waits for another workgroup:
//   0. memsets            the table to 0xff (every key the empty sentinel, every value above any index), the dropped
//                         counts and counts[0 .. 3) to 0
//   1. dedup_fingerprint  the hot path, the one kernel that reads every base of every read: a wave64 a read
//                         (wave_read.h); the per-base terms summed per lane and folded across the wave; lane 0 stores
//                         the key and inserts -- a CAS on the slot's key, linear probing from the Fibonacci hash, a
//                         64-bit atomicMin of the read index into the slot's value.  Slots never change their key.
//   2. dedup_resolve      a wave a read again: the slot by replaying the insert's probes, m = its value.  m == r: kept.
//                         Else the bytes of r and m are compared, a dword a lane, with a ballot (forward; where that
//                         fails and reverse_complement is set, against the reverse complement): equal -> dropped, one
//                         more copy of m; unequal -> kept, one more collided.  Integer atomics: exact in any order.
//   3. dedup_flags / dedup_scan / dedup_place   the sampler's three stages (sample_reads.hip) over the stored flags
//   4. the gather         gather_reads.hip (launch_gather_reads)
//
// Loads of the fingerprint kernel: a read's bases are taken in units of 16 bytes where the read has 1024 and more (a
// unit a lane fills the wave), of 4 bytes from 256 on, else byte by byte -- below those lengths a wider unit leaves
// most lanes idle while the others mix 16 bytes in a row, and mixing, not loading, is what the kernel spends its time
// on.  Bytes in front of the first unit that is aligned to its own size, and behind the last whole one, go byte by
// byte, so a unit is always naturally aligned and no load leaves the read: byte, dword and 16-byte starts alike.
#include <hip/hip_runtime.h>

#include "dedup.h"
#include "gather_reads.h"
#include "kmer_plan.h"
#include "read_fingerprint.h"
#include "scan.h"
#include "wave_read.h"

namespace covest {

namespace {

namespace fpr = fingerprint;
using kmer::kWaveReadsPerBlock;
using kmer::WaveRead;

constexpr int kThreads = kDedupShare;
constexpr int kWaves = kThreads / 64;
constexpr int kScanThreads = 1024;
constexpr int kScanPerLane = 4;

struct DedupSlot {
    unsigned long long key, value; // the fingerprint key (or the sentinel); the lowest read index that has it
};
static_assert(sizeof(DedupSlot) == 16, "a slot is 16 bytes");

struct Sums {
    unsigned long long fwd, rc;
};

__device__ __forceinline__ void add_byte(Sums &s, unsigned long long salt, unsigned long long j, unsigned long long len,
                                         unsigned b, int with_rc)
{
    s.fwd += fpr::term(salt, j, b);
    if (with_rc) // (uniform)
        s.rc += fpr::term_rc(salt, j, len, b);
}

__device__ __forceinline__ void add_word(Sums &s, unsigned long long salt, unsigned long long j, unsigned long long len,
                                         unsigned w, int with_rc)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
        add_byte(s, salt, j + i, len, (w >> (8 * i)) & 0xffu, with_rc);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// ---- 1. the fingerprint of every read, and its insert
__global__ __launch_bounds__(kWaveReadsPerBlock * 64) void dedup_fingerprint_kernel(
    const unsigned char *__restrict__ bases, const int64_t *__restrict__ offsets, const int64_t n_reads,
    const int64_t fixed_len, const unsigned long long first, const unsigned long long salt, const unsigned long long seed,
    const int with_rc, const int fp_bits, const int log2_slots, DedupSlot *__restrict__ slots,
    unsigned long long *__restrict__ state)
{
    WaveRead w;
    if (!kmer::wave_read(bases, offsets, n_reads, fixed_len, 1, w))
        return;
    const unsigned char *x = w.seq;
    const unsigned long long len = (unsigned long long)w.len;
    const unsigned unit = len >= 1024 ? 16u : len >= 256 ? 4u : 1u;
    unsigned long long head = (unsigned long long)(-(uintptr_t)x & (uintptr_t)(unit - 1u)); // bytes before the first aligned unit
    if (head > len)
        head = len;
    const unsigned long long n_units = (len - head) / unit, tail = head + n_units * unit;
    Sums s = {0ull, 0ull};
    if ((unsigned long long)w.lane < head)
        add_byte(s, salt, (unsigned long long)w.lane, len, x[w.lane], with_rc);
    if (unit == 16u) {
        for (unsigned long long u = w.lane; u < n_units; u += 64) {
            const unsigned long long j = head + 16ull * u;
            const uint4 v = *reinterpret_cast<const uint4 *>(x + j);
            add_word(s, salt, j, len, v.x, with_rc);
            add_word(s, salt, j + 4, len, v.y, with_rc);
            add_word(s, salt, j + 8, len, v.z, with_rc);
            add_word(s, salt, j + 12, len, v.w, with_rc);
        }
    } else if (unit == 4u) {
        for (unsigned long long u = w.lane; u < n_units; u += 64) {
            const unsigned long long j = head + 4ull * u;
            add_word(s, salt, j, len, *reinterpret_cast<const unsigned *>(x + j), with_rc);
        }
    } else {
        for (unsigned long long j = w.lane; j < n_units; j += 64) // (head == 0)
            add_byte(s, salt, j, len, x[j], with_rc);
    }
    if (tail + (unsigned long long)w.lane < len) // fewer than `unit` bytes
        add_byte(s, salt, tail + w.lane, len, x[tail + w.lane], with_rc);
    s.fwd = wave_sum_u64(s.fwd);
    if (with_rc)
        s.rc = wave_sum_u64(s.rc);
    if (w.lane != 0)
        return;
    const unsigned long long r = first + (unsigned long long)w.r;
    const unsigned long long key = fpr::key_of(s.fwd, s.rc, len, seed, with_rc, fp_bits);
    state[r] = key;
    const unsigned long long mask = (1ull << log2_slots) - 1ull;
    unsigned long long h = fpr::slot_of(key, log2_slots);
    for (int probe = 0; probe < kDedupMaxProbe; ++probe) {
        DedupSlot *slot = slots + h;
        // the CAS at once, with no load in front of it (kmer_table.h's try_slot loads first: its keys mostly repeat, a
        // read's mostly does not): one trip to memory a probe, and the wave has nothing else to hide a second behind
        const unsigned long long cur = atomicCAS(&slot->key, fpr::kEmptyKey, key); // returns the previous value
        if (cur == fpr::kEmptyKey || cur == key) {
            atomicMin(&slot->value, r);
            return;
        }
        h = (h + 1) & mask;
    }
    // out of probes: no slot holds the key within reach, and the resolve, which replays these probes, finds none
}

// the 4 bytes at p, of any alignment (all four within the read)
__device__ __forceinline__ unsigned load4(const unsigned char *p)
{
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// ---- 2. every read against the first read of its key: state[r] becomes its flag (1: kept)
__global__ __launch_bounds__(kWaveReadsPerBlock * 64) void dedup_resolve_kernel(
    const unsigned char *__restrict__ bases, const int64_t *__restrict__ offsets, const int64_t n_reads,
    const int64_t fixed_len, const unsigned long long first, const unsigned char *__restrict__ all_bases,
    const int64_t *__restrict__ all_offsets, const int with_rc, const int log2_slots,
    const DedupSlot *__restrict__ slots, unsigned long long *__restrict__ state, int *__restrict__ dropped_on,
    unsigned long long *__restrict__ collided)
{
    WaveRead w;
    if (!kmer::wave_read(bases, offsets, n_reads, fixed_len, 1, w))
        return;
    const unsigned long long r = first + (unsigned long long)w.r;
    const unsigned long long key = state[r]; // (every lane the same word; lane 0 alone writes it, below)
    const unsigned long long mask = (1ull << log2_slots) - 1ull;
    unsigned long long h = fpr::slot_of(key, log2_slots), m = fpr::kEmptyKey;
    for (int probe = 0; probe < kDedupMaxProbe; ++probe) { // (plain loads: the inserts ran in the launches before)
        const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(slots + h);
        if (e.x == key) {
            m = e.y;
            break;
        }
        if (e.x == fpr::kEmptyKey)
            break; // (cannot be: an insert stops at the first empty slot and takes it)
        h = (h + 1) & mask;
    }
    if (m == r) { // (uniform, as every branch below)
        if (w.lane == 0)
            state[r] = 1ull;
        return;
    }
    bool equal = false;
    if (m < r) { // (else: no slot within reach -- kept, and counted as collided)
        const int64_t q0 = all_offsets ? all_offsets[m] : (int64_t)m * fixed_len;
        const int64_t q_len = all_offsets ? all_offsets[m + 1] - q0 : fixed_len;
        if (q_len == w.len) {
            const unsigned char *x = w.seq, *y = all_bases + q0;
            const int64_t len = w.len;
            equal = true;
            for (int64_t base = 0; base < len && equal; base += 4 * 64) {
                const int64_t j = base + 4 * w.lane;
                bool differ = false;
                if (j + 4 <= len) {
                    differ = load4(x + j) != load4(y + j);
                } else {
                    for (int64_t i = j; i < len; ++i)
                        differ |= x[i] != y[i];
                }
                equal = __ballot(differ) == 0ull;
            }
            if (!equal && with_rc) {
                equal = true;
                for (int64_t base = 0; base < len && equal; base += 64) {
                    const int64_t j = base + w.lane;
                    const bool differ = j < len && (unsigned)x[j] != fpr::complement(y[len - 1 - j]);
                    equal = __ballot(differ) == 0ull;
                }
            }
        }
    }
    if (w.lane == 0) {
        state[r] = equal ? 0ull : 1ull;
        if (equal)
            atomicAdd(dropped_on + m, 1);
        else
            atomicAdd(collided, 1ull);
    }
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// ---- 3a. flags and kept lengths: pairs[2 * workgroup] = (reads kept, bases kept)
__global__ __launch_bounds__(kThreads) void dedup_flags_kernel(const long long *__restrict__ offsets, const long long read_len,
                                                               const long long n_reads,
                                                               const unsigned long long *__restrict__ state,
                                                               const long long block0, long long *__restrict__ pairs)
{
    __shared__ long long part[2][kWaves];
    const int tid = threadIdx.x;
    const long long blk = block0 + (long long)blockIdx.x;
    const long long idx = blk * kThreads + tid;
    long long cnt = 0, len = 0;
    if (idx < n_reads && state[idx] != 0ull) {
        cnt = 1;
        len = offsets ? offsets[idx + 1] - offsets[idx] : read_len;
    }
    cnt = wave_sum_i64(cnt);
    len = wave_sum_i64(len);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = cnt;
        part[1][tid >> 6] = len;
    }
    __syncthreads();
    if (tid == 0) {
        long long c = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            c += part[0][w];
            b += part[1][w];
        }
        pairs[2 * blk] = c;
        pairs[2 * blk + 1] = b;
    }
}

// ---- 3b. exclusive scan of the pairs, in place, by one workgroup; the totals (counts[2], the collided, stays)
__global__ __launch_bounds__(kScanThreads) void dedup_scan_kernel(long long *__restrict__ pairs, const long long n_blocks,
                                                                  long long *__restrict__ counts,
                                                                  long long *__restrict__ out_offsets)
{
    __shared__ long long wsum[2][kScanThreads / 64];
    long long carry_c, carry_b;
    scan_pair_row<kScanThreads, kScanPerLane>(pairs, n_blocks, &wsum[0][0], carry_c, carry_b);
    if (threadIdx.x == 0) {
        counts[0] = carry_c;
        counts[1] = carry_b;
        if (out_offsets)
            out_offsets[carry_c] = carry_b;
    }
}

// ---- 3c. every kept read to its rank: output offset, global index, copies, source offset
__global__ __launch_bounds__(kThreads) void dedup_place_kernel(
    const long long *__restrict__ offsets, const long long read_len, const long long n_reads,
    const unsigned long long first_read, const unsigned long long *__restrict__ state, const int *__restrict__ dropped_on,
    const long long block0, const long long *__restrict__ pairs, long long *__restrict__ out_offsets,
    long long *__restrict__ kept_index, int *__restrict__ copies, long long *__restrict__ src_off)
{
    __shared__ long long part[2][kWaves];
    const int tid = threadIdx.x;
    const long long blk = block0 + (long long)blockIdx.x;
    const long long idx = blk * kThreads + tid;
    long long cnt = 0, len = 0, src = 0;
    if (idx < n_reads && state[idx] != 0ull) {
        cnt = 1;
        if (offsets) {
            src = offsets[idx];
            len = offsets[idx + 1] - src;
        } else {
            src = idx * read_len;
            len = read_len;
        }
    }
    long long before[2] = {cnt, len}, all[2]; // the workgroup's kept reads, and their bases, before this one
    block_exclusive_scan<kWaves, 2>(before, &part[0][0], all);
    const long long rank = pairs[2 * blk] + before[0], at = pairs[2 * blk + 1] + before[1];
    if (cnt) {
        if (out_offsets)
            out_offsets[rank] = at;
        if (kept_index)
            kept_index[rank] = (long long)(first_read + (unsigned long long)idx);
        if (copies)
            copies[rank] = 1 + dropped_on[idx];
        src_off[rank] = src;
    }
}

// the parts of the scratch, each aligned to 16 bytes
struct Scratch {
    int log2_slots;
    int64_t n_blocks;
    size_t table, state, dropped, pairs, src_off, bytes; // byte offsets; the size
};
Scratch scratch_of(int64_t n_reads)
{
    const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    Scratch s;
    s.log2_slots = fpr::table_log2_slots(n_reads);
    s.n_blocks = (n_reads + kThreads - 1) / kThreads;
    s.table = 0;
    s.dropped = s.table + ((size_t)16 << s.log2_slots); // (next to the table: their two memsets touch one run of bytes)
    s.state = s.dropped + up16((size_t)n_reads * sizeof(int));
    s.pairs = s.state + up16((size_t)n_reads * sizeof(long long));
    s.src_off = s.pairs + up16((size_t)(2 * s.n_blocks) * sizeof(long long));
    s.bytes = s.src_off + up16((size_t)n_reads * sizeof(long long));
    return s;
}

} // namespace

size_t dedup_scratch_bytes(int64_t n_reads)
{
    return scratch_of(n_reads).bytes;
}

hipError_t launch_dedup_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                              int64_t first_read, int reverse_complement, int fp_bits, uint64_t seed,
                              unsigned char *out_bases, int64_t *out_offsets, int64_t *kept_index, int32_t *copies,
                              int64_t *counts, void *scratch, hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    const Scratch s = scratch_of(n_reads);
    unsigned char *base = static_cast<unsigned char *>(scratch);
    DedupSlot *slots = reinterpret_cast<DedupSlot *>(base + s.table);
    int *dropped_on = reinterpret_cast<int *>(base + s.dropped);
    unsigned long long *state = reinterpret_cast<unsigned long long *>(base + s.state);
    long long *pairs = reinterpret_cast<long long *>(base + s.pairs), *src_off = reinterpret_cast<long long *>(base + s.src_off);
    const long long *offs = reinterpret_cast<const long long *>(offsets);
    unsigned long long *collided = reinterpret_cast<unsigned long long *>(counts + 2);
    const int with_rc = reverse_complement != 0;
    const unsigned long long salt = fpr::salt_of(seed);

    hipError_t e = hipMemsetAsync(slots, 0xff, (size_t)16 << s.log2_slots, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(dropped_on, 0, (size_t)n_reads * sizeof(int), stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), stream);
    if (e != hipSuccess)
        return e;
    const dim3 wave_block(kWaveReadsPerBlock * 64);
    kmer_plan::for_each_wave_launch(n_reads, read_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        hipLaunchKernelGGL(dedup_fingerprint_kernel, dim3((unsigned)l.blocks), wave_block, 0, stream, bases + l.byte_at,
                           offsets ? offsets + l.first : nullptr, l.n, read_len, (unsigned long long)l.first, salt,
                           (unsigned long long)seed, with_rc, fp_bits, s.log2_slots, slots, state);
    });
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    kmer_plan::for_each_wave_launch(n_reads, read_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        hipLaunchKernelGGL(dedup_resolve_kernel, dim3((unsigned)l.blocks), wave_block, 0, stream, bases + l.byte_at,
                           offsets ? offsets + l.first : nullptr, l.n, read_len, (unsigned long long)l.first, bases, offsets,
                           with_rc, s.log2_slots, slots, state, dropped_on, collided);
    });
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    for (int64_t b0 = 0; b0 < s.n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, s.n_blocks));
        hipLaunchKernelGGL(dedup_flags_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           state, (long long)b0, pairs);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(dedup_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, pairs, (long long)s.n_blocks,
                       reinterpret_cast<long long *>(counts), reinterpret_cast<long long *>(out_offsets));
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    for (int64_t b0 = 0; b0 < s.n_blocks; b0 += kmer_plan::lane_blocks_per_launch()) {
        const dim3 grid((unsigned)kmer_plan::blocks_of_launch(b0, s.n_blocks));
        hipLaunchKernelGGL(dedup_place_kernel, grid, dim3(kThreads), 0, stream, offs, (long long)read_len, (long long)n_reads,
                           (unsigned long long)first_read, state, dropped_on, (long long)b0, pairs,
                           reinterpret_cast<long long *>(out_offsets), reinterpret_cast<long long *>(kept_index), copies, src_off);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (!offsets && read_len == 0)
        return hipSuccess; // nothing but empty reads: no byte to move
    return launch_gather_reads(bases, counts, offsets ? out_offsets : nullptr, read_len,
                               offsets ? -1 : n_reads * read_len, reinterpret_cast<const int64_t *>(src_off), out_bases, stream);
}

} // namespace covest
