// kmer_bulk.hip -- K-kmer, partitioned: the whole of bin/kmer_hist.py's main loop (:77-89: compute_counts over every
// read, then compute_histogram) for reads resident in HBM, WITHOUT a table in HBM.
//
// K-kmer's table (kmer_count.hip) pays one scattered memory-side operation pair per k-mer OCCURRENCE: 2e10 a
// second, whatever the table's size (tools/microbench_atomics.hip).  Here an occurrence costs LDS work only:
//
//   pass 0  (kmer_scatter.h: kmer_tile_kernel<COUNT>; kmer_place.h: kmer_caps_*)   the records pass 1 will write,
//           counted per bucket on a SAMPLE of
//           the reads (1 block of tiles in `sample`; everything when the input is small), turned into room per bucket
//           (the estimate plus three standard deviations) and, by a prefix sum, into the buckets' places in ONE array:
//           minimizers are far from equally frequent, a fixed room per bucket would be wasted on most and short for some.
//   pass 1  (kmer_scatter.h: kmer_tile_kernel<SCATTER>)   every window's MINIMIZER -- the m-mer of smallest hash among
//           the k - m + 1 it holds, canonical when the keys are -- names a BUCKET, a function of the k-mer alone: every occurrence
//           of a key lands in the same bucket.  Consecutive windows of a read mostly share their minimizer: the runs
//           of equal bucket ("super-k-mers") become ONE 16-byte record each -- the run's bases as 2-bit codes and their
//           number -- behind the bucket's cursor: one returning atomic and one store per ~5 windows, 6 bytes of HBM
//           traffic per k-mer instead of 16 scattered ones.  A workgroup works through tiles of 256 consecutive BYTES
//           of the read array: every thread packs the 16 bases from its byte on (one unaligned 16-byte load), hashes the
//           m-mer that starts there ONCE (LDS), and the window's minimizer is the smallest of w neighbouring entries.
//   pass 2  (kmer_lds_count.h: kmer_wave_count_kernel)   one WAVE per bucket, no barrier anywhere: the records' k-mers go
//           into the wave's own hash table in LDS (1024 slots; 64-bit compare-and-swap on the key, 32-bit add on the count), the table
//           is swept into the workgroup's count-of-counts bins (LDS too, flushed once at the end).  Twelve waves a CU
//           hide each other's latency.  (kmer_bucket_count_kernel)  the few buckets with too many records or too many
//           distinct keys for that: a workgroup each, 4096 slots.
//
// Exact by construction -- and by a fall-back for everything that does not fit: a bucket that overflows its room in
// HBM (the sample misjudged it), a bucket whose distinct keys do not fit the LDS tables: all of THAT bucket's k-mers
// (records in place and records in the overflow list alike -- a key must be counted in one place only) go to the
// open-addressing table of kmer_count.hip, whose histogram is added at the end (the to-table kernels below).
//
// Reference restated: bin/kmer_hist.py:18-41 (codes, counts), :57-64 (count-of-counts); `canonical` as in kmer_count.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "kmer_lds_count.h"
#include "kmer_place.h"
#include "kmer_scatter.h"
#include "kmer_table.h"
#include "wave.h"

namespace covest {

namespace {

// ---- what no LDS table could hold: into the table in HBM -------------------------------------------------------------
// Every k-mer of a record into the table.
__device__ __forceinline__ void record_to_table(ulonglong2 rec, const KmerBulk &p, const KmerTable &t, int *overflow)
{
    const int n_k = (int)rec.y - p.k + 1;
    for (int j = 0; j < n_k; ++j) {
        u64 h, rc;
        codes_from_le(low_bases(rec.x >> (2 * j), p.k), p.k, h, rc);
        canonical_pair(h, rc, p.canonical);
        table_add(t, h, rc, 1ull, overflow);
    }
}

// The buckets no LDS table could hold: their records' k-mers.
__global__ __launch_bounds__(256) void kmer_buckets_to_table_kernel(const KmerBulk p, const KmerTable t, int *overflow,
                                                                    const u64 *__restrict__ to_table,
                                                                    const unsigned *__restrict__ to_table_list)
{
    const unsigned n_listed = (unsigned)to_table[0];
    for (unsigned at = blockIdx.x; at < n_listed; at += gridDim.x) {
        const unsigned b = to_table_list[at];
        const ulonglong2 c = p.ctl[b];
        const u64 filled = p.fill[b], room = c.y - c.x;
        const u64 n = filled < room ? filled : room;
        for (u64 i = threadIdx.x; i < n; i += blockDim.x)
            record_to_table(p.recs[c.x + i], p, t, overflow);
    }
}

// The records that found their bucket full: their k-mers (their buckets' other records follow in pass 2).
__global__ __launch_bounds__(256) void kmer_overflow_to_table_kernel(const KmerBulk p, const KmerTable t, int *overflow)
{
    const unsigned shard = blockIdx.y; // (a part of the list per grid row)
    const u64 n = min(p.ovf_count[shard * kOvfStride], p.overflow_cap);
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        record_to_table(p.overflow[shard * p.overflow_cap + i], p, t, overflow);
}

// What bounds pass 1, measured: returning 64-bit atomic adds at pseudo-random places of `slots` words -- a wave
// instruction's 64 lanes all on different lines, as the records of a tile are.
__global__ __launch_bounds__(256) void kmer_scatter_rate_kernel(u64 *__restrict__ words, u64 slots, int per_thread,
                                                                u64 *__restrict__ sink)
{
    u64 x = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    u64 acc = 0;
    for (int i = 0; i < per_thread; ++i) {
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        x ^= x >> 32;
        acc += atomicAdd(&words[x % slots], 1ull);
    }
    if (acc == ~0ull)
        sink[0] = acc; // (never: keeps the returned values alive)
}

// out[0] = 0 if some read is not offsets[1] - offsets[0] bases long (out comes in as 1)
__global__ __launch_bounds__(256) void kmer_one_length_kernel(const int64_t *__restrict__ offsets, int64_t n_reads,
                                                              unsigned long long *__restrict__ out)
{
    const int64_t len0 = offsets[1] - offsets[0];
    bool same = true;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * blockDim.x)
        same = same && offsets[r + 1] - offsets[r] == len0;
    if (__ballot(!same) != 0ull && (threadIdx.x & (kWave - 1)) == 0)
        out[0] = 0ull;
}

template <bool COUNT>
hipError_t launch_tiles(const unsigned char *bases, int64_t n_reads, int64_t len, const KmerBulk &p, hipStream_t stream)
{
    for (int64_t first = 0; first < n_reads; first += kmer_plan::fixed_reads_per_launch(len)) {
        const kmer_plan::FixedLaunch l = kmer_plan::fixed_launch(first, n_reads, len, p.w);
        uint64_t blocks = (l.n_tiles + kTilesPerBlock - 1) / kTilesPerBlock;
        if (COUNT)
            blocks = (blocks + p.sample - 1) / p.sample;
        hipLaunchKernelGGL((kmer_tile_kernel<COUNT, false>), dim3((unsigned)blocks), dim3(kTile), 0, stream,
                           bases + first * len, (unsigned)l.positions, (u64)l.avail, (unsigned)len, (unsigned)l.n_tiles, p,
                           RaggedReads{});
    }
    return hipGetLastError();
}

// Reads of any length: the byte run offsets[0] .. offsets[n_reads] in launches of whole blocks of tiles (below 2^31
// bytes each; a launch need not end with a read: a window belongs to the launch its first byte is in).  first_read:
// room for a word per tile of the largest launch (kmer_plan::ragged_tiles).
template <bool COUNT>
hipError_t launch_ragged(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t base0, int64_t total,
                         unsigned *first_read, const KmerBulk &p, hipStream_t stream)
{
    for (int64_t pos0 = 0; pos0 < total; pos0 += kmer_plan::ragged_bytes_per_launch(p.w)) {
        const kmer_plan::RaggedLaunch l = kmer_plan::ragged_launch(pos0, total, p.w);
        const uint64_t n_tiles = l.n_tiles;
        uint64_t blocks = (n_tiles + kTilesPerBlock - 1) / kTilesPerBlock;
        RaggedReads src{offsets, n_reads, base0, pos0, first_read};
        // (both passes make the table again: a launch's table is gone once the next launch has made its own)
        hipLaunchKernelGGL(kmer_tile_first_read_kernel, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, stream, src,
                           (unsigned)n_tiles, kmer_plan::tile_windows(p.w), first_read);
        if (COUNT)
            blocks = (blocks + p.sample - 1) / p.sample;
        hipLaunchKernelGGL((kmer_tile_kernel<COUNT, true>), dim3((unsigned)blocks), dim3(kTile), 0, stream,
                           bases + base0 + pos0, (unsigned)l.positions, (u64)(total - pos0), 0u, (unsigned)n_tiles, p, src);
    }
    const int64_t step = COUNT ? p.sample : 1;
    const int64_t threads = (n_reads + step - 1) / step;
    const int64_t per = (int64_t)1 << 30; // threads a launch
    for (int64_t first = 0; first < threads; first += per) {
        const int64_t n = std::min(threads - first, per);
        hipLaunchKernelGGL(kmer_short_reads_kernel<COUNT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, bases,
                           offsets + first * step, n_reads - first * step, p);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_kmer_scatter(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                               int64_t base0, int64_t total_bytes, unsigned *first_read, const KmerBulk &p, bool count_only,
                               hipStream_t stream)
{
    if (n_reads <= 0)
        return hipSuccess;
    if (!offsets) // (the host sends reads shorter than k to the table path)
        return count_only ? launch_tiles<true>(bases, n_reads, fixed_len, p, stream)
                          : launch_tiles<false>(bases, n_reads, fixed_len, p, stream);
    return count_only ? launch_ragged<true>(bases, offsets, n_reads, base0, total_bytes, first_read, p, stream)
                      : launch_ragged<false>(bases, offsets, n_reads, base0, total_bytes, first_read, p, stream);
}

// sampled[] -> ctl[] = {first place, end} of every bucket; total[0] = the records there is room for.  partial: a word
// per 1024 buckets.
hipError_t launch_kmer_place_buckets(const KmerBulk &p, unsigned long long *partial, unsigned long long *total,
                                     hipStream_t stream)
{
    const unsigned n_blocks = (1u << p.log2_buckets) / kScanBlock; // (at least 2^10 buckets)
    hipLaunchKernelGGL(kmer_caps_partial_kernel, dim3(n_blocks), dim3(256), 0, stream, p, partial);
    hipLaunchKernelGGL(kmer_caps_scan_kernel, dim3(1), dim3(256), 0, stream, partial, n_blocks, total);
    hipLaunchKernelGGL(kmer_caps_place_kernel, dim3(n_blocks), dim3(256), 0, stream, p, partial);
    return hipGetLastError();
}

hipError_t launch_kmer_one_length(const int64_t *offsets, int64_t n_reads, unsigned long long *out, hipStream_t stream)
{
    hipLaunchKernelGGL(kmer_one_length_kernel, dim3(1024), dim3(256), 0, stream, offsets, n_reads, out);
    return hipGetLastError();
}

hipError_t launch_kmer_scatter_rate(unsigned long long *words, unsigned long long slots, long long ops, unsigned long long *sink,
                                    hipStream_t stream)
{
    const int per_thread = 64;
    const long long threads = (ops + per_thread - 1) / per_thread;
    hipLaunchKernelGGL(kmer_scatter_rate_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, words, slots,
                       per_thread, sink);
    return hipGetLastError();
}

hipError_t launch_kmer_bucket_count(const KmerBulk &p, unsigned long long *hist, unsigned long long hist_len,
                                    unsigned long long *stats, unsigned long long *big, unsigned long long big_cap,
                                    unsigned *later, unsigned *later_list, unsigned long long *to_table, unsigned *to_table_list,
                                    bool small_buckets, int n_cu, hipStream_t stream)
{
    // A wave per bucket: three workgroups of four per CU with tables of 1024 slots (52 KB of LDS each) -- or five with
    // 512 slots where the buckets are small enough for them (1 Gbp: 7.2 -> 5.8 ms; the 200 records of a 10 Gbp bucket do
    // not fit: 44 -> 92 ms with half a million buckets left to the workgroups).  Then a workgroup per bucket left over.
    if (small_buckets)
        hipLaunchKernelGGL(kmer_wave_count_kernel<kWaveSlots / 2>, dim3((unsigned)(5 * n_cu)), dim3(256), 0, stream, p, hist,
                           hist_len, stats, big, big_cap, later, later_list);
    else
        hipLaunchKernelGGL(kmer_wave_count_kernel<kWaveSlots>, dim3((unsigned)(3 * n_cu)), dim3(256), 0, stream, p, hist, hist_len,
                           stats, big, big_cap, later, later_list);
    hipLaunchKernelGGL(kmer_bucket_count_kernel, dim3((unsigned)(3 * n_cu)), dim3(256), 0, stream, p, hist, hist_len, stats, big,
                       big_cap, later, later_list, to_table, to_table_list);
    return hipGetLastError();
}

hipError_t launch_kmer_to_table(const KmerBulk &p, bool any_overflowed, const KmerTable &t, int *overflow,
                                const unsigned long long *to_table, const unsigned *to_table_list, hipStream_t stream)
{
    if (any_overflowed)
        hipLaunchKernelGGL(kmer_overflow_to_table_kernel, dim3(64, kOvfShards), dim3(256), 0, stream, p, t, overflow);
    hipLaunchKernelGGL(kmer_buckets_to_table_kernel, dim3(2048), dim3(256), 0, stream, p, t, overflow, to_table, to_table_list);
    return hipGetLastError();
}

} // namespace covest
