// kmer_plan.h -- the arithmetic of the partitioned k-mer counter (kmer_host.cpp, kmer_bulk.hip) in plain C++: table
// sizes, the tile geometry, the launch cuts (and the walk over the launches of a wave a read, for_each_wave_launch; the
// launchers of the adds and removals over both: kmer_update.h launch_update), the plan of a call, the sizes that follow
// from pass 0.  No HIP in it: tests/kmer_plan_check.cpp and, for the launch cuts
// and the walk, tests/kmer_stages_check.cpp run it under the host compiler's sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>

#ifdef __HIPCC__
#define KMER_PLAN_HD __host__ __device__
#else
#define KMER_PLAN_HD
#endif

namespace covest {

constexpr int kOvfShards = 64, kOvfStride = 16; // parts of the overflow list; 64-bit words between their counters

namespace kmer_plan {

// ---- tables in HBM -------------------------------------------------------------------------------------------------
// log2 of the smallest power of two >= min_slots, from 2^10 up to 2^cap
inline int log2_slots_for(int64_t min_slots, int cap)
{
    int lg = 10;
    while (((int64_t)1 << lg) < min_slots && lg < cap)
        ++lg;
    return lg;
}

// 64-bit words of a key of kmer_wide.hip (0: k <= 31, the one-word table of kmer_count.hip)
inline int kmer_wide_words(int k)
{
    return k <= 31 ? 0 : k <= 63 ? 2 : k <= 127 ? 4 : 8;
}

// ---- the table paths' launches (kmer_update.h, for kmer_count.hip, kmer_remove.hip, kmer_wide.hip): whole reads, `per` a launch ----
// A wave a read, reads_per_block reads a workgroup: HIP wraps a grid of more than 2^32 threads silently, so at most
// 2^23 workgroups of 256 threads a launch (called by for_each_wave_launch below alone).
inline int64_t wave_reads_per_launch(int reads_per_block)
{
    return (int64_t)reads_per_block << 23;
}

// A thread a window, the windows of reads of one length numbered through: a launch's windows, rounded up to workgroups
// of 256, stay below 2^31.
inline int64_t window_reads_per_launch(int64_t n_windows)
{
    return std::max<int64_t>(1, (((int64_t)1 << 31) - 256) / n_windows);
}

inline int64_t reads_of_launch(int64_t first, int64_t n_reads, int64_t per) // reads of the launch that starts at `first`
{
    return std::min(n_reads - first, per);
}

// One launch of a wave a read (wave_read.h): what its launcher hands the kernel follows from `first` and `byte_at` alone.
struct WaveLaunch {
    int64_t first, n; // reads first .. first + n - 1
    int64_t byte_at; // with offsets 0 (the reads say where they are themselves), else first * fixed_len
    int64_t blocks;  // ceil(n / reads_per_block) workgroups, at most 2^23
};
template <class F> void for_each_wave_launch(int64_t n_reads, int64_t fixed_len, bool has_offsets, int reads_per_block, F &&f)
{
    const int64_t per = wave_reads_per_launch(reads_per_block);
    for (int64_t first = 0; first < n_reads; first += per) {
        const int64_t n = reads_of_launch(first, n_reads, per);
        f(WaveLaunch{first, n, has_offsets ? 0 : first * fixed_len, (n + reads_per_block - 1) / reads_per_block});
    }
}

// A weighted add (covest_kmer_add_weighted*) has a weight a READ, indexed like the call's reads: the entry a launch's
// kernel starts from.  A wave-a-read launch indexes its reads from l.first on -- whatever byte_at says: with offsets the
// bytes do not advance, the reads still do --, the windows-numbered-through loop from its own `first`.
inline int64_t weights_at(const WaveLaunch &l)
{
    return l.first;
}

inline int64_t window_weights_at(int64_t first) // `first`: the read a launch of the windows numbered through starts at
{
    return first;
}

// A lane a read (or a few), workgroups of 256 threads (sample_reads.hip, split_reads.hip): 2^22 workgroups, 2^30 threads,
// a launch, for the same wrap.
inline int64_t lane_blocks_per_launch()
{
    return (int64_t)1 << 22;
}

inline int64_t blocks_of_launch(int64_t b0, int64_t n_blocks) // workgroups of the launch that starts at workgroup b0
{
    return std::min(n_blocks - b0, lane_blocks_per_launch());
}

// ---- pass 0 / 1: tiles of kTile bytes, kTilesPerBlock of them a workgroup --------------------------------------------
constexpr int kTile = 256;        // bytes (threads) of a tile
constexpr int kTilesPerBlock = 8; // consecutive tiles a workgroup works through (the unit of pass 0's sample)

// window starts a tile answers for: its last max(16, w - 1) bytes are the halo of the windows before them
KMER_PLAN_HD inline int tile_windows(int w)
{
    return kTile - std::max(16, w - 1);
}

KMER_PLAN_HD inline int block_bytes(int w) // bytes of the read array a workgroup answers for
{
    return kTilesPerBlock * tile_windows(w);
}

// Reads of one length go in launches of whole reads, their bytes (and the tiles' halo) below 2^32.
inline int64_t fixed_reads_per_launch(int64_t len)
{
    return std::max<int64_t>(1, ((int64_t)1 << 31) / len);
}

struct FixedLaunch {
    int64_t n;          // reads of this launch, from `first` on
    uint64_t positions; // their bytes
    uint64_t avail;     // bytes that may be read from the launch's first on: to the end of the array
    uint64_t n_tiles;
};
inline FixedLaunch fixed_launch(int64_t first, int64_t n_reads, int64_t len, int w)
{
    FixedLaunch l;
    l.n = std::min(n_reads - first, fixed_reads_per_launch(len));
    l.positions = (uint64_t)(l.n * len);
    l.avail = (uint64_t)((n_reads - first) * len);
    l.n_tiles = (l.positions + tile_windows(w) - 1) / tile_windows(w);
    return l;
}

// Reads of any length go as one run of bytes, in launches of whole blocks of tiles below 2^31 bytes each.
inline int64_t ragged_bytes_per_launch(int w)
{
    return (((int64_t)1 << 31) / block_bytes(w)) * block_bytes(w);
}

struct RaggedLaunch {
    int64_t positions; // bytes of this launch, from pos0 on
    uint64_t n_tiles;
};
inline RaggedLaunch ragged_launch(int64_t pos0, int64_t total, int w)
{
    RaggedLaunch l;
    l.positions = std::min(total - pos0, ragged_bytes_per_launch(w));
    l.n_tiles = (uint64_t)((l.positions + tile_windows(w) - 1) / tile_windows(w));
    return l;
}

// words of the tiles' first-read table: a word per tile of the largest launch (and one to spare)
inline int64_t ragged_tiles(int64_t total, int w)
{
    return (std::min(total, ragged_bytes_per_launch(w)) + tile_windows(w) - 1) / tile_windows(w) + 1;
}

// ---- the plan of a call --------------------------------------------------------------------------------------------
struct Partition {
    int m, w, max_run; // minimizer length, m-mers per k-mer (k - m + 1), windows per record (a record holds 32 bases)
    int log2_buckets;
    int sample;        // pass 0 looks at 1 block of tiles (1 read) in `sample`
};

// windows (an upper bound for reads of different lengths: every base starts at most one)
inline double plan_windows(int k, bool ragged, int64_t n_reads, int64_t read_len, int64_t total_bases)
{
    return ragged ? (double)std::max<int64_t>(total_bases, n_reads) : (double)n_reads * (double)(read_len - k + 1);
}

inline double plan_bytes(bool ragged, int64_t n_reads, int64_t read_len, int64_t total_bases)
{
    // (no reads: no bytes, whatever the caller said of them -- total_bases is then the caller's hint)
    return ragged ? (n_reads > 0 ? (double)total_bases : 0.0) : (double)n_reads * (double)read_len;
}

// pass 0 looks at everything when that is little, else at one block of tiles (one read) in 2 .. 16: as thin a sample as
// leaves the average bucket six sampled records (a record per ~5 windows) -- the room is the estimate plus three of its
// standard deviations, and below that the estimate is mostly deviation (1 Gbp with one block in 16: 2 % of the buckets
// overflowed their room and went through the table in HBM)
inline int sample_for(double windows, double bytes, int w, int log2_buckets)
{
    const double per_bucket = windows / 5.0 / (double)((int64_t)1 << log2_buckets);
    int thin = 1;
    while (thin < 16 && (double)(2 * thin) * 6.0 <= per_bucket)
        thin *= 2;
    const bool large = bytes / (double)block_bytes(w) >= 4096.0;
    return large ? thin : 1;
}

// ragged: reads with offsets (total_bases = offsets[n_reads] - offsets[0]), else n_reads reads of read_len bases
inline Partition plan_partition(int k, bool ragged, int64_t n_reads, int64_t read_len, int64_t total_bases)
{
    const double windows = plan_windows(k, ragged, n_reads, read_len, total_bases);
    Partition p;
    p.m = std::min(k - 8, 13);
    p.w = k - p.m + 1;
    p.max_run = 32 - k + 1;
    // 1000-2000 windows per bucket, at least 2^10 buckets, at most an eighth of the minimizers there are.  Measured
    // (diagnostic build, COVEST_KMER_LG): 1 Gbp 2^22 / 2^21 / 2^20 / 2^19 buckets 20.3 / 18.2 / 17.8 / 16.5 ms, 10 Gbp
    // 2^25 / 2^24 / 2^23 / 2^22 / 2^21 205 / 174 / 141-155 / 143-145 / 146 ms: fewer, fuller buckets keep the sectors
    // that pass 1 writes into within the caches' reach and the sample of pass 0 thin; a bucket of 2000 windows still
    // fits a workgroup's LDS table when every one of them is a different key.
    p.log2_buckets = 10;
    while (p.log2_buckets < 2 * p.m - 3 && (double)((int64_t)1 << p.log2_buckets) * 2048.0 < windows)
        ++p.log2_buckets;
    p.sample = sample_for(windows, plan_bytes(ragged, n_reads, read_len, total_bases), p.w, p.log2_buckets);
    return p;
}

// ---- what follows from pass 0's room (records the buckets were given places for) and from pass 2 ----------------------
inline uint64_t overflow_cap_for(uint64_t room) // records per part of the overflow list
{
    return std::max<uint64_t>(4096, room / 8) / kOvfShards;
}

inline bool small_buckets(uint64_t room, uint64_t n_buckets) // pass 2 with LDS tables of half the size
{
    return (double)room <= 128.0 * (double)n_buckets;
}

inline double records_bytes_wanted(uint64_t room, uint64_t overflow_cap) // of 16-byte records, buckets and list
{
    return ((double)room + (double)overflow_cap * kOvfShards) * 16.0;
}

// Slots of the table in HBM for what pass 2 hands back: twice the k-mers of the listed buckets and of the records
// that overflowed (max_run each at most), and 1024.  The parent compared in double, (double)2^lg < 2.0 * ((double)
// listed + (double)overflowed * (double)max_run) + 1024.0: both counts are of things in device memory, below 2^40, so
// every term and the sum are integers below 2^53, the double arithmetic was exact, and the integers compare alike.
inline int64_t hand_back_slots(uint64_t listed_kmers, uint64_t n_overflowed, int max_run)
{
    return (int64_t)1 << log2_slots_for((int64_t)(2 * (listed_kmers + n_overflowed * (uint64_t)max_run) + 1024), 40);
}

} // namespace kmer_plan
} // namespace covest
