// kmer_plan_check.cpp -- the host-side check of the partitioned k-mer counter's arithmetic (covest_amd/csrc/kmer_plan.h;
// DESIGN.md section 6q), compiled and run by tests/test_kmer_plan_cpu.py with the host compiler under
// -fsanitize=address,undefined.  No device: what the host plans and where it cuts its launches is plain C++.
#include <cstdio>
#include <cstdlib>

#include "kmer_plan.h"

using namespace covest;
using namespace covest::kmer_plan;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

// 1. Plans worked out by hand from the rules (m = min(k - 8, 13); buckets double from 2^10 while 2048 windows a bucket
// are not enough, up to 2^(2m - 3); the sample halves while the average bucket keeps six sampled records, from 4096
// blocks of reads on).
struct Pinned {
    int k;
    bool ragged;
    long long n_reads, len_or_total;
    int m, w, max_run, log2_buckets, sample;
};
static void check_plans()
{
    const Pinned pinned[] = {
        {21, false, 20000, 100, 13, 9, 12, 10, 1},
        {21, false, 100000, 100, 13, 9, 12, 12, 16},
        {21, false, 10000000, 100, 13, 9, 12, 19, 16},
        {21, false, 100000000, 100, 13, 9, 12, 22, 16},
        {19, false, 100000000, 100, 11, 9, 14, 19, 16}, // the 2m - 3 cap
        {19, false, 4000000, 50, 11, 9, 14, 16, 16},
        {31, false, 20000, 100, 13, 19, 2, 10, 1},
        {31, false, 10000000, 100, 13, 19, 2, 19, 16},
        {25, false, 1, 25, 13, 13, 8, 10, 1},
        {21, true, 4002, 300000, 13, 9, 12, 10, 1},
        {21, true, 3, 1, 13, 9, 12, 10, 1},
        {23, true, 26000000, 2600000000ll, 13, 11, 10, 21, 16},
    };
    for (const Pinned &c : pinned) {
        const Partition p = plan_partition(c.k, c.ragged, c.n_reads, c.ragged ? 0 : c.len_or_total, c.ragged ? c.len_or_total : 0);
        CHECK(p.m == c.m && p.w == c.w && p.max_run == c.max_run && p.log2_buckets == c.log2_buckets && p.sample == c.sample,
              "k %d %s (%lld, %lld): m %d w %d max_run %d log2_buckets %d sample %d", c.k, c.ragged ? "ragged" : "fixed",
              c.n_reads, c.len_or_total, p.m, p.w, p.max_run, p.log2_buckets, p.sample);
    }
    // no reads behind offsets: the caller's hint sizes the buckets, but there are no bytes to sample
    CHECK(plan_partition(21, true, 0, 0, 1ll << 33).sample == 1 && plan_partition(21, true, 0, 0, 1ll << 33).log2_buckets == 22,
          "no reads");
    for (int w = 2; w <= 24; ++w) {
        CHECK(tile_windows(w) == (w <= 17 ? 240 : 256 - (w - 1)), "tile_windows(%d) = %d", w, tile_windows(w));
        CHECK(block_bytes(w) == 8 * tile_windows(w), "block_bytes(%d)", w);
    }
    CHECK(tile_windows(19) == 238 && block_bytes(9) == 1920 && block_bytes(19) == 1904, "geometry");
}

// 2. The sizes that follow from pass 0 and pass 2, and the tables'.
static int64_t hand_back_in_double(uint64_t listed, uint64_t overflowed, int max_run) // the comparison as it was made before
{
    const double want = 2.0 * ((double)listed + (double)overflowed * (double)max_run) + 1024.0;
    int lg = 10;
    while (lg < 40 && (double)((int64_t)1 << lg) < want)
        ++lg;
    return (int64_t)1 << lg;
}

static void check_sizes()
{
    CHECK(overflow_cap_for(0) == 64 && overflow_cap_for(32767) == 64 && overflow_cap_for(32768) == 64, "overflow_cap_for: floor");
    CHECK(overflow_cap_for(4000000) == 7812 && overflow_cap_for(800000000) == 1562500, "overflow_cap_for");
    CHECK(small_buckets(128 * 1024, 1024) && !small_buckets(128 * 1024 + 1, 1024), "small_buckets");
    CHECK(records_bytes_wanted(1000, 64) == (1000.0 + 64.0 * 64.0) * 16.0, "records_bytes_wanted");
    CHECK(log2_slots_for(-5, 40) == 10 && log2_slots_for(0, 40) == 10 && log2_slots_for(1024, 40) == 10, "log2_slots_for: floor");
    CHECK(log2_slots_for(1025, 40) == 11 && log2_slots_for(1 << 20, 40) == 20 && log2_slots_for((1 << 20) + 1, 38) == 21,
          "log2_slots_for: exact powers stay");
    CHECK(log2_slots_for((int64_t)1 << 62, 40) == 40 && log2_slots_for((int64_t)1 << 62, 38) == 38 &&
              log2_slots_for(((int64_t)1 << 38) + 1, 38) == 38 && log2_slots_for(((int64_t)1 << 38) + 1, 40) == 39,
          "log2_slots_for: caps");
    const int words[][2] = {{1, 0}, {31, 0}, {32, 2}, {63, 2}, {64, 4}, {127, 4}, {128, 8}, {255, 8}};
    for (const auto &kw : words)
        CHECK(kmer_wide_words(kw[0]) == kw[1], "kmer_wide_words(%d)", kw[0]);
    // hand_back_slots: 2 s + 1024 passes 2^p at s = 2^(p - 1) - 512; one below, at, one above, for every way to make s
    for (int p = 10; p <= 37; ++p)
        for (int d = -1; d <= 1; ++d) {
            const int64_t s = ((int64_t)1 << (p - 1)) - 512 + d;
            if (s < 0)
                continue;
            for (const int max_run : {2, 12, 14}) {
                const uint64_t by_records = (uint64_t)s / max_run, rest = (uint64_t)s % max_run;
                CHECK(hand_back_slots((uint64_t)s, 0, max_run) == hand_back_in_double((uint64_t)s, 0, max_run), "s %lld listed",
                      (long long)s);
                CHECK(hand_back_slots(rest, by_records, max_run) == hand_back_in_double(rest, by_records, max_run),
                      "s %lld overflowed, max_run %d", (long long)s, max_run);
                CHECK(hand_back_slots((uint64_t)s, 0, max_run) == (int64_t)1 << (d <= 0 ? p : p + 1), "s %lld: %lld slots",
                      (long long)s, (long long)hand_back_slots((uint64_t)s, 0, max_run));
            }
        }
    CHECK(hand_back_slots(0, 0, 12) == 1024 && hand_back_slots(1, 0, 12) == 2048 && hand_back_slots((uint64_t)1 << 45, 0, 12) == (int64_t)1 << 40,
          "hand_back_slots: floor and cap");
}

// 3. The launch cuts: totals just below, at and above each multiple of a launch's size, up to three launches.
static void check_fixed(int64_t len, int w)
{
    const int64_t per = fixed_reads_per_launch(len);
    CHECK(per >= 1 && per * len <= (int64_t)1 << 31 && (per + 1) * len > (int64_t)1 << 31, "len %lld", (long long)len);
    const int64_t totals[] = {1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per - 1, 3 * per};
    for (const int64_t n_reads : totals) {
        if (n_reads < 1)
            continue;
        int64_t next = 0;
        int launches = 0;
        for (int64_t first = 0; first < n_reads; first += per, ++launches) {
            const FixedLaunch l = fixed_launch(first, n_reads, len, w);
            CHECK(first == next && l.n >= 1, "len %lld n_reads %lld first %lld", (long long)len, (long long)n_reads, (long long)first);
            next = first + l.n;
            CHECK(l.positions == (uint64_t)(l.n * len) && l.positions < (uint64_t)1 << 32, "len %lld n_reads %lld: positions",
                  (long long)len, (long long)n_reads);
            CHECK(l.avail == (uint64_t)((n_reads - first) * len) && l.avail >= l.positions, "len %lld n_reads %lld: avail",
                  (long long)len, (long long)n_reads);
            CHECK(l.n_tiles * tile_windows(w) >= l.positions && (l.n_tiles - 1) * tile_windows(w) < l.positions &&
                      l.n_tiles < (uint64_t)1 << 32,
                  "len %lld n_reads %lld: n_tiles", (long long)len, (long long)n_reads);
        }
        CHECK(next == n_reads && launches == (n_reads + per - 1) / per && launches <= 3, "len %lld n_reads %lld: %d launches end at %lld",
              (long long)len, (long long)n_reads, launches, (long long)next);
    }
}

static void check_ragged(int w)
{
    const int64_t cut = ragged_bytes_per_launch(w), block = block_bytes(w);
    CHECK(cut % block == 0 && cut <= (int64_t)1 << 31 && cut + block > (int64_t)1 << 31, "w %d: cut", w);
    const int64_t totals[] = {1, 19, 100, (1 << 30) - 1, cut - 1, cut, cut + 1, 2 * cut - 1, 2 * cut, 2 * cut + 1, 3 * cut - 1, 3 * cut};
    for (const int64_t total : totals) {
        int64_t next = 0;
        int launches = 0;
        for (int64_t pos0 = 0; pos0 < total; pos0 += cut, ++launches) {
            const RaggedLaunch l = ragged_launch(pos0, total, w);
            CHECK(pos0 == next && l.positions >= 1 && l.positions <= cut, "w %d total %lld pos0 %lld", w, (long long)total, (long long)pos0);
            next = pos0 + l.positions;
            CHECK(l.positions % block == 0 || next == total, "w %d total %lld: a launch that is not the last ends inside a block", w,
                  (long long)total);
            CHECK((int64_t)l.n_tiles * tile_windows(w) >= l.positions && ((int64_t)l.n_tiles - 1) * tile_windows(w) < l.positions,
                  "w %d total %lld: n_tiles", w, (long long)total);
            CHECK(ragged_tiles(total, w) >= (int64_t)l.n_tiles, "w %d total %lld: the first-read table is short", w, (long long)total);
        }
        CHECK(next == total && launches == (total + cut - 1) / cut && launches <= 3, "w %d total %lld: %d launches end at %lld", w,
              (long long)total, launches, (long long)next);
    }
}

// A lane a read: 2^22 workgroups a launch -- 2^30 threads of 256 -- so 2^22 blocks are one launch and one more is two.
static void check_lane_blocks()
{
    const int64_t per = lane_blocks_per_launch();
    CHECK(per == (int64_t)1 << 22 && per * 256 == (int64_t)1 << 30, "lane_blocks_per_launch %lld", (long long)per);
    const int64_t totals[] = {1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per};
    for (const int64_t n_blocks : totals) {
        int64_t next = 0;
        int launches = 0;
        for (int64_t b0 = 0; b0 < n_blocks; b0 += per, ++launches) {
            const int64_t n = blocks_of_launch(b0, n_blocks);
            CHECK(b0 == next && n >= 1 && n <= per, "n_blocks %lld b0 %lld: %lld blocks", (long long)n_blocks, (long long)b0, (long long)n);
            CHECK(n == per || b0 + n == n_blocks, "n_blocks %lld b0 %lld: a launch that is not the last is not full", (long long)n_blocks,
                  (long long)b0);
            next = b0 + n;
        }
        CHECK(next == n_blocks && launches == (n_blocks + per - 1) / per, "n_blocks %lld: %d launches end at %lld", (long long)n_blocks,
              launches, (long long)next);
    }
    CHECK(blocks_of_launch(0, per) == per && blocks_of_launch(0, per + 1) == per && blocks_of_launch(per, per + 1) == 1,
          "2^22 blocks and one more");
}

int main()
{
    check_plans();
    check_sizes();
    for (const int w : {9, 11, 19})
        for (const int64_t len : {(int64_t)19, (int64_t)100, ((int64_t)1 << 30) - 1})
            check_fixed(len, w);
    for (const int w : {9, 11, 17, 18, 19})
        check_ragged(w);
    check_lane_blocks();
    std::printf("kmer_plan ok\n");
    return 0;
}
