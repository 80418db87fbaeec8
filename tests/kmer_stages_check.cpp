// kmer_stages_check.cpp -- the integer logic of the partitioned k-mer counter's kernels that the host compiler can build
// (covest_amd/csrc/kmer_codes.h, kmer_runs.h, and the table paths' launch cuts and launch walk of kmer_plan.h; DESIGN.md
// sections 6ad, 6aj),
// compiled and run by tests/test_kmer_plan_cpu.py under -fsanitize=address,undefined.  On the device a mistake in any of
// it shows only as a wrong histogram.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmer_codes.h"
#include "kmer_plan.h"
#include "kmer_runs.h"

using namespace covest;
using namespace covest::kmer;
typedef unsigned long long u64;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

static u64 rng_state = 0x2545F4914F6CDD1Dull;
static u64 rnd() // xorshift64*
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

// 1. Run lengths against a walk over the tile's 256 threads.  valid[t]: thread t starts a window; head[t]: ... and a
// run (a head is a window).  The run of head t: t and the threads behind it up to the next head, the first thread
// that starts no window, or the tile's end.
static void check_tile(const bool *valid, const bool *head, const char *what)
{
    u64 hm[kRunWaves] = {}, vm[kRunWaves] = {};
    for (int t = 0; t < kmer_plan::kTile; ++t) {
        hm[t / kRunWave] |= (u64)head[t] << (t % kRunWave);
        vm[t / kRunWave] |= (u64)valid[t] << (t % kRunWave);
    }
    int covered = 0, windows = 0;
    for (int t = 0; t < kmer_plan::kTile; ++t) {
        windows += valid[t];
        if (!head[t])
            continue;
        int want = 1;
        while (t + want < kmer_plan::kTile && valid[t + want] && !head[t + want])
            ++want;
        const int got = run_length(t % kRunWave, t / kRunWave, hm[t / kRunWave], vm[t / kRunWave], hm, vm);
        CHECK(got == want, "%s: thread %d: run %d, walked %d", what, t, got, want);
        covered += got;
    }
    CHECK(covered == windows, "%s: the runs hold %d of %d windows", what, covered, windows);
}

static void check_runs()
{
    bool valid[kmer_plan::kTile], head[kmer_plan::kTile];
    auto reset = [&](int n_win) {
        for (int t = 0; t < kmer_plan::kTile; ++t) {
            valid[t] = t < n_win;
            head[t] = false;
        }
        head[0] = true;
    };
    // a run that ends in its own wave, in a later wave (the next, and two on), at lane 63, at the halo
    reset(240);
    head[5] = head[40] = true;
    check_tile(valid, head, "same wave");
    reset(240);
    head[10] = head[70] = true;
    check_tile(valid, head, "next wave");
    reset(240);
    head[10] = head[200] = true;
    check_tile(valid, head, "two waves on");
    reset(240);
    head[63] = head[64] = head[127] = head[191] = true;
    check_tile(valid, head, "heads at lane 63");
    reset(240);
    head[62] = true;
    valid[64] = false;
    head[65] = true;
    check_tile(valid, head, "a read ends at lane 63");
    reset(240);
    check_tile(valid, head, "one run to the halo");
    reset(238);
    head[237] = true;
    check_tile(valid, head, "a run of one before the halo");
    // nowhere: every thread of the tile a window (no geometry has that; the walk over the waves then ends with the tile)
    reset(256);
    check_tile(valid, head, "one run to the tile's end");
    reset(256);
    head[255] = head[192] = true;
    check_tile(valid, head, "heads in the last wave, to the tile's end");
    // seeded random tiles: windows in stretches (reads), heads at a stretch's first window and at random ones
    for (int trial = 0; trial < 4000; ++trial) {
        const int n_win = trial % 3 == 0 ? 256 : trial % 3 == 1 ? 240 : 238;
        const unsigned gap_1_in = 2 + (unsigned)(rnd() % 60), head_1_in = 1 + (unsigned)(rnd() % 40);
        for (int t = 0; t < kmer_plan::kTile; ++t) {
            valid[t] = t < n_win && rnd() % gap_1_in != 0;
            head[t] = valid[t] && (t == 0 || !valid[t - 1] || rnd() % head_1_in == 0);
        }
        check_tile(valid, head, "random tile");
    }
}

// 2. The pieces of a run cover it exactly once, in order, each within a record's 32 bases.
static void check_pieces()
{
    for (int k = 19; k <= 31; ++k) {
        const int max_run = 32 - k + 1;
        for (int run = 1; run <= 240; ++run) {
            int next = 0, n = 0;
            for_each_piece(run, max_run, k, [&](int first, int n_bases) {
                CHECK(first == next, "k %d run %d: piece %d starts at %d, not %d", k, run, n, first, next);
                CHECK(n_bases >= k && n_bases <= 32, "k %d run %d: piece %d of %d bases", k, run, n, n_bases);
                next = first + n_bases - k + 1;
                CHECK(next == run || n_bases - k + 1 == max_run, "k %d run %d: piece %d is short and not the last", k, run, n);
                ++n;
            });
            CHECK(next == run, "k %d run %d: the pieces end at window %d", k, run, next);
            CHECK(n == pieces_of(run, max_run), "k %d run %d: %d pieces, %d counted", k, run, n, pieces_of(run, max_run));
        }
    }
}

// 3. The pair reversals against the base-by-base loops, at every length.
static u64 reversed_base_by_base(u64 x, int n) // base j of x to place n - 1 - j
{
    u64 out = 0;
    for (int j = 0; j < n; ++j)
        out |= ((x >> (2 * j)) & 3ull) << (2 * (n - 1 - j));
    return out;
}

static void check_codes()
{
    for (int n = 1; n <= 32; ++n)
        for (int trial = 0; trial < 300; ++trial) {
            u64 x = trial == 0 ? 0ull : trial == 1 ? ~0ull : trial == 2 ? 0x1B1B1B1B1B1B1B1Bull : rnd();
            x = low_bases(x, n);
            CHECK(n == 32 || x >> (2 * n) == 0, "low_bases(%d)", n);
            CHECK(reverse_pairs64(x) >> (64 - 2 * n) == reversed_base_by_base(x, n), "reverse_pairs64, %d bases, %llx", n, x);
            CHECK(reverse_pairs64(~x) >> (64 - 2 * n) == revcomp_code(x, n), "reverse complement at 64 bits, %d bases, %llx", n, x);
            if (n <= 16) {
                const unsigned y = (unsigned)x;
                CHECK(reverse_pairs32(y) >> (32 - 2 * n) == (unsigned)reversed_base_by_base(x, n), "reverse_pairs32, %d bases, %x", n, y);
                CHECK(reverse_pairs32(~y) >> (32 - 2 * n) == (unsigned)revcomp_code(x, n), "reverse complement at 32 bits, %d bases, %x",
                      n, y);
            }
            CHECK(revcomp_code(revcomp_code(x, n), n) == x, "revcomp_code twice, %d bases", n);
        }
    CHECK(low_bases(~0ull, 32) == ~0ull && low_bases(~0ull, 31) == ~0ull >> 2 && low_bases(~0ull, 1) == 3ull, "low_bases");
    CHECK(kmer_mask(19) == (1ull << 38) - 1ull && kmer_mask(32) == ~0ull, "kmer_mask");
    // the bases: a=0 c=1 g=2 t=3 in either case, four at a time as one at a time
    const char *acgt = "acgtACGT";
    for (int i = 0; i < 8; ++i)
        CHECK(base_code((unsigned char)acgt[i]) == (unsigned)(i % 4), "base_code(%c)", acgt[i]);
    for (int trial = 0; trial < 256; ++trial) {
        unsigned word = 0, want = 0;
        for (int j = 0; j < 4; ++j) {
            const unsigned char ch = (unsigned char)acgt[((trial >> (2 * j)) & 3) + 4 * (j & 1)]; // (lower and upper case)
            word |= (unsigned)ch << (8 * j);
            want |= base_code(ch) << (2 * j);
        }
        CHECK(pack4(word) == want, "pack4(%08x) = %x, base by base %x", word, pack4(word), want);
    }
    // lds_slot stays inside the table, whatever its size, and uses both halves of the key
    for (unsigned slots = 64; slots <= 4096; slots <<= 1) {
        std::vector<int> hit(slots, 0);
        for (int trial = 0; trial < 20000; ++trial) {
            const u64 key = trial < 64 ? 1ull << trial : rnd();
            const unsigned at = lds_slot(key, slots - 1u);
            CHECK(at < slots, "lds_slot(%llx, %u) = %u", key, slots - 1u, at);
            ++hit[at];
        }
        int used = 0;
        for (const int h : hit)
            used += h > 0;
        CHECK(2 * used > (int)slots, "lds_slot: 20000 keys reach %d of %u slots", used, slots);
    }
    CHECK(lds_slot(1ull << 40, 4095u) != lds_slot(0ull, 4095u) && lds_slot(1ull, 4095u) != lds_slot(0ull, 4095u), "lds_slot: halves");
}

// 4. The table paths' launch cuts tile n_reads exactly once, around each multiple of a launch.
static void check_cut(int64_t per, const char *what)
{
    CHECK(per >= 1, "%s: %lld reads a launch", what, (long long)per);
    const int64_t totals[] = {1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per - 1, 3 * per};
    for (const int64_t n_reads : totals) {
        if (n_reads < 1)
            continue;
        int64_t next = 0;
        int launches = 0;
        for (int64_t first = 0; first < n_reads; first += per, ++launches) {
            const int64_t n = kmer_plan::reads_of_launch(first, n_reads, per);
            CHECK(first == next && n >= 1 && n <= per, "%s n_reads %lld first %lld: %lld reads", what, (long long)n_reads,
                  (long long)first, (long long)n);
            next = first + n;
        }
        CHECK(next == n_reads && launches == (n_reads + per - 1) / per && launches <= 3, "%s n_reads %lld: %d launches end at %lld",
              what, (long long)n_reads, launches, (long long)next);
    }
}

// 5. The walk the launchers of a wave a read make (for_each_wave_launch): the visits tile n_reads exactly once, a
// launch's bytes begin where its reads do (0 with offsets), its workgroups hold its reads and are at most 2^23.
static void check_wave_walk(int reads_per_block)
{
    const int64_t per = kmer_plan::wave_reads_per_launch(reads_per_block), fixed_len = 100;
    const int64_t totals[] = {0, 1, reads_per_block, reads_per_block + 1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1,
                              3 * per - 1, 3 * per};
    for (const int64_t n_reads : totals)
        for (const bool has_offsets : {false, true}) {
            int64_t next = 0;
            int launches = 0;
            kmer_plan::for_each_wave_launch(n_reads, fixed_len, has_offsets, reads_per_block, [&](const kmer_plan::WaveLaunch &l) {
                CHECK(l.first == next && l.n >= 1, "walk(%d) n_reads %lld offsets %d: first %lld, %lld reads", reads_per_block,
                      (long long)n_reads, (int)has_offsets, (long long)l.first, (long long)l.n);
                CHECK(l.byte_at == (has_offsets ? 0 : l.first * fixed_len), "walk(%d) n_reads %lld offsets %d first %lld: byte_at %lld",
                      reads_per_block, (long long)n_reads, (int)has_offsets, (long long)l.first, (long long)l.byte_at);
                CHECK(l.blocks * reads_per_block >= l.n && l.blocks * reads_per_block < l.n + reads_per_block &&
                          l.blocks <= (int64_t)1 << 23,
                      "walk(%d) n_reads %lld first %lld: %lld workgroups for %lld reads", reads_per_block, (long long)n_reads,
                      (long long)l.first, (long long)l.blocks, (long long)l.n);
                next = l.first + l.n;
                ++launches;
            });
            CHECK(next == n_reads && launches == (n_reads + per - 1) / per && launches <= 3,
                  "walk(%d) n_reads %lld offsets %d: %d launches end at %lld", reads_per_block, (long long)n_reads, (int)has_offsets,
                  launches, (long long)next);
        }
}

static void check_cuts()
{
    for (const int reads_per_block : {1, 4}) {
        const int64_t per = kmer_plan::wave_reads_per_launch(reads_per_block);
        CHECK(per / reads_per_block == (int64_t)1 << 23, "wave_reads_per_launch(%d): workgroups", reads_per_block); // threads < 2^32
        check_cut(per, "a wave a read");
        check_wave_walk(reads_per_block);
    }
    for (const int64_t n_windows : {(int64_t)1, (int64_t)70, (int64_t)80, (int64_t)4096, ((int64_t)1 << 31) - 256, (int64_t)1 << 31}) {
        const int64_t per = kmer_plan::window_reads_per_launch(n_windows);
        // a launch's windows, rounded up to workgroups of 256, stay below 2^31 -- or the launch is one read
        CHECK(per == 1 || (per * n_windows + 255 < (int64_t)1 << 31 && (per + 1) * n_windows > ((int64_t)1 << 31) - 256),
              "window_reads_per_launch(%lld) = %lld", (long long)n_windows, (long long)per);
        check_cut(per, "a thread a window");
    }
}

int main()
{
    check_runs();
    check_pieces();
    check_codes();
    check_cuts();
    std::printf("kmer_stages ok\n");
    return 0;
}
