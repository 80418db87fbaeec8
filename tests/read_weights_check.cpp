// read_weights_check.cpp -- where a launch of a weighted add starts in the weights (kmer_plan.h weights_at,
// window_weights_at), and the multiplicity table of the read bootstrap (sim_philox.h poisson1_multiplicity), on the host:
// plain C++, its own main, built and run under the host compiler's sanitizers by tests/test_read_bootstrap_cpu.py.
//
// The cut of a wave-a-read launch lies at 2^25 reads, that of the windows numbered through at about 2.7 * 10^7 reads of
// 80 windows: neither is reached by a GPU test of a few seconds.  What a weighted launcher adds to the weights pointer is
// therefore a function of its own here, and is walked over read counts beyond one cut and beyond two.  The check stands
// in for the kernel: a launch's kernel reads weights_base[local read], local = 0 .. n - 1, and every read of the call
// must be met exactly once, at its own index -- whatever the bytes do (with offsets they do not advance at all).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmer_plan.h"
#include "sim_philox.h"

using namespace covest;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::fprintf(stderr, "read_weights_check: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                           \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

// 1. a wave a read: the launches' weights tile [0, n_reads) in order; with offsets byte_at stays 0 and the weights move
static void wave_walk()
{
    const int reads_per_block = 4; // wave_read.h kWaveReadsPerBlock
    const int64_t per = kmer_plan::wave_reads_per_launch(reads_per_block);
    CHECK(per == (int64_t)1 << 25, "a launch of a wave a read holds %lld reads", (long long)per);
    const int64_t counts[] = {1, per - 1, per, per + 1, per + 5, 2 * per, 2 * per + 3};
    for (const int64_t n_reads : counts)
        for (const bool has_offsets : {false, true}) {
            const int64_t fixed_len = has_offsets ? 0 : 100;
            int64_t next = 0;
            int launches = 0;
            kmer_plan::for_each_wave_launch(n_reads, fixed_len, has_offsets, reads_per_block, [&](const kmer_plan::WaveLaunch &l) {
                const int64_t at = kmer_plan::weights_at(l);
                // the kernel's first and last read: weights_base[0] and weights_base[l.n - 1] are the call's weights of
                // the reads `next` and `next + l.n - 1`
                CHECK(at == next, "n_reads %lld offsets %d launch %d: the weights start at %lld, the reads at %lld", (long long)n_reads,
                      (int)has_offsets, launches, (long long)at, (long long)next);
                CHECK(at >= 0 && at + l.n <= n_reads, "n_reads %lld launch %d: weights %lld .. %lld leave the array", (long long)n_reads,
                      launches, (long long)at, (long long)(at + l.n));
                if (has_offsets)
                    CHECK(l.byte_at == 0 && (launches == 0 || at > 0), "offsets: the bytes stay, the weights move");
                else
                    CHECK(l.byte_at == at * fixed_len, "one length: read %lld lies at byte %lld", (long long)at, (long long)l.byte_at);
                next += l.n;
                ++launches;
            });
            CHECK(next == n_reads && launches == (n_reads + per - 1) / per, "n_reads %lld: %d launches end at read %lld",
                  (long long)n_reads, launches, (long long)next);
        }
}

// 2. the windows of reads of one length numbered through: the loop of kmer_update.h launch_update
static void window_walk()
{
    for (const int64_t n_windows : {1, 2, 80, 81}) {
        const int64_t per = kmer_plan::window_reads_per_launch(n_windows);
        const int64_t counts[] = {1, per, per + 1, 2 * per + 3};
        for (const int64_t n_reads : counts) {
            int64_t next = 0;
            for (int64_t first = 0; first < n_reads; first += per) {
                const int64_t n = kmer_plan::reads_of_launch(first, n_reads, per);
                const int64_t at = kmer_plan::window_weights_at(first);
                CHECK(at == next && at + n <= n_reads, "windows %lld n_reads %lld: weights at %lld, reads at %lld", (long long)n_windows,
                      (long long)n_reads, (long long)at, (long long)next);
                // the last thread of the launch: window n * n_windows - 1 is of local read n - 1
                CHECK((n * n_windows - 1) / n_windows == n - 1, "windows %lld: the last window's read", (long long)n_windows);
                next += n;
            }
            CHECK(next == n_reads, "windows %lld n_reads %lld: the launches end at read %lld", (long long)n_windows, (long long)n_reads,
                  (long long)next);
        }
    }
}

// 3. a small array for the sanitizer to watch: weights[i] = i, every launch reads its first and last entry through the
// pointer the launcher would pass
static void pointer_walk()
{
    const int reads_per_block = 4;
    const int64_t n_reads = kmer_plan::wave_reads_per_launch(reads_per_block) + 5;
    std::vector<uint32_t> weights((size_t)n_reads);
    for (int64_t i = 0; i < n_reads; ++i)
        weights[(size_t)i] = (uint32_t)i;
    int64_t seen = 0;
    kmer_plan::for_each_wave_launch(n_reads, 0, true, reads_per_block, [&](const kmer_plan::WaveLaunch &l) {
        const uint32_t *base = weights.data() + kmer_plan::weights_at(l);
        CHECK(base[0] == (uint32_t)l.first && base[l.n - 1] == (uint32_t)(l.first + l.n - 1), "launch at read %lld reads other weights",
              (long long)l.first);
        seen += l.n;
    });
    CHECK(seen == n_reads, "the launches cover %lld of %lld reads", (long long)seen, (long long)n_reads);
}

// 4. the multiplicity: thirteen steps, each taken exactly at its threshold
static void multiplicity_steps()
{
    const uint32_t t[kPoisson1Steps] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u,
                                        4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u};
    CHECK(poisson1_multiplicity(0u) == 0u && poisson1_multiplicity(0xFFFFFFFFu) == 13u, "the ends of the table");
    for (int i = 0; i < kPoisson1Steps; ++i) {
        CHECK(poisson1_multiplicity(t[i]) == (uint32_t)i + 1u, "at threshold %d", i);
        CHECK(poisson1_multiplicity(t[i] - 1u) == (uint32_t)i, "below threshold %d", i);
        CHECK(i == 0 || t[i] > t[i - 1], "threshold %d does not ascend", i);
    }
    // the stream's number and one known block: counter (5, 0, 2, 9) under key (7, 0) is what bootstrap_weight(5, 2, 7) reads
    uint32_t w[4];
    philox_block(5, 2u, kStreamBootstrap, philox_key(7), w);
    CHECK(kStreamBootstrap == 9u && bootstrap_weight(5, 2u, philox_key(7)) == poisson1_multiplicity(w[0]), "bootstrap_weight");
}

int main()
{
    wave_walk();
    window_walk();
    pointer_walk();
    multiplicity_steps();
    std::printf("read_weights ok\n");
    return 0;
}
