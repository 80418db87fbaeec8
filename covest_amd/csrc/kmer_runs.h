// kmer_runs.h -- the runs of pass 1 of the partitioned k-mer counter (kmer_scatter.h) as integer arithmetic, in plain
// C++: how many windows the run that starts at a thread has, and the pieces it goes out as.  The host compiler builds
// it too: tests/kmer_stages_check.cpp walks it against a lane-by-lane count under sanitizers.
#pragma once
#include "kmer_codes.h"
#include "kmer_plan.h"

namespace covest {
namespace kmer {

constexpr int kRunWave = 64;                             // lanes of a wave: a bit each in the masks below
constexpr int kRunWaves = kmer_plan::kTile / kRunWave;   // waves of a tile

// Windows of the run whose head is `lane` of `wave`.  heads / valid: the wave's own masks (bit l: thread l starts a
// run / starts a window); tile_heads / tile_valid: the same of the tile's kRunWaves waves.  A run ends before the next
// head or the first byte that starts no window, in this wave or a later one, or with the tile.
KMER_HD int run_length(int lane, int wave, unsigned long long heads, unsigned long long valid,
                       const unsigned long long *tile_heads, const unsigned long long *tile_valid)
{
    const unsigned long long stop = (heads | ~valid) & (lane == kRunWave - 1 ? 0ull : (~0ull << (lane + 1)));
    if (stop)
        return __builtin_ctzll(stop) - lane;
    int run = kRunWave - lane;
    for (int wv = wave + 1; wv < kRunWaves; ++wv) {
        const unsigned long long s2 = tile_heads[wv] | ~tile_valid[wv];
        if (s2)
            return run + __builtin_ctzll(s2);
        run += kRunWave;
    }
    return run;
}

// A record holds 32 bases, max_run = 32 - k + 1 windows: a longer run goes out as pieces of max_run windows and a rest.
KMER_HD int pieces_of(int run, int max_run)
{
    return (run + max_run - 1) / max_run;
}

// emit(first window of the piece, counted from the run's head; bases of the piece) for every piece of the run
template <class Emit>
KMER_HD void for_each_piece(int run, int max_run, int k, Emit &&emit)
{
    for (int first = 0; first < run; first += max_run)
        emit(first, (run - first < max_run ? run - first : max_run) + k - 1);
}

} // namespace kmer
} // namespace covest
