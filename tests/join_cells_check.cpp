// join_cells_check.cpp -- the cell arithmetic of the k-mer join (kmer_join.h: the clip, the LDS rectangle, the flat index,
// the bound on the matrix) on the host: plain C++, its own main, built and run under the host compiler's sanitizers by
// tests/test_join_cpu.py.  The kernel compiles the same header; what it indexes with these functions -- 16 KB of bins in
// LDS, n_rows * n_cols words in HBM -- is an array here that the address sanitizer watches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmer_join.h"

using namespace covest;
using namespace covest::kmer_join;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::fprintf(stderr, "join_cells_check: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                           \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

// 1. the clip: min(count, n - 1), for every n from 1 and counts at, below and far above it
static void clips()
{
    const unsigned long long counts[] = {0ull, 1ull, 2ull, 15ull, 16ull, 17ull, 255ull, 256ull, 257ull, 70000ull,
                                         (1ull << 22) - 1, 1ull << 22, (1ull << 32) - 1, 1ull << 32, ~0ull};
    const uint32_t sizes[] = {1u, 2u, 3u, 16u, 17u, 256u, 257u, 70001u, 1u << 22};
    for (const uint32_t n : sizes)
        for (const unsigned long long c : counts) {
            const unsigned long long want = c < n - 1ull ? c : n - 1ull;
            CHECK(clip(c, n) == want && clip(c, n) < n, "clip(%llu, %u) = %u", c, n, clip(c, n));
        }
}

// 2. the LDS rectangle: its edges, and a bin of its own, inside the array, for every cell in it
static void lds_rectangle()
{
    CHECK(kLdsBins == kLdsRows * kLdsCols && kLdsBins * (int)sizeof(unsigned) <= 64 * 1024, "the bins fit the LDS");
    CHECK(in_lds(0, 0) && in_lds(kLdsRows - 1, kLdsCols - 1), "the corners are inside");
    CHECK(!in_lds(kLdsRows, 0) && !in_lds(0, kLdsCols) && !in_lds(kLdsRows, kLdsCols), "one beyond is outside");
    CHECK(!in_lds(kLdsRows - 1, kLdsCols) && !in_lds(kLdsRows, kLdsCols - 1), "one beyond on one side is outside");
    CHECK(!in_lds(0xFFFFFFFFu, 0) && !in_lds(0, 0xFFFFFFFFu), "the largest indices are outside");
    std::vector<unsigned> bins((size_t)kLdsBins, 0u);
    for (uint32_t i = 0; i < (uint32_t)kLdsRows + 2; ++i)
        for (uint32_t j = 0; j < (uint32_t)kLdsCols + 2; ++j)
            if (in_lds(i, j))
                ++bins[lds_index(i, j)]; // (the sanitizer's: inside the array)
    for (const unsigned b : bins)
        CHECK(b == 1u, "a bin serves %u cells", b);
    // the flush's way back: bin -> (i, j)
    for (uint32_t at = 0; at < (uint32_t)kLdsBins; ++at)
        CHECK(lds_index(at / kLdsCols, at % kLdsCols) == at, "bin %u does not come back", at);
}

// 3. the flat index: every cell of a matrix once, inside it -- small shapes in full, the largest at their corners
static void flat_indices()
{
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {256, 16}, {257, 17}, {16, 256}, {3, 5}};
    for (const auto &s : shapes) {
        std::vector<unsigned char> seen((size_t)s[0] * s[1], 0);
        for (uint32_t i = 0; i < s[0]; ++i)
            for (uint32_t j = 0; j < s[1]; ++j)
                ++seen[flat_index(i, j, s[1])];
        for (const unsigned char v : seen)
            CHECK(v == 1, "%u x %u: a cell is met %d times", s[0], s[1], (int)v);
    }
    const int64_t big[][2] = {{kMaxCells, 1}, {1, kMaxCells}, {2048, 2048}, {1 << 20, 4}, {4, 1 << 20}, {70001, 59}};
    for (const auto &s : big) {
        CHECK(cells_ok(s[0], s[1]), "%lld x %lld is refused", (long long)s[0], (long long)s[1]);
        std::vector<unsigned char> cells((size_t)(s[0] * s[1]), 0);
        const uint32_t r = (uint32_t)s[0], c = (uint32_t)s[1];
        // what the kernel forms for the largest counts: the last cell, through the clips
        const uint32_t last = flat_index(clip(~0ull, r), clip(~0ull, c), c);
        CHECK((int64_t)last == s[0] * s[1] - 1, "%lld x %lld: the last cell lies at %u", (long long)s[0], (long long)s[1], last);
        cells[last] = 1;
        cells[flat_index(0, clip(~0ull, c), c)] = 1;
        cells[flat_index(clip(~0ull, r), 0, c)] = 1;
        cells[flat_index(0, 0, c)] = 1;
    }
}

// 4. the bound: n_rows * n_cols = 2^22 passes, one cell more does not, and no product overflows on the way
static void bounds()
{
    CHECK(kMaxCells == (int64_t)1 << 22, "the bound is 2^22 cells");
    CHECK(cells_ok(1, 1) && cells_ok(kMaxCells, 1) && cells_ok(1, kMaxCells) && cells_ok(2048, 2048), "at the bound");
    CHECK(!cells_ok(kMaxCells + 1, 1) && !cells_ok(1, kMaxCells + 1), "one row, one column beyond");
    CHECK(!cells_ok(2048, 2049) && !cells_ok(2049, 2048) && !cells_ok(kMaxCells, 2) && !cells_ok(2, kMaxCells), "one beyond");
    CHECK(cells_ok(2047, 2049) && cells_ok(3, kMaxCells / 3) && !cells_ok(3, kMaxCells / 3 + 1), "no multiple of the side");
    CHECK(!cells_ok(0, 1) && !cells_ok(1, 0) && !cells_ok(0, 0) && !cells_ok(-1, 1) && !cells_ok(1, -1) && !cells_ok(-2, -2),
          "less than one row or column");
    const int64_t huge = INT64_MAX;
    CHECK(!cells_ok(huge, huge) && !cells_ok(huge, 2) && !cells_ok(2, huge) && !cells_ok((int64_t)1 << 32, (int64_t)1 << 32) &&
              !cells_ok(INT64_MIN, INT64_MIN) && !cells_ok(INT64_MIN, 1),
          "sizes whose product leaves 64 bits");
}

int main()
{
    clips();
    lds_rectangle();
    flat_indices();
    bounds();
    std::printf("join_cells ok\n");
    return 0;
}
