// batch_grad_host_check.cpp -- the chunk arithmetic of a batch's gradient table (covest_amd/csrc/batch_host.h:
// batch_points_per_chunk, with batch_chunk_count and batch_chunk) in a program of its own, for
// tests/test_batch_grad_cpu.py to build with the host compiler under -fsanitize=address,undefined and run.  No device.
#include <cstdio>
#include <vector>

#include "batch_host.h"

using namespace covest;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// a list of n points cut at `per`: every point in exactly one chunk, in order, none empty or over the size; each chunk's
// rows fit `cells` doubles unless the chunk is the single point that no budget holds.  The chunks are marked in a vector
// of exactly n entries, so that a cut past the list is a write the sanitizer sees.
static void check_list(int64_t n, int64_t per, int64_t rows, int64_t n_keys, int64_t cells, int64_t want_chunks)
{
    std::vector<int> seen((size_t)(n > 0 ? n : 0), 0);
    const int64_t chunks = batch_chunk_count(n, per);
    CHECK(chunks == want_chunks);
    int64_t next = 0;
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, count;
        batch_chunk(n, per, c, &first, &count);
        CHECK(first == next && count >= 1 && count <= per);
        CHECK(count * rows * n_keys <= cells || count == 1);
        for (int64_t i = first; i < first + count; ++i)
            ++seen[(size_t)i];
        next = first + count;
    }
    CHECK(next == (n > 0 ? n : 0));
    for (const int s : seen)
        CHECK(s == 1);
}

int main()
{
    const int64_t budget = kBatchHostTableBytes, cells = budget / 8;
    CHECK(batch_points_per_chunk(256, 3, budget) == 43690); // 2^28 / (3 * 256 * 8)
    CHECK(batch_points_per_chunk(256, 6, budget) == 21845);
    CHECK(batch_points_per_chunk(256, 1, budget) == 131072); // one row a point: the value table's chunk
    for (const int64_t rows : {(int64_t)3, (int64_t)6}) {
        for (const int64_t n_keys : {(int64_t)1, (int64_t)63, (int64_t)256, (int64_t)257, (int64_t)100000}) {
            const int64_t per = batch_points_per_chunk(n_keys, rows, budget);
            CHECK(per >= 1);
            CHECK(per * rows * n_keys <= cells);             // a chunk fits the budget ...
            CHECK((per + 1) * rows * n_keys > cells);        // ... and one point more would not
            CHECK(per == budget / (rows * n_keys * 8));      // the issue's arithmetic, one division
            if (per > (int64_t)1 << 22)
                continue; // (the lists below are marked point by point: the small chunk sizes carry the arithmetic)
            check_list(0, per, rows, n_keys, cells, 0);
            check_list(1, per, rows, n_keys, cells, 1);
            check_list(per, per, rows, n_keys, cells, 1);     // one chunk exactly
            check_list(per + 1, per, rows, n_keys, cells, 2); // one chunk plus one
            check_list(2 * per + 21, per, rows, n_keys, cells, 3);
        }
        // a row larger than the budget: one point a chunk
        const int64_t huge = cells + 1;
        CHECK(batch_points_per_chunk(huge, rows, budget) == 1);
        CHECK(batch_points_per_chunk(cells / rows + 1, rows, budget) == 1);
        check_list(3, 1, rows, huge, cells, 3);
        // a small budget, so that the large counts are walked too
        const int64_t small = 4096 * 8;
        for (const int64_t n_keys : {(int64_t)1, (int64_t)5, (int64_t)4096, (int64_t)5000}) {
            const int64_t per = batch_points_per_chunk(n_keys, rows, small);
            CHECK(per == (small / (rows * n_keys * 8) > 0 ? small / (rows * n_keys * 8) : 1));
            check_list(0, per, rows, n_keys, 4096, 0);
            check_list(per, per, rows, n_keys, 4096, 1);
            check_list(per + 1, per, rows, n_keys, 4096, 2);
        }
    }
    // degenerate arguments stay defined: at least one point, whatever is asked
    CHECK(batch_points_per_chunk(0, 3, budget) == batch_points_per_chunk(0, 1, budget) / 3);
    CHECK(batch_points_per_chunk(256, 0, budget) == batch_points_per_chunk(256, 1, budget));
    CHECK(batch_points_per_chunk(256, 3, 0) == 1);
    if (failures) {
        std::printf("batch_grad_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("batch_grad_host_check ok\n");
    return 0;
}
