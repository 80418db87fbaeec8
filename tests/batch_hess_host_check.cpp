// batch_hess_host_check.cpp -- the host arithmetic of a batch's second-order table (covest_amd/csrc/batch_host.h:
// batch_rows_per_point, batch_table_order, batch_points_per_chunk at R2 = 6 and 21 rows a point, the cap on the
// histograms) in a program of its own, for tests/test_batch_hess_cpu.py to build with the host compiler under
// -fsanitize=address,undefined and run.  No device.
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

// the chunks of a list of n points cut at `per`, marked in a vector of exactly n entries (a cut past the list is a write the
// sanitizer sees): every point once, no chunk over the budget unless it is the single point that no budget holds
static void check_list(int64_t n, int64_t per, int64_t rows, int64_t n_keys, int64_t cells)
{
    std::vector<int> seen((size_t)n, 0);
    int64_t next = 0;
    for (int64_t c = 0; c < batch_chunk_count(n, per); ++c) {
        int64_t first, count;
        batch_chunk(n, per, c, &first, &count);
        CHECK(first == next && count >= 1 && count <= per);
        CHECK(count * rows * n_keys <= cells || count == 1);
        for (int64_t i = first; i < first + count; ++i)
            ++seen[(size_t)i];
        next = first + count;
    }
    CHECK(next == n);
    for (const int s : seen)
        CHECK(s == 1);
}

int main()
{
    // rows a point by order: 1, P + 1, 1 + P + P (P + 1) / 2 -- and back
    CHECK(batch_rows_per_point(2, 0) == 1 && batch_rows_per_point(2, 1) == 3 && batch_rows_per_point(2, 2) == 6);
    CHECK(batch_rows_per_point(5, 0) == 1 && batch_rows_per_point(5, 1) == 6 && batch_rows_per_point(5, 2) == 21);
    for (const int P : {2, 5})
        for (const int order : {0, 1, 2})
            CHECK(batch_table_order(P, batch_rows_per_point(P, order)) == order);
    // (6 rows are the repeat model's gradient table AND the basic model's Hessian table: the order follows from P)
    CHECK(batch_table_order(5, 6) == 1 && batch_table_order(2, 6) == 2);

    const int64_t budget = kBatchHostTableBytes, cells = budget / 8;
    CHECK(batch_points_per_chunk(256, 6, budget) == 21845); // 2^28 / (6 * 256 * 8)
    CHECK(batch_points_per_chunk(256, 21, budget) == 6241); // 2^28 / (21 * 256 * 8)
    for (const int64_t rows : {(int64_t)6, (int64_t)21}) {
        for (const int64_t n_keys : {(int64_t)1, (int64_t)63, (int64_t)256, (int64_t)257, (int64_t)10000, (int64_t)100000}) {
            const int64_t per = batch_points_per_chunk(n_keys, rows, budget);
            CHECK(per >= 1);                          // one point at least
            CHECK(per * rows * n_keys <= cells);      // the product never over the budget ...
            CHECK((per + 1) * rows * n_keys > cells); // ... and one point more would be
            if (per > (int64_t)1 << 22)
                continue; // (the lists are marked point by point)
            check_list(per, per, rows, n_keys, cells);
            check_list(per + 1, per, rows, n_keys, cells);
            check_list(2 * per + 4, per, rows, n_keys, cells);
        }
        // a point larger than the budget: one point a chunk
        CHECK(batch_points_per_chunk(cells / rows + 1, rows, budget) == 1);
        CHECK(batch_points_per_chunk(cells + 1, rows, budget) == 1);
        check_list(3, 1, rows, cells + 1, cells);
        // a small budget, so that the cut at a few points a chunk is walked
        const int64_t small = 4096 * 8;
        for (const int64_t n_keys : {(int64_t)1, (int64_t)5, (int64_t)100, (int64_t)4096}) {
            const int64_t per = batch_points_per_chunk(n_keys, rows, small);
            CHECK(per == (small / (rows * n_keys * 8) > 0 ? small / (rows * n_keys * 8) : 1));
            check_list(per, per, rows, n_keys, 4096);
            check_list(3 * per + 1, per, rows, n_keys, 4096);
        }
    }
    // the cap on the histograms of a batch: 2^20, whatever the table's order
    const std::vector<double> one(1, 1.0);
    CHECK(kBatchHostMaxHist == (int64_t)1 << 20);
    CHECK(batch_check_create(1, 0, nullptr, nullptr) == nullptr);
    CHECK(batch_check_create(1, 1, one.data(), nullptr) == nullptr);
    CHECK(batch_check_create(1, kBatchHostMaxHist + 1, one.data(), nullptr) != nullptr); // (refused before a count is read)
    // the argument rules of the three second-order entry points are the first-order ones' (abi_batch.cpp)
    CHECK(batch_check_points(-1, 1, one.data(), one.data()) != nullptr);
    CHECK(batch_check_points(1, 1, nullptr, one.data()) != nullptr);
    CHECK(batch_check_points(1, 1, one.data(), one.data(), nullptr) != nullptr);
    const int64_t idx[2] = {0, 3};
    CHECK(batch_check_pairs(2, 3, idx, one.data(), one.data()) != nullptr && batch_check_pairs(2, 4, idx, one.data(), one.data()) == nullptr);
    if (failures == 0)
        std::printf("batch_hess_host_check ok\n");
    return failures == 0 ? 0 : 1;
}
