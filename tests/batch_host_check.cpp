// batch_host_check.cpp -- the argument rules and the host arithmetic of the covest_batch_* entry points
// (covest_amd/csrc/batch_host.h, which abi_batch.cpp wraps) in a program of its own, for tests/test_batch_cpu.py to
// build with the host compiler under -fsanitize=address,undefined and run.  No device.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
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

// every point of a list of n is in exactly one chunk, the chunks are in order, none is empty or over the size
static void check_chunks(int64_t n, int64_t per)
{
    const int64_t chunks = batch_chunk_count(n, per);
    int64_t next = 0;
    for (int64_t c = 0; c < chunks; ++c) {
        int64_t first, count;
        batch_chunk(n, per, c, &first, &count);
        CHECK(first == next && count >= 1 && count <= per);
        next = first + count;
    }
    CHECK(next == (n > 0 ? n : 0));
}

static void check_parts(int64_t total, int64_t cap)
{
    const int64_t parts = batch_launch_parts(total, cap);
    int64_t next = 0;
    for (int64_t k = 0; k < parts; ++k) {
        int64_t first, count;
        batch_launch_part(total, cap, k, &first, &count);
        CHECK(first == next && count >= 1 && count <= cap);
        next = first + count;
    }
    CHECK(next == (total > 0 ? total : 0));
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- covest_batch_create's rules
    {
        const std::vector<double> h = {0.0, 1.0, 2.5, 1e6, 0.0, 3.0}; // exactly 2 x 3: the sanitizer sees a read past it
        const std::vector<double> t = {0.0, 7.0};
        CHECK(batch_check_create(3, 2, h.data(), t.data()) == nullptr);
        CHECK(batch_check_create(3, 2, h.data(), nullptr) == nullptr);
        CHECK(batch_check_create(6, 1, h.data(), nullptr) == nullptr);
        CHECK(batch_check_create(3, 0, nullptr, nullptr) == nullptr); // an empty batch
        CHECK(batch_check_create(3, 2, nullptr, nullptr) != nullptr);
        CHECK(batch_check_create(3, -1, h.data(), nullptr) != nullptr);
        CHECK(batch_check_create(0, 2, h.data(), nullptr) != nullptr);
        CHECK(batch_check_create(1, kBatchHostMaxHist + 1, h.data(), nullptr) != nullptr); // (refused before it reads)
        for (const double bad : {-1.0, -1e-300, nan, inf, -inf}) {
            std::vector<double> hb = h, tb = t;
            hb[5] = bad;
            tb[1] = bad;
            CHECK(batch_check_create(3, 2, hb.data(), t.data()) != nullptr);
            CHECK(batch_check_create(3, 2, h.data(), tb.data()) != nullptr);
        }
    }
    // ---- an evaluation's
    {
        const double par[2] = {10.0, 0.05};
        double out[1];
        CHECK(batch_check_points(1, 1, par, out) == nullptr);
        CHECK(batch_check_points(0, 1, nullptr, nullptr) == nullptr); // an empty list
        CHECK(batch_check_points(5, 0, nullptr, nullptr) == nullptr); // an empty batch
        CHECK(batch_check_points(-1, 1, par, out) != nullptr);
        CHECK(batch_check_points(1, 1, nullptr, out) != nullptr);
        CHECK(batch_check_points(1, 1, par, nullptr) != nullptr);
        const std::vector<int64_t> idx = {0, 4, 4, 2};
        CHECK(batch_check_index(4, idx.data(), 5) == nullptr);
        CHECK(batch_check_index(0, nullptr, 5) == nullptr);
        CHECK(batch_check_index(4, nullptr, 5) != nullptr);
        CHECK(batch_check_index(4, idx.data(), 4) != nullptr);
        CHECK(batch_check_index(1, idx.data(), 0) != nullptr);
        const int64_t neg = -1;
        CHECK(batch_check_index(1, &neg, 5) != nullptr);
        // the arg-min's two results and the score table's: both, whenever there is anything to do
        int64_t arg[1];
        CHECK(batch_check_points(1, 1, par, out, arg) == nullptr);
        CHECK(batch_check_points(0, 1, nullptr, nullptr, nullptr) == nullptr);
        CHECK(batch_check_points(5, 0, nullptr, nullptr, nullptr) == nullptr); // (an empty batch has no minimum to write)
        CHECK(batch_check_points(-1, 1, par, out, arg) != nullptr);
        CHECK(batch_check_points(-1, 0, par, out, arg) != nullptr);
        CHECK(batch_check_points(1, 1, nullptr, out, arg) != nullptr);
        CHECK(batch_check_points(1, 1, par, nullptr, arg) != nullptr);
        CHECK(batch_check_points(1, 1, par, out, nullptr) != nullptr);
        // a pairs call: the sign of n before anything is read, the buffers whatever the batch holds, then the index
        double four[4];
        const std::vector<double> pts(8, 1.0);
        CHECK(batch_check_pairs(4, 5, idx.data(), pts.data(), four) == nullptr);
        CHECK(batch_check_pairs(0, 5, nullptr, nullptr, nullptr) == nullptr);
        CHECK(batch_check_pairs(0, 0, nullptr, nullptr, nullptr) == nullptr);
        CHECK(batch_check_pairs(-1, 5, nullptr, pts.data(), four) != nullptr); // (a null index of -1 entries is not read)
        CHECK(batch_check_pairs(4, 5, idx.data(), nullptr, four) != nullptr);
        CHECK(batch_check_pairs(4, 5, idx.data(), pts.data(), nullptr) != nullptr);
        CHECK(batch_check_pairs(4, 0, idx.data(), nullptr, four) != nullptr); // an empty batch: still a null buffer
        CHECK(batch_check_pairs(4, 5, nullptr, pts.data(), four) != nullptr);
        CHECK(batch_check_pairs(4, 4, idx.data(), pts.data(), four) != nullptr);
        CHECK(batch_check_pairs(1, 0, idx.data(), pts.data(), four) != nullptr);
    }
    // ---- the chunking of a point list against the table budget: 0, 1, one chunk exactly, one chunk plus one
    {
        CHECK(batch_points_per_chunk(256, 1, 256 * 8 * 10) == 10);
        CHECK(batch_points_per_chunk(256, 1, 256 * 8 * 10 + 7) == 10);
        CHECK(batch_points_per_chunk(256, 1, 100) == 1); // a row beyond the budget: one point at a time
        CHECK(batch_points_per_chunk(1, 1, kBatchHostTableBytes) == kBatchHostTableBytes / 8);
        CHECK(batch_points_per_chunk(256, 1, kBatchHostTableBytes) == 131072);
        for (const int64_t per : {(int64_t)1, (int64_t)10, (int64_t)131072}) {
            CHECK(batch_chunk_count(0, per) == 0);
            CHECK(batch_chunk_count(1, per) == 1);
            CHECK(batch_chunk_count(per, per) == 1);
            CHECK(batch_chunk_count(per + 1, per) == 2);
            CHECK(batch_chunk_count(-3, per) == 0);
            for (const int64_t n : {(int64_t)0, (int64_t)1, per - 1, per, per + 1, 2 * per, 2 * per + 1, 7 * per + 3})
                check_chunks(n, per);
            int64_t first, count;
            batch_chunk(per + 1, per, 1, &first, &count);
            CHECK(first == per && count == 1);
            batch_chunk(per, per, 0, &first, &count);
            CHECK(first == 0 && count == per);
        }
    }
    // ---- the cut of launches
    {
        for (const int64_t cap : {(int64_t)1, (int64_t)5, kBatchHostMaxBlocks}) {
            CHECK(batch_launch_parts(0, cap) == 0);
            CHECK(batch_launch_parts(1, cap) == 1);
            CHECK(batch_launch_parts(cap, cap) == 1);
            CHECK(batch_launch_parts(cap + 1, cap) == 2);
            for (const int64_t total : {(int64_t)0, (int64_t)1, cap - 1, cap, cap + 1, 3 * cap + 2})
                check_parts(total, cap);
        }
        CHECK(batch_cross_groups_y(1) == 1 && batch_cross_groups_y(64) == 1 && batch_cross_groups_y(65) == 2);
        CHECK(batch_cross_groups_y(kBatchHostMaxHist) == 16384); // (a grid's y stays below 65536)
        CHECK(batch_cross_groups_x(1) == 1 && batch_cross_groups_x(64) == 1 && batch_cross_groups_x(65) == 2);
        CHECK(batch_cross_x_per_launch(1, kBatchHostMaxBlocks) == kBatchHostMaxBlocks);
        CHECK(batch_cross_x_per_launch(16384, kBatchHostMaxBlocks) == 512);
        CHECK(batch_cross_x_per_launch(kBatchHostMaxBlocks + 5, kBatchHostMaxBlocks) == 1);
    }
    // ---- the exactly rounded sum
    {
        CHECK(batch_fsum(nullptr, 0) == 0.0);
        const double one = 1.0;
        CHECK(batch_fsum(&one, 1) == 1.0);
        const std::vector<double> a = {1e100, 1.0, -1e100};
        CHECK(batch_fsum(a.data(), 3) == 1.0);
        const std::vector<double> b(10, 0.1);
        CHECK(batch_fsum(b.data(), 10) == 1.0); // (the naive sum gives 0.9999999999999999)
        const std::vector<double> c = {1.0, 1e-16, 1e-16, 1e-16, 1e-16, 1e-16, 1e-16};
        CHECK(batch_fsum(c.data(), (int64_t)c.size()) == 1.0000000000000007);
        const std::vector<double> half = {1.0, 1.1102230246251565e-16, 1e-40}; // 1 + 2^-53 + a little: rounds UP
        CHECK(batch_fsum(half.data(), 3) == 1.0000000000000002);
        const std::vector<double> half_down = {1.0, 1.1102230246251565e-16, -1e-40};
        CHECK(batch_fsum(half_down.data(), 3) == 1.0);
        std::mt19937_64 rng(20240801);
        std::uniform_real_distribution<double> uni(0.0, 1.0);
        std::vector<double> p(1000);
        long double wide = 0.0L;
        for (double &v : p) {
            v = std::ldexp(uni(rng), -(int)(rng() % 40)) / 1000.0;
            wide += v;
        }
        const double got = batch_fsum(p.data(), (int64_t)p.size());
        CHECK(std::fabs((double)((long double)got - wide)) <= 4e-16 * got);
        // ---- the weights of a draw
        std::vector<double> w(p.size() + 1, -1.0);
        batch_draw_weights((int64_t)p.size(), p.data(), true, w.data());
        CHECK(w[0] == p[0] && w[p.size() - 1] == p.back() && w.back() == 1.0 - got);
        std::vector<double> w2(p.size(), -1.0); // exactly n_keys entries without a tail
        batch_draw_weights((int64_t)p.size(), p.data(), false, w2.data());
        CHECK(w2.back() == p.back());
        const std::vector<double> over = {0.75, 0.5};
        std::vector<double> w3(3);
        batch_draw_weights(2, over.data(), true, w3.data());
        CHECK(w3[2] == 0.0); // max(0, 1 - 1.25)
    }
    if (failures)
        return 1;
    std::printf("batch_host_check ok\n");
    return 0;
}
