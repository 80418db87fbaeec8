// draw_host_check.cpp -- the host arithmetic and argument rules of covest_draw_thresholds / covest_draw_histograms*
// (covest_amd/csrc/draw_host.h, which abi_draw.cpp wraps) in a program of its own, for tests/test_draw_cpu.py to build
// with the host compiler under -fsanitize=address,undefined and run.  No device.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "draw_host.h"

using namespace covest;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

constexpr uint64_t kTop = 1ull << 63;

// thresholds of `w` into a buffer of exactly m entries (the sanitizer sees a write past it), with the properties any
// weight vector has: ascending, the last exactly 2^63, a zero weight repeating its predecessor
static std::vector<uint64_t> thresholds(const std::vector<double> &w)
{
    CHECK(draw_check_weights((int64_t)w.size(), w.data()) == nullptr);
    std::vector<uint64_t> t(w.size());
    draw_thresholds((int64_t)w.size(), w.data(), t.data());
    for (size_t i = 0; i < t.size(); ++i) {
        CHECK(t[i] <= kTop);
        if (i)
            CHECK(t[i - 1] <= t[i]);
        if (w[i] == 0.0)
            CHECK(t[i] == (i ? t[i - 1] : 0));
    }
    CHECK(t.back() == kTop);
    return t;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the shapes
    CHECK(thresholds({0.25})[0] == kTop);
    {
        const auto t = thresholds({1.0, 0.0});
        CHECK(t[0] == kTop && t[1] == kTop);
    }
    {
        const auto t = thresholds({0.0, 1.0});
        CHECK(t[0] == 0 && t[1] == kTop);
    }
    {
        const auto t = thresholds({0.0, 0.0, 5.0, 0.0, 0.0});
        CHECK(t[0] == 0 && t[1] == 0 && t[2] == kTop && t[3] == kTop && t[4] == kTop);
    }
    {
        const auto t = thresholds({1e-300, 1e-200, 1e-100, 1e-18, 1.0, 4.9406564584124654e-324});
        CHECK(t[0] == 0 && t[3] > 0 && t[4] == kTop && t[5] == kTop);
    }
    {
        const auto t = thresholds({4.9406564584124654e-324, 4.9406564584124654e-324}); // two denormals: a half each
        CHECK(t[0] == kTop / 2 && t[1] == kTop);
    }
    {
        const auto t = thresholds({1.0, 1.2, 1.5}); // total 3.7
        CHECK(t[0] == (uint64_t)(1.0 / (1.0 + 1.2 + 1.5) * 9223372036854775808.0));
    }
    {
        const auto t = thresholds({2.5e-13, 2.5e-13, 5e-13}); // total 1e-12
        CHECK(t[0] == kTop / 4 && t[1] == kTop / 2);
    }
    {
        std::mt19937_64 rng(20240613);
        std::uniform_real_distribution<double> uni(0.0, 1.0);
        std::vector<double> w(10001);
        for (double &v : w)
            v = uni(rng) < 0.1 ? 0.0 : uni(rng);
        w[0] = 1.0;
        thresholds(w);
    }
    // ---- every refusal
    const double one = 1.0, neg[2] = {1.0, -1e-300}, bad_nan[2] = {nan, 1.0}, bad_inf[2] = {1.0, inf}, zeros[3] = {0.0, 0.0, 0.0};
    const double huge[2] = {1.7e308, 1.7e308}; // finite weights, an infinite total
    CHECK(draw_check_weights(0, &one) != nullptr);
    CHECK(draw_check_weights(-1, &one) != nullptr);
    CHECK(draw_check_weights(1, nullptr) != nullptr);
    CHECK(draw_check_weights(2, neg) != nullptr);
    CHECK(draw_check_weights(2, bad_nan) != nullptr);
    CHECK(draw_check_weights(2, bad_inf) != nullptr);
    CHECK(draw_check_weights(3, zeros) != nullptr);
    CHECK(draw_check_weights(2, huge) != nullptr);
    CHECK(draw_check_weights(1, &one) == nullptr);
    const int64_t two32 = (int64_t)1 << 32, i64_max = std::numeric_limits<int64_t>::max();
    CHECK(draw_check_call(0, 1, 0, 1) != nullptr);
    CHECK(draw_check_call(kDrawHostMaxCells + 1, 1, 0, 1) != nullptr);
    CHECK(draw_check_call(1, -1, 0, 1) != nullptr);
    CHECK(draw_check_call(1, 1, 0, -1) != nullptr);
    CHECK(draw_check_call(1, 1, -1, 1) != nullptr);
    CHECK(draw_check_call(1, 1, two32, 1) != nullptr);
    CHECK(draw_check_call(1, 1, two32 - 1, 2) != nullptr);
    CHECK(draw_check_call(1, 1, 1, i64_max) != nullptr); // (no overflow in the sum)
    CHECK(draw_check_call(1, 1, i64_max, i64_max) != nullptr);
    CHECK(draw_check_call(1, 1, two32 - 1, 1) == nullptr);
    CHECK(draw_check_call(1, 1, 0, two32) == nullptr);
    CHECK(draw_check_call(kDrawHostMaxCells, 0, 0, 0) == nullptr);
    CHECK(draw_check_call(1, i64_max, 5, 3) == nullptr);
    if (failures)
        return 1;
    std::printf("draw_host_check ok\n");
    return 0;
}
