// colhi_check.cpp -- covest_amd/csrc/band.h column_limit_of_block on the host, for tests/test_colhi_host.py: one
// workgroup's slots a line on stdin,
//     n_waves  slots_per_wave  n_build  plain  floor_min  n_extra_max  n_qtiles  tile[..]  nsh[..]  cont[..]  top[n_qtiles]
// (integers; the three slot arrays hold n_waves * slots_per_wave entries each), one "floor extra[0] .. extra[n_extra_max - 1]"
// a line on stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "band.h"

int main()
{
    std::vector<char> line(1 << 16);
    long n = 0;
    while (std::fgets(line.data(), (int)line.size(), stdin)) {
        if (std::strlen(line.data()) < 2)
            continue;
        std::vector<long> v;
        char *p = line.data();
        for (;;) {
            char *end = nullptr;
            const long x = std::strtol(p, &end, 10);
            if (end == p)
                break;
            v.push_back(x);
            p = end;
        }
        ++n;
        if (v.size() < 7 || v[0] < 1 || v[0] > 16 || v[1] < 1 || v[1] > 16 || v[2] < 0 || v[5] < 0 || v[5] > 64 || v[6] < 1 || v[6] > 4096 ||
            v.size() != (size_t)(7 + 3 * v[0] * v[1] + v[6])) {
            std::fprintf(stderr, "line %ld: %zu values do not make a case\n", n, v.size());
            return 2;
        }
        const int n_waves = (int)v[0], spw = (int)v[1], n_build = (int)v[2], n_extra_max = (int)v[5], n_qtiles = (int)v[6];
        const size_t slots = (size_t)n_waves * (size_t)spw;
        std::vector<int32_t> tile(slots), nsh(slots), cont(slots), top((size_t)n_qtiles), extra((size_t)n_extra_max + 1, -7);
        for (size_t i = 0; i < slots; ++i) {
            tile[i] = (int32_t)v[7 + i];
            nsh[i] = (int32_t)v[7 + slots + i];
            cont[i] = (int32_t)v[7 + 2 * slots + i];
            if (tile[i] >= n_qtiles) {
                std::fprintf(stderr, "line %ld: slot %zu names q-tile %d of %d\n", n, i, (int)tile[i], n_qtiles);
                return 2;
            }
        }
        for (int t = 0; t < n_qtiles; ++t)
            top[(size_t)t] = (int32_t)v[7 + 3 * slots + (size_t)t];
        const int floor = covest::column_limit_of_block(tile.data(), nsh.data(), cont.data(), top.data(), n_waves, spw, n_build,
                                                        v[3] != 0, (int)v[4], extra.data(), n_extra_max);
        if (extra[(size_t)n_extra_max] != -7) { // (the entry behind the list is not the function's)
            std::fprintf(stderr, "line %ld: the list of extra slots was overrun\n", n);
            return 3;
        }
        std::printf("%d", floor);
        for (int j = 0; j < n_extra_max; ++j)
            std::printf(" %d", (int)extra[(size_t)j]);
        std::printf("\n");
    }
    return 0;
}
