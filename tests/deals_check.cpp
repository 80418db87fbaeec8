// deals_check.cpp -- covest_amd/csrc/unit_deal.h on the host, for tests/test_deals_host.py: the planner's own charges and
// deal of units to waves.  One workgroup's units a line on stdin,
//     n_waves  n_columns  builders_charged  units_per_wave  one_block_a_pair  list_mode  n_pass  o_base  low_keys
//     build_cost  last_builder_extra  n_units  cost[n_units]
// (integers; the costs by falling cost, as plan_factored.cpp place_units sorts them), one "wave_of[0] .. wave_of[n_units - 1]"
// a line on stdout, or "full" where a unit finds no wave.  Built with -DCOVEST_TUNE the environment's overrides are read
// as the tuning library reads them.
#include <cstdio>
#include <cstring>
#include <vector>

#include "unit_deal.h"

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
        if (v.size() < 12 || v[11] < 0 || v[11] > 4096 || v.size() != (size_t)(12 + v[11]) || v[3] < 0) {
            std::fprintf(stderr, "line %ld: %zu values do not make a case\n", n, v.size());
            return 2;
        }
        const bool low_keys = v[8] != 0;
        covest::Charges ch = {0, (int)v[9], 1, (int)v[10], 0, {}};
        for (int w = 0; w < covest::kBuildShareWaves; ++w)
            ch.build_share[w] = covest::wave_share(low_keys, w);
#if defined(COVEST_DIAG) || defined(COVEST_TUNE)
        covest::charges_from_env(ch);
#endif
        const int n_units = (int)v[11];
        std::vector<int> cost((size_t)n_units), wave_of((size_t)n_units + 1, -7);
        for (int i = 0; i < n_units; ++i)
            cost[(size_t)i] = (int)v[12 + (size_t)i];
        const bool shares = covest::wave_shares_apply(v[4] != 0, (int)v[5], (int)v[6], (int)v[7]);
        const bool ok = covest::deal_units(cost.data(), n_units, (int)v[0], (int)v[1], v[2] != 0, (int)v[3], ch, shares, wave_of.data());
        if (wave_of[(size_t)n_units] != -7) { // (the entry behind the list is not the function's)
            std::fprintf(stderr, "line %ld: the list of waves was overrun\n", n);
            return 3;
        }
        if (!ok) {
            std::printf("full\n");
            continue;
        }
        for (int i = 0; i < n_units; ++i)
            std::printf(i ? " %d" : "%d", wave_of[(size_t)i]);
        std::printf("\n");
    }
    return 0;
}
