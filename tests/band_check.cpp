// band_check.cpp -- covest_amd/csrc/band.h on the host, for tests/test_band_host.py: one case a line on stdin,
//     rate0  ln_rate[0..7]  ln_comb[0..7]  ln(1-q)  o_ref_max  n_steps  key_first  key_last
// (doubles as printed by Python's repr: they round-trip), one "step_lo step_hi" a line on stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "band.h"

int main()
{
    std::vector<char> line(1 << 12);
    long n = 0;
    while (std::fgets(line.data(), (int)line.size(), stdin)) {
        if (std::strlen(line.data()) < 2)
            continue;
        double v[1 + 2 * covest::kBandClasses + 5];
        const int want = (int)(sizeof(v) / sizeof(v[0]));
        char *p = line.data();
        for (int i = 0; i < want; ++i) {
            char *end = nullptr;
            v[i] = std::strtod(p, &end);
            if (end == p) {
                std::fprintf(stderr, "line %ld: %d values, %d expected\n", n + 1, i, want);
                return 2;
            }
            p = end;
        }
        const double *ln_rate = v + 1, *ln_comb = v + 1 + covest::kBandClasses, *rest = v + 1 + 2 * covest::kBandClasses;
        const covest::BandTile t = covest::band_tile(ln_rate, ln_comb, rest[3], rest[4]);
        const covest::Band b = covest::band_of_unit(covest::BandMathHost{}, v[0], rest[0], (int)rest[1], (int)rest[2], t);
        std::printf("%d %d\n", b.step_lo, b.step_hi);
        ++n;
    }
    return 0;
}
