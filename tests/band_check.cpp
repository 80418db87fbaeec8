// band_check.cpp -- covest_amd/csrc/band.h on the host, for tests/test_band_host.py: one case a line on stdin,
//     rate0  ln_rate[0..7]  ln_comb[0..7]  ln(1-q)  o_ref_max  n_steps  key_first  key_last
// (doubles as printed by Python's repr: they round-trip), one "step_lo step_hi" a line on stdout.  Before the first
// line: BandBytes, the bytes the kernel keeps the edges in, over every slot (exit status 3 if it fails).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "band.h"

// every slot 0 .. 5: what is set is got, the other slots stay "not banded", an edge of 255 or more is "not banded"
static bool band_bytes_sound()
{
    using covest::BandBytes;
    const int edges[] = {0, 1, 2, 37, 127, 128, 254, 255, 256, 1000, 1 << 20};
    for (int k = 0; k < BandBytes::kSlots; ++k)
        for (int edge : edges) {
            BandBytes b;
            b.set(k, edge);
            for (int j = 0; j < BandBytes::kSlots; ++j)
                if (b.get(j) != (j != k || edge >= 255 ? 255 : edge))
                    return false;
            b.set(k, 3); // (set again: the byte is replaced, not or-ed)
            if (b.get(k) != 3)
                return false;
        }
    BandBytes all; // every slot set, each to its own edge: no byte runs into its neighbour
    for (int k = 0; k < BandBytes::kSlots; ++k)
        all.set(k, 250 - 40 * k);
    for (int k = 0; k < BandBytes::kSlots; ++k)
        if (all.get(k) != 250 - 40 * k)
            return false;
    return BandBytes{}.get(0) == BandBytes::kNone && BandBytes::kNone == 255;
}

int main()
{
    if (!band_bytes_sound()) {
        std::fprintf(stderr, "BandBytes (band.h): set / get over the six slots\n");
        return 3;
    }
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
