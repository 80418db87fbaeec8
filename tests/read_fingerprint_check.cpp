// read_fingerprint_check.cpp -- csrc/read_fingerprint.h under the host compiler's sanitizers (tests/test_dedup_cpu.py
// builds and runs it): F of a read and of its reverse complement swap, the canonical key is the same for the two, any
// split of a read into lane shares sums to the same word, the lengths at the wave's edges, the table's size up to 2^40
// reads, and the sentinel.  With arguments it prints keys for the restatement to compare: SEED RC FP_BITS READ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "read_fingerprint.h"

using namespace covest::fingerprint;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static std::vector<unsigned char> random_read(size_t len, uint64_t &state, const char *alphabet)
{
    const size_t n = std::strlen(alphabet);
    std::vector<unsigned char> x(len);
    for (auto &b : x) {
        state = mix64(state + 0x9E3779B97F4A7C15ull);
        b = (unsigned char)alphabet[state % n];
    }
    return x;
}

static std::vector<unsigned char> revcomp(const std::vector<unsigned char> &x)
{
    std::vector<unsigned char> y(x.size());
    for (size_t j = 0; j < x.size(); ++j)
        y[x.size() - 1 - j] = (unsigned char)complement(x[j]);
    return y;
}

static void sums(const std::vector<unsigned char> &x, uint64_t seed, uint64_t &s, uint64_t &t)
{
    s = t = 0;
    add_share(x.data(), 0, x.size(), x.size(), salt_of(seed), s, t);
}

int main(int argc, char **argv)
{
    if (argc > 3) { // keys of the given reads, a line each
        const uint64_t seed = std::strtoull(argv[1], nullptr, 0);
        const int rc = std::atoi(argv[2]), bits = std::atoi(argv[3]);
        for (int i = 4; i < argc; ++i) {
            const std::string r = std::strcmp(argv[i], "-") ? argv[i] : ""; // ("-": the empty read)
            const std::vector<unsigned char> x(r.begin(), r.end());
            uint64_t s, t;
            sums(x, seed, s, t);
            std::printf("%llu\n", (unsigned long long)key_of(s, t, x.size(), seed, rc, bits));
        }
        return 0;
    }
    // the complement: an involution that keeps the case and every other byte
    for (unsigned b = 0; b < 256; ++b) {
        CHECK(complement(complement(b)) == b);
        const bool base = std::strchr("acgtACGT", (int)b) != nullptr && b != 0;
        CHECK((complement(b) != b) == base);
        CHECK(((complement(b) ^ b) & 0x20u) == 0u);
    }
    CHECK(complement('a') == 't' && complement('c') == 'g' && complement('G') == 'C' && complement('T') == 'A');
    CHECK(complement('n') == 'n' && complement('N') == 'N');

    uint64_t state = 12345;
    const size_t lengths[] = {0, 1, 63, 64, 65, 1000};
    for (const uint64_t seed : {0ull, 1ull, 0x57e40badf00dull, ~0ull})
        for (const size_t len : lengths)
            for (const char *alphabet : {"acgt", "acgtnACGTN*"}) {
                const std::vector<unsigned char> x = random_read(len, state, alphabet), y = revcomp(x);
                uint64_t sx, tx, sy, ty;
                sums(x, seed, sx, tx);
                sums(y, seed, sy, ty);
                CHECK(sx == ty && tx == sy); // F(x) and F(rc(x)) swap
                CHECK(revcomp(y) == x);
                for (const int bits : {1, 4, 8, 32, 62, 63}) {
                    CHECK(key_of(sx, tx, len, seed, 1, bits) == key_of(sy, ty, len, seed, 1, bits));
                    CHECK(key_of(sx, tx, len, seed, 0, bits) == (finish(sx, len, seed) & key_mask(bits)));
                    CHECK(key_of(sx, tx, len, seed, 1, bits) != kEmptyKey && key_of(sx, tx, len, seed, 0, bits) != kEmptyKey);
                    CHECK((key_of(sx, tx, len, seed, 1, bits) >> bits) == 0);
                }
                // any split into lane shares: contiguous pieces, and lanes striding by 1, 4 and 16 bytes
                for (const size_t cut : {(size_t)0, len / 3, len / 2, len}) {
                    uint64_t s = 0, t = 0;
                    add_share(x.data(), cut, len, len, salt_of(seed), s, t); // (the later share first)
                    add_share(x.data(), 0, cut, len, salt_of(seed), s, t);
                    CHECK(s == sx && t == tx);
                }
                for (const size_t unit : {(size_t)1, (size_t)4, (size_t)16}) {
                    uint64_t lane_s[64] = {0}, lane_t[64] = {0}, s = 0, t = 0;
                    for (size_t at = 0, u = 0; at < len; at += unit, ++u)
                        add_share(x.data(), at, at + unit < len ? at + unit : len, len, salt_of(seed), lane_s[u % 64], lane_t[u % 64]);
                    for (int lane = 63; lane >= 0; --lane) {
                        s += lane_s[lane];
                        t += lane_t[lane];
                    }
                    CHECK(s == sx && t == tx);
                }
                if (len > 1 && x[0] != x[len - 1]) { // the position counts: the same bytes in another order
                    std::vector<unsigned char> z = x;
                    std::swap(z[0], z[len - 1]);
                    uint64_t sz, tz;
                    sums(z, seed, sz, tz);
                    CHECK(sz != sx);
                }
            }
    // the seed and the length go into the last mix: equal sums, other keys
    CHECK(finish(7, 3, 0) != finish(7, 4, 0) && finish(7, 3, 0) != finish(7, 3, 1));
    {   // the empty read: both sums 0
        uint64_t s = 1, t = 1;
        sums(std::vector<unsigned char>(), 5, s, t);
        CHECK(s == 0 && t == 0);
    }
    // the sentinel is no key, whatever the sums: bit 63 of a key is never set
    for (int bits = 1; bits <= 63; ++bits) {
        CHECK(key_mask(bits) == (bits == 63 ? 0x7fffffffffffffffull : (1ull << bits) - 1ull));
        CHECK((kEmptyKey & key_mask(bits)) != kEmptyKey);
    }
    // the table: a power of two of slots, at least 2 n, the smallest such from 2^10 on; no overflow up to 2^40 reads
    for (int lg = 0; lg <= 40; ++lg)
        for (const int64_t d : {-1, 0, 1}) {
            const int64_t n = ((int64_t)1 << lg) + d;
            if (n < 0)
                continue;
            const int got = table_log2_slots(n);
            CHECK(got >= kMinLog2Slots && got <= 42); // (2^40 + 1 reads: 2^42 slots)
            CHECK(((int64_t)1 << got) >= 2 * n);
            CHECK(got == kMinLog2Slots || ((int64_t)1 << (got - 1)) < 2 * n);
            CHECK(slot_of(~0ull >> 1, got) < (1ull << got) && slot_of(0, got) == 0);
        }
    CHECK(table_log2_slots(0) == 10 && table_log2_slots(512) == 10 && table_log2_slots(513) == 11);
    CHECK(table_log2_slots((int64_t)1 << 40) == 41);
    if (failures)
        return 1;
    std::printf("read_fingerprint ok\n");
    return 0;
}
