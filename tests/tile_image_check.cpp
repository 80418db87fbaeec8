// tile_image_check.cpp -- the host-side check of the generators' shared layer (covest_amd/csrc/tile_image.h and
// sim_philox.h), compiled and run by tests/test_tile_image_cpu.py with the host compiler under
// -fsanitize=address,undefined.  No device: the arithmetic that decides where the store step writes is plain C++.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim_philox.h"
#include "tile_image.h"

using namespace covest;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

// 1. Every lead and the totals around each boundary: the tiles of image_tiles and their 256 lanes store every byte of
// [0, total) exactly once and none outside; a vector store is 16-byte aligned in memory; no tile is empty; one tile
// less would not cover.
static void check_tiles()
{
    const long long totals[] = {1, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 7};
    for (int lead = 0; lead < 16; ++lead)
        for (const long long total : totals) {
            // the caller's buffer with a guard tile either side: an index outside it is an error of the rule, and one
            // outside the vector is the sanitizer's to report
            std::vector<int> stored((size_t)(total + 2 * kImageTile), 0);
            int *const at0 = stored.data() + kImageTile;
            const long long n_tiles = image_tiles(total, lead);
            CHECK(n_tiles >= 1, "lead %d total %lld", lead, total);
            CHECK((n_tiles - 1) * kImageTile - lead < total, "lead %d total %lld: a tile too many", lead, total);
            CHECK(n_tiles * kImageTile - lead >= total, "lead %d total %lld: a tile too few", lead, total);
            for (long long tile = 0; tile < n_tiles; ++tile) {
                const TileSpan s = tile_span(tile, lead, total);
                CHECK((s.t_begin + lead) % kImageTile == 0, "lead %d total %lld tile %lld", lead, total, tile);
                CHECK(s.o_begin < s.o_end, "lead %d total %lld tile %lld is empty", lead, total, tile);
                CHECK(s.o_begin >= 0 && s.o_end <= total && s.o_begin >= s.t_begin && s.o_end <= s.t_begin + kImageTile,
                      "lead %d total %lld tile %lld", lead, total, tile);
                for (int tid = 0; tid < kImageThreads; ++tid) {
                    // store_image's own steps, with a count in place of the store
                    const long long at = lane_at(s, tid);
                    CHECK(at == s.t_begin + 16 * tid, "lead %d total %lld tile %lld lane %d", lead, total, tile, tid);
                    const bool vector = lane_vector(s, at);
                    if (vector)
                        CHECK((lead + at) % 16 == 0, "lead %d total %lld tile %lld lane %d: vector store at %lld", lead,
                              total, tile, tid, at);
                    for (int b = 0; b < 16; ++b)
                        if (vector || lane_byte(s, at, b)) {
                            CHECK(at + b >= 0 && at + b < total, "lead %d total %lld tile %lld lane %d: byte %lld is not the caller's",
                                  lead, total, tile, tid, at + b);
                            ++at0[at + b];
                        }
                }
            }
            for (long long i = -kImageTile; i < total + kImageTile; ++i)
                CHECK(at0[i] == (i >= 0 && i < total ? 1 : 0), "lead %d total %lld: byte %lld stored %d times", lead, total, i,
                      at0[i]);
        }
    alignas(16) static const char probe[32] = {};
    for (int lead = 0; lead < 16; ++lead)
        CHECK(image_lead(probe + lead) == lead, "lead %d", lead);
}

// 2. philox_block is philox4x32_10 with the index split by hand: the known answers of tests/test_simulate_cpu.py, and an
// index beyond 2^32 on every named stream.
static void check_stream()
{
    struct Known {
        uint32_t c[4], k[2], want[4];
    };
    const Known known[] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
         {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
         {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (const Known &kn : known) {
        uint32_t direct[4], block[4];
        philox4x32_10(kn.c[0], kn.c[1], kn.c[2], kn.c[3], kn.k[0], kn.k[1], direct);
        philox_block((uint64_t)kn.c[0] | ((uint64_t)kn.c[1] << 32), kn.c[2], kn.c[3], PhiloxKey{kn.k[0], kn.k[1]}, block);
        for (int i = 0; i < 4; ++i)
            CHECK(direct[i] == kn.want[i] && block[i] == kn.want[i], "known answer, word %d: %08x %08x, want %08x", i,
                  direct[i], block[i], kn.want[i]);
    }
    const uint32_t streams[] = {kStreamRead,   kStreamGenome,  kStreamKeep,      kStreamFamily,
                                kStreamCopies, kStreamShuffle, kStreamDivergence};
    for (int s = 0; s < 7; ++s)
        CHECK(streams[s] == (uint32_t)s, "stream %d is numbered %u", s, streams[s]);
    const uint64_t seed = 0x0123456789abcdefull, index = ((uint64_t)7 << 32) + 0x89abcdefull;
    const PhiloxKey key = philox_key(seed);
    CHECK(key.k0 == 0x89abcdefu && key.k1 == 0x01234567u, "philox_key: %08x %08x", key.k0, key.k1);
    for (const uint32_t stream : streams)
        for (const uint32_t c2 : {0u, 1u, 64u}) {
            uint32_t direct[4], block[4];
            philox4x32_10(0x89abcdefu, 7u, c2, stream, 0x89abcdefu, 0x01234567u, direct);
            philox_block(index, c2, stream, key, block);
            for (int i = 0; i < 4; ++i)
                CHECK(direct[i] == block[i], "stream %u c2 %u word %d", stream, c2, i);
        }
}

// 3. the base code: the four bases in both cases, their characters, and the substitution's three others
static void check_bases()
{
    const char upper[] = "ACGT", lower[] = "acgt";
    for (uint32_t c = 0; c < 4; ++c) {
        CHECK(code_of((unsigned char)upper[c]) == c && code_of((unsigned char)lower[c]) == c, "code_of %c", upper[c]);
        CHECK(char_of(c) == (uint32_t)upper[c], "char_of %u", c);
    }
    CHECK(pack_chars(0, 1, 2, 3) == kAcgt && pack_chars(3, 2, 1, 0) == 0x41434754u, "pack_chars");
    for (uint32_t c = 0; c < 4; ++c) {
        unsigned reached = 0;
        for (uint32_t w = 0; w < 3000; ++w) {
            const uint32_t word = w * 0x9E3779B1u; // (spread over the 32 bits: mod3 sees all of them)
            CHECK(mod3(word) == word % 3u, "mod3 %u", word);
            const uint32_t sub = substituted(c, word, (uint64_t)1 << 32); // rate 1: every word is below
            CHECK(sub < 4 && sub != c, "substituted(%u, %u) = %u", c, word, sub);
            CHECK(sub == ((c + 1u + word % 3u) & 3u), "substituted(%u, %u) = %u", c, word, sub);
            reached |= 1u << sub;
            CHECK(substituted(c, word, 0) == c, "rate 0 substitutes");
            CHECK(substituted(c, word, (uint64_t)word) == c && substituted(c, word, (uint64_t)word + 1) == sub,
                  "the threshold is exclusive");
        }
        CHECK(reached == (0xfu & ~(1u << c)), "substituted(%u, .) reaches %x", c, reached);
    }
}

int main()
{
    check_tiles();
    check_stream();
    check_bases();
    std::printf("tile image, stream and base code: ok\n");
    return 0;
}
