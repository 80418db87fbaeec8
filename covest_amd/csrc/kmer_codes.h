// kmer_codes.h -- the arithmetic on 2-bit base codes that the k-mer counters share (kmer_table.h includes it), once
// each and in plain C++: the host compiler builds it too, and tests/kmer_stages_check.cpp runs it under sanitizers.
// A code holds base j at bits 2j ("little-endian") unless it says otherwise.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMER_HD __host__ __device__ __forceinline__
#else
#define KMER_HD inline
#endif

namespace covest {
namespace kmer {

// ASCII base -> 2-bit code for a/c/g/t in either case: bits 2:1 give a=0 c=1 t=2 g=3; x ^ (x>>1) swaps g,t.
KMER_HD unsigned base_code(unsigned char ch)
{
    const unsigned x = (ch >> 1) & 3u;
    return x ^ (x >> 1);
}

// four ASCII bases -> one byte of 2-bit codes (base j at bits 2j)
KMER_HD unsigned pack4(unsigned w)
{
    unsigned x = (w >> 1) & 0x03030303u;
    x ^= (x >> 1) & 0x01010101u;
    return (x * 0x01041040u) >> 24;
}

// the low 2k bits: a k-mer's code
KMER_HD unsigned long long kmer_mask(int k)
{
    return k < 32 ? (1ull << (2 * k)) - 1ull : ~0ull;
}

// the low n bases of a code
KMER_HD unsigned long long low_bases(unsigned long long code, int n)
{
    return code & kmer_mask(n);
}

// All bits of a word in reverse order: one instruction on the device, the ladder of swaps for the host compiler.
KMER_HD unsigned reverse_bits32(unsigned x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __brev(x);
#else
    x = (x >> 16) | (x << 16);
    x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
#endif
}

KMER_HD unsigned long long reverse_bits64(unsigned long long x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __brevll(x);
#else
    return ((unsigned long long)reverse_bits32((unsigned)x) << 32) | reverse_bits32((unsigned)(x >> 32));
#endif
}

// The 2-bit pairs of a word in reverse order: the bits reversed, then the two bits of every pair swapped back.  The
// reverse complement of the n >= 1 bases of x, as a little-endian code: reverse_pairs(~x) >> (bits - 2n) -- the bits
// of ~x above 2n leave at the bottom.
KMER_HD unsigned reverse_pairs32(unsigned x)
{
    const unsigned r = reverse_bits32(x);
    return ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);
}

KMER_HD unsigned long long reverse_pairs64(unsigned long long x)
{
    const unsigned long long r = reverse_bits64(x);
    return ((r & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((r & 0x5555555555555555ull) << 1);
}

// the same base by base: the code of the reverse complement of the k-mer coded by x
KMER_HD unsigned long long revcomp_code(unsigned long long x, int k)
{
    unsigned long long rc = 0;
    for (int i = 0; i < k; ++i) {
        rc = (rc << 2) | (3ull - (x & 3ull));
        x >>= 2;
    }
    return rc;
}

// The slot a key's probes start from in an LDS table of smask + 1 slots (pass 2 of kmer_bulk.hip): every bit of the
// key reaches the product's upper half, the slot is taken from there.
KMER_HD unsigned lds_slot(unsigned long long key, unsigned smask)
{
    const unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
    const unsigned x = (lo ^ (hi << 15) ^ (hi >> 5) ^ (hi << 27)) * 0x9E3779B1u;
    return (x >> 12) & smask;
}

} // namespace kmer
} // namespace covest
