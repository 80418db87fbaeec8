// kmer_correct.hip -- isolated substitutions corrected from the k-mer table: the rule, the outputs and why every output
// byte is stored exactly once are stated in kmer_correct.h.
//
// One wave64 a read, four reads a workgroup.  The wave walks the windows in chunks of 64, lane l on window 64c + l;
// __ballot(weak) hands the chunk's mask to every lane as a wave-uniform value, and a wave-uniform state (run open, its
// first window) carried from chunk to chunk closes the runs with count-trailing-zeros arithmetic.  A closed run of at
// most k <= 31 windows lies in chunk c or straddles c - 1 | c, so the codes of chunk c - 1 stay in a register: a trial
// lane takes its window's code from the lane that walked it (a shuffle), never from the bytes again.  Two alternatives
// are tried at a time, lanes 0..31 and 32..63 on the run's windows; an alternative patches the two bits of its base in
// the window's little-endian code and derives both strands' codes from that (codes_from_le, as window_codes does).
//
// Bound: the lookup's one scattered 16-byte load a window, plus, for a run of n windows that names a position, 3 n such
// loads (the whole-read case of a short read: 3 n a position).  Measured beside the lookup: DESIGN.md section 6af.
#include "kmer_correct.h"

#include "wave_read.h"

namespace covest {

namespace {

using namespace kmer;

enum Verdict { kUnfixable = 0, kCorrected = 1, kAmbiguous = 2 };

// The run [f, l] of a read of `len` bases judged (rule 3 to 5 of kmer_correct.h); everything but `lane`, `le_cur` and
// `le_prev` is wave-uniform.  le_cur / le_prev: the little-endian code of this lane's window of chunk c / c - 1.
// kCorrected: base `p` becomes code `b`.
__device__ __forceinline__ Verdict judge_run(const KmerTable &t, int canonical, uint32_t cutoff, int lane, int64_t f,
                                             int64_t l, int64_t len, int64_t c, unsigned long long le_cur,
                                             unsigned long long le_prev, int64_t &p, unsigned &b)
{
    const int k = t.k;
    const int64_t last = len - k, n = l - f + 1;
    if (n > k)
        return kUnfixable;
    int64_t p_lo, p_hi;
    if (f > 0) {
        p_lo = p_hi = f + k - 1;
        if (l != (p_lo < last ? p_lo : last))
            return kUnfixable;
    } else if (l < last) {
        p_lo = p_hi = l;
    } else {
        p_lo = last;
        p_hi = k - 1 < len - 1 ? k - 1 : len - 1;
    }
    const int half = lane >> 5, j = lane & 31;
    const int64_t s = f + j;                 // this lane's window of the run, if j < n
    const bool has_window = j < n;
    const int src = (int)(s & (kWave - 1));  // l - 30 <= f and 64c - 1 <= l <= 64c + 63: s is in chunk c - 1 or c
    const unsigned long long from_cur = __shfl(le_cur, src, kWave), from_prev = __shfl(le_prev, src, kWave);
    const unsigned long long le = (s >> 6) == c ? from_cur : from_prev;
    const int n_alt = 3 * (int)(p_hi - p_lo + 1);
    int n_valid = 0;
    for (int first = 0; first < n_alt && n_valid < 2; first += 2) {
        const int a = first + half;            // this half's alternative: position p_lo + a / 3, the (a % 3)-th other base
        const int64_t at = p_lo + a / 3;
        bool ok = true;
        unsigned other = 0;
        if (has_window && a < n_alt) {
            const int i = (int)(at - s);       // 0 <= i < k: the windows that cover `at` are exactly [f, l]
            const unsigned own = (unsigned)(le >> (2 * i)) & 3u;
            other = (own + 1u + (unsigned)(a % 3)) & 3u;
            unsigned long long h, rc;
            codes_from_le(le ^ ((unsigned long long)(own ^ other) << (2 * i)), k, h, rc);
            canonical_pair(h, rc, canonical);
            ok = table_find(t, h, rc) >= (unsigned long long)cutoff;
        }
        const unsigned long long good = __ballot(ok);
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            if (first + side < n_alt && (uint32_t)(good >> (32 * side)) == 0xFFFFFFFFu) {
                ++n_valid;
                p = p_lo + (first + side) / 3;
                b = (unsigned)__builtin_amdgcn_readlane((int)other, 32 * side); // (lane 32 side: window f, n >= 1)
            }
        }
    }
    return n_valid == 1 ? kCorrected : n_valid ? kAmbiguous : kUnfixable;
}

// the letter of code (fix - 1) in the case of `old`
__device__ __forceinline__ unsigned char fixed_letter(unsigned char old, unsigned fix)
{
    return (unsigned char)(((0x54474341u >> (8u * (fix - 1u))) & 0xFFu) | (old & 0x20u)); // "ACGT"
}

// (`bases` and `out` may be one pointer: neither is __restrict__)
__global__ __launch_bounds__(256) void kmer_correct_kernel(const unsigned char *bases, const int64_t *__restrict__ offsets,
                                                           int64_t n_reads, int64_t fixed_len, int canonical,
                                                           const KmerTable t, uint32_t cutoff, unsigned char *out,
                                                           uint32_t *__restrict__ fix)
{
    // wave_read.h's opening with the wave index made scalar (readfirstlane): with the plain index the other four kernels
    // share, this one takes 75 VGPRs for 44 and loses a wave of occupancy; with the scalar one the lookup is 7 % slower
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * kWaveReadsPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    if (r >= n_reads) // (the whole wave: a wave is a read)
        return;
    const int64_t p0 = offsets ? offsets[r] : r * fixed_len;
    const int64_t len = offsets ? offsets[r + 1] - p0 : fixed_len;
    const unsigned char *seq = bases + p0;
    const bool in_place = out == bases;
    const int k = t.k;
    const int64_t n_windows = len >= k ? len - k + 1 : 0;
    const int64_t window_chunks = (n_windows + kWave - 1) >> 6, byte_chunks = (len + kWave - 1) >> 6;

    uint32_t runs = 0, corrected = 0, ambiguous = 0;
    bool open = false; // wave-uniform: a run is open, and its first window
    int64_t f = 0;
    unsigned long long le_prev = 0;
    // code + 1 of the correction to byte 64(c - 1) + lane, 64c + lane, 64(c + 1) + lane (0: none): a run closed in
    // chunk c has 64c - 1 <= l <= 64c + 63 and l <= p <= l + k - 1, so its base lies in one of the three
    unsigned fix0 = 0, fix1 = 0, fix2 = 0;
    for (int64_t c = 0; c <= byte_chunks; ++c) {
        unsigned long long le_cur = 0;
        if (c < window_chunks) {
            const int64_t base = c << 6, s = base + lane;
            bool weak = false;
            if (s < n_windows) {
                unsigned long long h, rc;
                window_codes(seq, s, len, k, h, rc); // (window_key in two steps: le_cur is rc before the canonical swap)
                le_cur = ~rc & kmer_mask(k);
                canonical_pair(h, rc, canonical);
                weak = table_find(t, h, rc) < (unsigned long long)cutoff;
            }
            const unsigned long long m = __ballot(weak);
            const int valid = n_windows - base < kWave ? (int)(n_windows - base) : kWave; // windows of this chunk
            int at = 0;
            for (;;) {
                if (!open) {
                    const unsigned long long rest = m >> at;
                    if (!rest)
                        break;
                    at += __builtin_ctzll(rest);
                    open = true;
                    f = base + at;
                }
                const unsigned long long strong = ~m >> at; // (bits from `valid` on are set: no window is not weak)
                const int e = strong ? at + __builtin_ctzll(strong) : kWave;
                if (e >= valid && c + 1 < window_chunks)
                    break; // the run goes on in the next chunk
                const int64_t l = e >= valid ? n_windows - 1 : base + e - 1;
                int64_t p = 0;
                unsigned b = 0;
                const Verdict v = judge_run(t, canonical, cutoff, lane, f, l, len, c, le_cur, le_prev, p, b);
                ++runs;
                corrected += v == kCorrected;
                ambiguous += v == kAmbiguous;
                if (v == kCorrected && lane == (int)(p & (kWave - 1))) {
                    const int d = (int)((p >> 6) - c); // -1, 0, 1
                    fix0 = d < 0 ? b + 1u : fix0;
                    fix1 = d == 0 ? b + 1u : fix1;
                    fix2 = d > 0 ? b + 1u : fix2;
                }
                open = false;
                if (e >= valid)
                    break;
                at = e; // (< 64)
            }
        }
        if (c >= 1) { // bytes 64(c - 1) .. 64c - 1: no later run reaches them
            const int64_t q = ((c - 1) << 6) + lane;
            if (q < len) {
                if (!in_place)
                    out[p0 + q] = fix0 ? fixed_letter(seq[q], fix0) : seq[q];
                else if (fix0)
                    out[p0 + q] = fixed_letter(seq[q], fix0);
            }
        }
        fix0 = fix1;
        fix1 = fix2;
        fix2 = 0;
        le_prev = le_cur;
    }
    if (fix && lane == 0)
        reinterpret_cast<uint4 *>(fix)[r] = make_uint4(runs, corrected, ambiguous, runs - corrected - ambiguous);
}

} // namespace

hipError_t launch_kmer_correct(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                               int canonical, const KmerTable &t, uint32_t cutoff, unsigned char *out, uint32_t *fix,
                               hipStream_t stream)
{
    kmer_plan::for_each_wave_launch(n_reads, fixed_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        hipLaunchKernelGGL(kmer_correct_kernel, dim3((unsigned)l.blocks), dim3(kWaveReadsPerBlock * kWave), 0, stream,
                           bases + l.byte_at, offsets ? offsets + l.first : nullptr, l.n, fixed_len, canonical, t, cutoff,
                           out + l.byte_at, fix ? fix + 4 * l.first : nullptr); // (out as bases: in place is out == bases)
    });
    return hipGetLastError();
}

} // namespace covest
