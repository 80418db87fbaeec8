// kmer_lookup.hip -- per-read k-mer abundance lookup against the table of kmer_count.hip: what each output holds, the
// fixed order of the score's sum and the deliberate difference for reads shorter than k are stated in kmer_lookup.h.
//
// Bound: one scattered 16-byte load a window (table_find's first slot; neighbouring windows mostly share their line,
// kmer_table.h), against the add's load, sometimes a CAS, and an atomic add to the same line.
#include "kmer_lookup.h"

#include "wave_read.h"

namespace covest {

namespace {

using namespace kmer;

__global__ __launch_bounds__(256) void kmer_lookup_kernel(const unsigned char *__restrict__ bases,
                                                          const int64_t *__restrict__ offsets, int64_t n_reads,
                                                          int64_t fixed_len, int canonical, const KmerTable t,
                                                          uint32_t cutoff, const double *__restrict__ weights,
                                                          int n_weights, uint32_t *__restrict__ abundance,
                                                          uint32_t *__restrict__ summary, double *__restrict__ score)
{
    const int k = t.k;
    WaveRead w;
    if (!wave_read(bases, offsets, n_reads, fixed_len, k, w))
        return;

    uint32_t lowest = kNoWindow, weak = 0, first_weak = kNoWindow, last_weak_1 = 0; // (last weak window + 1; 0: none)
    double partial = 0.0;
    for (int64_t s = w.lane; s < w.len; s += kWave) {
        uint32_t a = kNoWindow;
        if (s < w.n_windows) {
            unsigned long long h, rc;
            window_key(w.seq, s, w.len, k, canonical, h, rc);
            const unsigned long long count = table_find(t, h, rc);
            a = count < (unsigned long long)(kNoWindow - 1) ? (uint32_t)count : kNoWindow - 1;
            lowest = a < lowest ? a : lowest;
            if (a < cutoff) {
                ++weak;
                first_weak = first_weak == kNoWindow ? (uint32_t)s : first_weak; // (ascending: the first stays)
                last_weak_1 = (uint32_t)s + 1u;
            }
            if (score) {
                const unsigned long long top = (unsigned long long)(n_weights - 1);
                partial = partial + weights[count < top ? count : top];
            }
        }
        if (abundance)
            abundance[w.p0 + s] = a;
    }
    if (!summary && !score)
        return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o_low = __shfl_xor(lowest, off, kWave), o_first = __shfl_xor(first_weak, off, kWave);
        const uint32_t o_last = __shfl_xor(last_weak_1, off, kWave);
        lowest = o_low < lowest ? o_low : lowest;
        first_weak = o_first < first_weak ? o_first : first_weak;
        last_weak_1 = o_last > last_weak_1 ? o_last : last_weak_1;
        weak += __shfl_xor(weak, off, kWave);
        partial = partial + __shfl_xor(partial, off, kWave);
    }
    if (w.lane == 0) {
        if (summary)
            reinterpret_cast<uint4 *>(summary)[w.r] = make_uint4(lowest, weak, first_weak, last_weak_1 - 1u); // (0 - 1: none)
        if (score)
            score[w.r] = partial;
    }
}

} // namespace

hipError_t launch_kmer_lookup(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                              int canonical, const KmerTable &t, uint32_t cutoff, const double *weights, int n_weights,
                              uint32_t *abundance, uint32_t *summary, double *score, hipStream_t stream)
{
    kmer_plan::for_each_wave_launch(n_reads, fixed_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        hipLaunchKernelGGL(kmer_lookup_kernel, dim3((unsigned)l.blocks), dim3(kWaveReadsPerBlock * kWave), 0, stream,
                           bases + l.byte_at, offsets ? offsets + l.first : nullptr, l.n, fixed_len, canonical, t, cutoff, weights,
                           n_weights, abundance ? abundance + l.byte_at : nullptr, summary ? summary + 4 * l.first : nullptr,
                           score ? score + l.first : nullptr);
    });
    return hipGetLastError();
}

} // namespace covest
