// kmer_influence.hip -- the delete-one-read influence rows and the moments of such rows: what each output holds, the
// multiplicity rule and the fixed order of every sum are stated in kmer_influence.h.
//
// Bound of the influence kernel: per read ceil(W / 64)^2 stagings of 64 keys (a key derivation and 64 broadcast LDS
// compares a lane each), and one scattered 16-byte load (table_find's first slot) per FIRST window -- the lookup's
// load, plus the stagings.
#include "kmer_influence.h"

#include "wave_read.h"

// the rows are held bit for bit against a restatement: no a * b + c may become an fma in this file
#pragma clang fp contract(off)

namespace covest {

namespace {

using namespace kmer;

constexpr unsigned long long kAbsentKey = ~0ull; // (a key of k <= 31 has at most 62 bits)

// What a wave has written to its own LDS row is read by its other lanes, and the other way round: LDS operations of one
// wave complete in order, the fence keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void kmer_read_influence_kernel(const unsigned char *__restrict__ bases,
                                                                  const int64_t *__restrict__ offsets, int64_t n_reads,
                                                                  int64_t fixed_len, int canonical, const KmerTable t,
                                                                  const double *__restrict__ table, int64_t n_rows,
                                                                  int n_cols, double *__restrict__ rows)
{
    __shared__ unsigned long long staged[kWaveReadsPerBlock][kWave];
    const int k = t.k;
    WaveRead w;
    if (!wave_read(bases, offsets, n_reads, fixed_len, k, w)) // (no workgroup barrier below)
        return;
    const int lane = w.lane;
    const int64_t n_windows = w.n_windows;
    double *out = rows + w.r * (n_cols + 1);
    if (n_windows > kInfluenceMaxWindows) {
        if (lane == 0) {
            for (int col = 0; col < n_cols; ++col)
                out[col] = __builtin_nan("");
            out[n_cols] = (double)n_windows;
        }
        return;
    }

    unsigned long long *keys = staged[threadIdx.x / kWave];
    const unsigned long long top = (unsigned long long)(n_rows - 1);
    const int n_chunks = (int)((n_windows + kWave - 1) / kWave);
    double partial[kInfluenceMaxCols];
#pragma unroll
    for (int col = 0; col < kInfluenceMaxCols; ++col)
        partial[col] = 0.0;
    for (int c = 0; c < n_chunks; ++c) { // the lane's own window of chunk c
        const int64_t s = (int64_t)c * kWave + lane;
        const bool own = s < n_windows;
        unsigned long long h = kAbsentKey, rc = 0;
        if (own)
            window_key(w.seq, s, w.len, k, canonical, h, rc);
        unsigned m = 0;
        bool earlier = false;
        for (int d = 0; d < n_chunks; ++d) { // against the 64 windows of chunk d
            unsigned long long other = h;
            if (d != c) {
                const int64_t s2 = (int64_t)d * kWave + lane;
                other = kAbsentKey;
                if (s2 < n_windows) {
                    unsigned long long rc2;
                    window_key(w.seq, s2, w.len, k, canonical, other, rc2);
                }
            }
            wave_lds_sync(); // (the compares of the chunk before are done)
            keys[lane] = other;
            wave_lds_sync();
            const int before = d < c ? kWave : d == c ? lane : 0; // staged windows j < before come before window s
#pragma unroll 8
            for (int j = 0; j < kWave; ++j) {
                const bool same = keys[j] == h; // (one address across the wave: a broadcast)
                m += same ? 1u : 0u;
                earlier = earlier || (same && j < before);
            }
        }
        if (own && !earlier) {
            const unsigned long long a = table_find(t, h, rc);
            const unsigned long long left = a > m ? a - m : 0ull;
            const double *after = table + (left < top ? left : top) * (unsigned long long)n_cols;
            const double *now = table + (a < top ? a : top) * (unsigned long long)n_cols;
#pragma unroll
            for (int col = 0; col < kInfluenceMaxCols; ++col)
                if (col < n_cols)
                    partial[col] = partial[col] + (after[col] - now[col]);
        }
    }
#pragma unroll
    for (int col = 0; col < kInfluenceMaxCols; ++col) {
        if (col < n_cols) { // (wave-uniform)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
                partial[col] = partial[col] + __shfl_xor(partial[col], off, kWave);
            if (lane == 0)
                out[col] = partial[col];
        }
    }
    if (lane == 0)
        out[n_cols] = (double)n_windows;
}

// ---- moments ---------------------------------------------------------------------------------------------------------
constexpr int kMomentsThreads = 256;

template <int Q> constexpr int width() { return Q + Q * (Q + 1) / 2; }

// v += (d, the upper triangle of d d^T), d = row - centre
template <int Q> __device__ __forceinline__ void add_row(double (&v)[width<Q>()], const double *__restrict__ row,
                                                         const double *__restrict__ centre)
{
    double d[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        d[k] = row[k] - centre[k];
        v[k] = v[k] + d[k];
    }
    int at = Q; // (row by row over k <= l: pair_index's order)
#pragma unroll
    for (int k = 0; k < Q; ++k)
#pragma unroll
        for (int l = k; l < Q; ++l, ++at)
            v[at] = v[at] + d[k] * d[l];
}

// The block's fold of kmer_influence.h: the butterfly in each wave, then the four waves in ascending order.  Entry i of
// the result goes to out_a[i] for i < Q and to out_b[i - Q] behind.
template <int Q> __device__ __forceinline__ void block_fold(double (&v)[width<Q>()], double *out_a, double *out_b)
{
    constexpr int W = width<Q>();
    constexpr int kWaves = kMomentsThreads / kWave;
    __shared__ double part[kWaves][W];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < W; ++i) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            v[i] = v[i] + __shfl_xor(v[i], off, kWave);
        if (lane == 0)
            part[wave][i] = v[i];
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < W) {
        double total = part[0][i];
        for (int w = 1; w < kWaves; ++w)
            total = total + part[w][i];
        if (i < Q)
            out_a[i] = total;
        else
            out_b[i - Q] = total;
    }
}

template <int Q> __global__ __launch_bounds__(kMomentsThreads) void rows_moments_blocks_kernel(
    const double *__restrict__ rows, int64_t n, const double *__restrict__ centre, double *__restrict__ partials)
{
    constexpr int W = width<Q>();
    double v[W];
#pragma unroll
    for (int i = 0; i < W; ++i)
        v[i] = 0.0;
    const int64_t first = (int64_t)blockIdx.x * kMomentsBlockRows;
#pragma unroll
    for (int j = 0; j < kMomentsBlockRows / kMomentsThreads; ++j) {
        const int64_t row = first + j * kMomentsThreads + threadIdx.x;
        if (row < n)
            add_row<Q>(v, rows + row * Q, centre);
    }
    double *out = partials + (int64_t)blockIdx.x * W;
    block_fold<Q>(v, out, out + Q);
}

template <int Q> __global__ __launch_bounds__(kMomentsThreads) void rows_moments_final_kernel(
    const double *__restrict__ partials, int64_t n_blocks, double *__restrict__ sum, double *__restrict__ cross)
{
    constexpr int W = width<Q>();
    double v[W];
#pragma unroll
    for (int i = 0; i < W; ++i)
        v[i] = 0.0;
    for (int64_t b = threadIdx.x; b < n_blocks; b += kMomentsThreads) {
#pragma unroll
        for (int i = 0; i < W; ++i)
            v[i] = v[i] + partials[b * W + i];
    }
    block_fold<Q>(v, sum, cross);
}

template <int Q> hipError_t launch_moments_q(const double *rows, int64_t n, const double *centre, double *sum, double *cross,
                                            double *partials, hipStream_t stream)
{
    const int64_t n_blocks = (n + kMomentsBlockRows - 1) / kMomentsBlockRows;
    if (n_blocks > 0)
        hipLaunchKernelGGL(rows_moments_blocks_kernel<Q>, dim3((unsigned)n_blocks), dim3(kMomentsThreads), 0, stream, rows, n,
                           centre, partials);
    hipLaunchKernelGGL(rows_moments_final_kernel<Q>, dim3(1), dim3(kMomentsThreads), 0, stream, partials, n_blocks, sum, cross);
    return hipGetLastError();
}

} // namespace

hipError_t launch_kmer_read_influence(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                                      int canonical, const KmerTable &t, const double *table, int64_t n_rows, int n_cols,
                                      double *rows, hipStream_t stream)
{
    kmer_plan::for_each_wave_launch(n_reads, fixed_len, offsets != nullptr, kWaveReadsPerBlock, [&](const kmer_plan::WaveLaunch &l) {
        hipLaunchKernelGGL(kmer_read_influence_kernel, dim3((unsigned)l.blocks), dim3(kWaveReadsPerBlock * kWave), 0, stream,
                           bases + l.byte_at, offsets ? offsets + l.first : nullptr, l.n, fixed_len, canonical, t, table, n_rows,
                           n_cols, rows + l.first * (n_cols + 1));
    });
    return hipGetLastError();
}

hipError_t launch_rows_moments(const double *rows, int64_t n, int q, const double *centre, double *sum, double *cross,
                               void *scratch, hipStream_t stream)
{
    double *partials = static_cast<double *>(scratch);
    switch (q) {
#define COVEST_MOMENTS_CASE(Q) \
    case Q:                    \
        return launch_moments_q<Q>(rows, n, centre, sum, cross, partials, stream);
        COVEST_MOMENTS_CASE(1)
        COVEST_MOMENTS_CASE(2)
        COVEST_MOMENTS_CASE(3)
        COVEST_MOMENTS_CASE(4)
        COVEST_MOMENTS_CASE(5)
        COVEST_MOMENTS_CASE(6)
        COVEST_MOMENTS_CASE(7)
        COVEST_MOMENTS_CASE(8)
        COVEST_MOMENTS_CASE(9)
#undef COVEST_MOMENTS_CASE
    default:
        return hipErrorInvalidValue;
    }
}

} // namespace covest
