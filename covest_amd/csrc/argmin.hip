// argmin.hip -- K-argmin: (min -LL, lowest flat index attaining it) over the LL
// buffer of one GPU's block of the grid.
//
// Restates the selection scan of covest/grid.py:65-70 (maximize=False) started
// from +inf:  `if val < min_val` is STRICT, so the lowest index wins ties, NaN
// never wins, +inf (LL = -inf) never wins, -inf (LL = +inf) does.
//
// HBM-bound streaming read of 8 bytes per grid point, two launches: a
// grid-stride pass of at most 256 workgroups (one per CU) that leaves one
// candidate per workgroup, then one workgroup over the candidates.  No
// atomics, so the result is deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cand.h"
#include "kernels.h"
#include "wave.h"

namespace covest {

namespace {

__device__ __forceinline__ Cand block_best(Cand c)
{
    __shared__ double sv[16];
    __shared__ int64_t si[16];
    c = wave_best(c);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) {
        sv[w] = c.v;
        si[w] = c.i;
    }
    __syncthreads();
    const int n_w = blockDim.x / kWave;
    Cand r;
    r.v = (threadIdx.x < n_w) ? sv[threadIdx.x] : INFINITY;
    r.i = (threadIdx.x < n_w) ? si[threadIdx.x] : INT64_MAX;
    return wave_best(r); // valid in wave 0
}

__global__ __launch_bounds__(256) void argmin_stage1(const double *__restrict__ ll, int64_t n,
                                                     double *__restrict__ pv, int64_t *__restrict__ pi)
{
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = -ll[i];
        // ascending i within a thread: strict < keeps the first occurrence
        if (v < c.v) {
            c.v = v;
            c.i = i;
        }
    }
    c = block_best(c);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = c.v;
        pi[blockIdx.x] = c.i;
    }
}

// The winner where it is wanted: in HBM (the ranks' exchange reads it there) and, when the caller gave one, in a
// page-locked HOST mirror -- the kernel's own store, visible once the stream is synchronised: no copy launch and no
// staging for 16 bytes.
__device__ __forceinline__ void publish(Cand c, int64_t flat_begin, ArgminResult *__restrict__ result,
                                        ArgminResult *__restrict__ host_mirror, bool unproven = false)
{
    ArgminResult r;
    r.min_negll = c.v;
    r.index = (c.i == INT64_MAX) ? -1 : c.i;
    r.unproven = unproven ? 1 : 0;
    // the same as a pair of doubles with the GLOBAL flat index, for the cross-GPU exchange (flat indices
    // stay below 2^53)
    r.pair[0] = c.v;
    r.pair[1] = (c.i == INT64_MAX) ? -1.0 : (double)(flat_begin + c.i);
    *result = r;
    if (host_mirror)
        *host_mirror = r;
}

// The hand-back queue of the launch before, taken over by thread 0: its length goes to the control word BEHIND the
// counter -- where a strict re-evaluation that was put off (abi_grid.cpp grid_complete) finds it -- and the counter starts
// empty again.  Returns the length to thread 0; every thread reads it from *s_queued behind the next barrier.
__device__ __forceinline__ void take_queue(unsigned *__restrict__ queue_count, unsigned *s_queued)
{
    if (threadIdx.x != 0)
        return;
    unsigned q = 0;
    if (queue_count) {
        q = queue_count[0];
        queue_count[1] = q;
        queue_count[0] = 0;
    }
    *s_queued = q;
}

// IS THE WINNER THE FINAL ONE while the queued points still hold their provisional values?  (The strict re-evaluation put
// off: abi_grid.cpp.)  ll_fix.hip forms a queued point's final value by ADDING h_j (safe_log(p_j) - log p_clamp) <= 0, row
// by row, to the provisional one, and touches no other point: a queued point's provisional -LL is a lower bound of its
// final -LL, everybody else's value is final.  So the winner (v_w, i_w) over the provisional values stands under the
// selection rule (strict <, lowest index, NaN never) unless it is queued itself or a queued point's provisional -LL
// reaches v_w + 1e-9 |v_w| -- a safety margin, not a measurement: it covers the rounding of the pass's own adds (a
// contribution whose device log lands an ulp above the host's log p_clamp) and exact ties.  A false alarm costs the
// caller the strict pass and a second arg-min, nothing else.  Nothing won (every value +inf or NaN): a queued point's
// -LL only rises, nothing can win afterwards either.  v_w = -inf: the bound is NaN and only the winner's own entry
// counts -- a queued -inf at a lower index would have won, at a higher one it cannot.
// `c` as block_best left it (thread 0's counts); a workgroup-wide answer.
__device__ __forceinline__ bool winner_unproven(Cand c, const double *__restrict__ ll, const int64_t *__restrict__ queue_index,
                                                const unsigned *s_queued)
{
    __shared__ double win_v;
    __shared__ int64_t win_i;
    if (threadIdx.x == 0) {
        win_v = c.v;
        win_i = c.i;
    }
    __syncthreads();
    const double v_w = win_v;
    const int64_t i_w = win_i;
    const unsigned queued = *s_queued;
    int threat = 0;
    if (i_w != INT64_MAX) {
        const double bound = v_w + 1e-9 * fabs(v_w);
        // an entry is two dependent loads (the index, then the value): four entries' loads a thread are issued together,
        // as small_grid_values does (one after the other, 256 threads: 0.6 us an entry and thread -- C2's 7 791 entries
        // 18 us, more than the pass they spare the step)
        for (unsigned base = threadIdx.x; base < queued; base += 4 * blockDim.x) {
            int64_t i[4];
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned q = base + (unsigned)u * blockDim.x;
                i[u] = q < queued ? queue_index[q] : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = i[u] >= 0 ? -ll[i[u]] : INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                threat |= (v[u] <= bound || i[u] == i_w) ? 1 : 0;
        }
    }
    return __syncthreads_or(threat) != 0;
}

// (256 threads; 1 024 where it walks the queue: launch_argmin_proving)
__global__ __launch_bounds__(1024) void argmin_stage2(const double *__restrict__ ll, const int64_t *__restrict__ queue_index,
                                                     const double *__restrict__ pv,
                                                     const int64_t *__restrict__ pi, int n_part, int64_t flat_begin,
                                                     ArgminResult *__restrict__ result, ArgminResult *__restrict__ host_mirror,
                                                     unsigned *__restrict__ queue_count)
{
    __shared__ unsigned s_queued;
    take_queue(queue_count, &s_queued); // (drained by ll_fix_list_kernel already, or -- queue_index given -- still to be)
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    for (int i = threadIdx.x; i < n_part; i += blockDim.x) {
        Cand o;
        o.v = pv[i];
        o.i = pi[i];
        c = better(c, o);
    }
    c = block_best(c);
    const bool unproven = queue_index ? winner_unproven(c, ll, queue_index, &s_queued) : false; // (workgroup-uniform)
    if (threadIdx.x == 0)
        publish(c, flat_begin, result, host_mirror, unproven);
}

// A small grid (optimize_grid's have a few thousand points, C1 2 500): both stages in ONE workgroup and one launch.
// kSmallThreads threads, every thread's loads issued four at a time (round 5: 256 threads walked their 31 values of a
// 7 776-point grid one dependent load after the other -- 12 us for 62 KB by the trace of an optimize_grid search).
constexpr int kSmallThreads = 1024;

// The values of a small grid, negated, through `take(i, -ll[i])` in ascending i per thread.
template <class Take>
__device__ __forceinline__ void small_grid_values(const double *__restrict__ ll, int64_t n, Take take)
{
    for (int64_t base = threadIdx.x; base < n; base += 4 * kSmallThreads) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)u * kSmallThreads;
            v[u] = i < n ? -ll[i] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = base + (int64_t)u * kSmallThreads;
            if (i < n)
                take(i, v[u]);
        }
    }
}

__global__ __launch_bounds__(kSmallThreads) void argmin_small(const double *__restrict__ ll, int64_t n, int64_t flat_begin,
                                                             ArgminResult *__restrict__ result, ArgminResult *__restrict__ host_mirror,
                                                             unsigned *__restrict__ queue_count, const int64_t *__restrict__ queue_index)
{
    __shared__ unsigned s_queued;
    take_queue(queue_count, &s_queued);
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    small_grid_values(ll, n, [&](int64_t i, double v) { // ascending i within a thread: strict < keeps the first
        if (v < c.v) {
            c.v = v;
            c.i = i;
        }
    });
    c = block_best(c);
    const bool unproven = queue_index ? winner_unproven(c, ll, queue_index, &s_queued) : false; // (workgroup-uniform)
    if (threadIdx.x == 0)
        publish(c, flat_begin, result, host_mirror, unproven);
}

// The selection scan of covest/grid.py:65-70 ON THE DEVICE, for the caller that runs it every iteration
// (optimize_grid): started from `start` -- the minimum the search holds when the iteration begins -- the loop
//     if val < min_val: diff += min_val - val; min_val = val; min_args = args
// changes its state exactly at the STRICT RUNNING-MINIMUM RECORDS below `start`, in index order: a handful of points
// once a search is under way.  The kernel lists them -- {flat index, -LL} -- straight into page-locked host memory, and
// the host replays the loop over that list alone (covest_amd/grid.py replay_records): same comparisons, same sums, same
// order.  Until round 5 every iteration copied the whole LL array back (62 KB for 7 776 points) to run the loop there.
// One workgroup (grids up to kArgminSmall points); the values are staged in LDS, every thread owns a contiguous run of
// them: its minimum, an exclusive prefix minimum across the threads, then its own records behind a prefix sum.  A NaN
// never passes `<`.  More than kScanCap records: `truncated`, and the caller reads the array back as before.
__global__ __launch_bounds__(kSmallThreads) void argmin_scan_small(const double *__restrict__ ll, int64_t n, int64_t flat_begin,
                                                                  double start, ArgminResult *__restrict__ result,
                                                                  ArgminResult *__restrict__ host_mirror,
                                                                  ScanRecords *__restrict__ scan, unsigned *__restrict__ queue_count)
{
    constexpr int NW = kSmallThreads / kWave;
    extern __shared__ double vals[]; // [n] -LL
    __shared__ double wave_min[NW];
    __shared__ int wave_cnt[NW];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    if (tid == 0 && queue_count)
        *queue_count = 0;
    Cand c;
    c.v = INFINITY;
    c.i = INT64_MAX;
    small_grid_values(ll, n, [&](int64_t i, double v) { // coalesced; ascending i within a thread: strict < keeps the first
        vals[i] = v;
        if (v < c.v) {
            c.v = v;
            c.i = i;
        }
    });
    c = block_best(c); // (ends with a barrier: vals is complete)
    if (tid == 0)
        publish(c, flat_begin, result, host_mirror);
    // every thread a contiguous run of the values; prefix minimum and prefix count across the threads by shuffles
    // inside a wave and a word per wave across them (two barriers in all)
    const int chunk = (int)((n + kSmallThreads - 1) / kSmallThreads);
    const int lo = min((int)n, tid * chunk), hi = min((int)n, lo + chunk);
    double m = INFINITY;
    for (int i = lo; i < hi; ++i)
        m = vals[i] < m ? vals[i] : m;
    double incl = m; // inclusive prefix minimum inside the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double o = __shfl_up(incl, off, kWave);
        if (lane >= off)
            incl = o < incl ? o : incl;
    }
    if (lane == kWave - 1)
        wave_min[w] = incl;
    __syncthreads();
    // the running minimum this thread's run starts from: `start`, the waves before, the lanes before
    double run0 = start;
    for (int k = 0; k < w; ++k)
        run0 = wave_min[k] < run0 ? wave_min[k] : run0;
    {
        const double before = __shfl_up(incl, 1, kWave);
        if (lane > 0 && before < run0)
            run0 = before;
    }
    double run = run0;
    int cnt = 0;
    for (int i = lo; i < hi; ++i)
        if (vals[i] < run) {
            run = vals[i];
            ++cnt;
        }
    int pre = cnt; // inclusive prefix count inside the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(pre, off, kWave);
        if (lane >= off)
            pre += o;
    }
    if (lane == kWave - 1)
        wave_cnt[w] = pre;
    __syncthreads();
    int at = pre - cnt, total = 0;
    for (int k = 0; k < NW; ++k) {
        if (k < w)
            at += wave_cnt[k];
        total += wave_cnt[k];
    }
    run = run0;
    for (int i = lo; i < hi; ++i)
        if (vals[i] < run) {
            run = vals[i];
            if (at < kScanCap) {
                scan->rec[at].index = flat_begin + i;
                scan->rec[at].negll = run;
            }
            ++at;
        }
    if (tid == 0) {
        scan->start = start;
        scan->truncated = total > kScanCap ? 1 : 0;
        scan->n = min(total, kScanCap);
    }
}

} // namespace

// the instantiations of this file's dispatchers, by name (the launch record, covest_compiled_variants)
const char *const kArgminVariantNames[kArgminVariants] = {"argmin_small", "argmin_stage1+2", "argmin_scan_small"};

hipError_t launch_argmin_scan(const double *ll, int64_t n, int64_t flat_begin, double start, ArgminResult *result,
                              ArgminResult *host_mirror, ScanRecords *scan, unsigned *queue_count, hipStream_t stream)
{
    if (n > kArgminSmall || n < 1)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)n * sizeof(double);
    static bool raised[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        dev = 0;
    if (!raised[dev]) { // (128 KB of dynamic LDS for the largest grid: above the default ceiling)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&argmin_scan_small),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kArgminSmall * sizeof(double)));
        if (e != hipSuccess)
            return e;
        raised[dev] = true;
    }
    record_launch(kArgminVariantNames[2]);
    hipLaunchKernelGGL(argmin_scan_small, dim3(1), dim3(kSmallThreads), lds, stream, ll, n, flat_begin, start, result, host_mirror, scan,
                       queue_count);
    return hipGetLastError();
}


hipError_t launch_argmin(const double *ll, int64_t n, int64_t flat_begin, double *partial_val, int64_t *partial_idx,
                         ArgminResult *result, ArgminResult *host_mirror, unsigned *queue_count, hipStream_t stream)
{
    return launch_argmin_proving(ll, n, flat_begin, partial_val, partial_idx, result, host_mirror, queue_count, nullptr, stream);
}

hipError_t launch_argmin_proving(const double *ll, int64_t n, int64_t flat_begin, double *partial_val, int64_t *partial_idx,
                                 ArgminResult *result, ArgminResult *host_mirror, unsigned *queue_count,
                                 const int64_t *queue_index, hipStream_t stream)
{
    if (queue_index && !queue_count)
        return hipErrorInvalidValue;
    if (n <= kArgminSmall) {
        record_launch(kArgminVariantNames[0]);
        hipLaunchKernelGGL(argmin_small, dim3(1), dim3(kSmallThreads), 0, stream, ll, n, flat_begin, result, host_mirror, queue_count,
                           queue_index);
        return hipGetLastError();
    }
    // (a small grid needs no more workgroups than it has waves of points)
    const int blocks = (int)std::min<int64_t>(kArgminBlocks, std::max<int64_t>(1, (n + 255) / 256));
    // (measured and not kept, round 4: both stages in ONE launch -- every workgroup stores its candidate, adds to a
    // counter behind a fence, the workgroup whose add came last reduces the candidates -- is 20-27 us SLOWER a step than
    // the second launch it saves: 1 024 agent-scope fences cost more than a 4 us launch)
    record_launch(kArgminVariantNames[1]);
    hipLaunchKernelGGL(argmin_stage1, dim3(blocks), dim3(256), 0, stream, ll, n, partial_val, partial_idx);
    hipLaunchKernelGGL(argmin_stage2, dim3(1), dim3(queue_index ? 1024 : 256), 0, stream, ll, queue_index, partial_val, partial_idx,
                       blocks, flat_begin, result, host_mirror, queue_count);
    return hipGetLastError();
}

} // namespace covest
