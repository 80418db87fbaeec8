// factored_diag.h -- K-factored's in-kernel stamps (ll_factored.hip): where a wave's cycles go.  DIAGNOSTIC builds only
// (-DCOVEST_DIAG, tiles.h FactoredPlan::diag): in the shipped library Stamps is empty and every member an empty inline
// function, so the stages call it without an #ifdef and pay nothing.  Eight words per wave go to plan.diag
// ([workgroup][wave][8]: tools/factored_diag.py and tools/factored_diag_walk.py read them), by COVEST_FACTORED_DIAG:
//   1     the laps of the walk, in the order of Lap: cycles in build / contract / log / barrier, ...
//   2, 3  the wait at the barrier by eighths of the walk (3: the first seven intervals one by one)
//   4     where a workgroup's time OUTSIDE the walk goes: the stages' ends, see dump_stages
#pragma once
#include <hip/hip_runtime.h>

#include "tiles.h"

namespace covest {

struct StampNames {
    // a wave's laps (COVEST_FACTORED_DIAG=1), the words in this order
    enum Lap {
        kBuild,    // phase A
        kContract, // phase B, the shared steps included
        kLog,      // phase C
        kWait,     // the barrier
        kShared,   // of phase B: the first MFMAs and the shared steps
        kZero,     // (a count) key tiles whose G columns of this (builder) wave were all zero; times 2^20: items it skipped
        kEnter,    // of phase A: StreamSet::enter_tile
        kFirst,    // of phase B: waiting for the first A fragments (LDS) and the tile's weights (HBM / L2)
    };
    // the stages outside the walk (COVEST_FACTORED_DIAG=4), stamped at their ends
    enum Stage {
        kStart,     // the kernel's first instruction
        kFetched,   // the table, the point, the classes' rates, the items' constants; the first barrier
        kStreams,   // the streams' constants (builder waves)
        kUnits,     // the units' tables and first weights
        kWalked,    // the walk
    };
};

#ifdef COVEST_DIAG
struct Stamps : StampNames {
    long long *out;  // this wave's eight words (nullptr: no stamps asked for)
    int mode;        // plan.skip_phases: its bits 16 .. 18 choose what the words are
    long long t0 = 0, lap_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, at[5] = {0, 0, 0, 0, 0};
    __device__ Stamps(const FactoredPlan &plan, int waves, int wave)
        : out(plan.diag ? plan.diag + ((int64_t)(blockIdx.x * gridDim.y + blockIdx.y) * waves + wave) * 8 : nullptr),
          mode(plan.skip_phases)
    {
        stage(kStart);
    }
    __device__ void stage(Stage s) { at[s] = (long long)clock64(); }
    __device__ void walk_begins()
    {
        if (out)
            t0 = (long long)clock64();
    }
    __device__ void lap(Lap which)
    {
        if (out) {
            const long long now = (long long)clock64();
            lap_sum[which] += now - t0;
            t0 = now;
        }
    }
    __device__ void count_zero_tile()
    {
        if (out)
            lap_sum[kZero] += 1;
    }
    // (items a builder wave skipped by the column limit, factored_build.h: counted in the same word, from bit 20 up)
    __device__ void count_skipped_item()
    {
        if (out)
            lap_sum[kZero] += 1ll << 20;
    }
    // until the first fragments and the weights are there
    template <int MU>
    __device__ void first_fragments(const double (&a0)[MU], const double (&wfirst)[MU])
    {
        if (out) {
            double sink = 0.0;
#pragma unroll
            for (int k = 0; k < MU; ++k)
                sink += a0[k] + wfirst[k];
            asm volatile("" ::"v"(sink));
            lap(kFirst);
        }
    }
    // behind an interval's barrier: (modes 2 and 3) the wait by eighths of the walk, and the lap
    __device__ void barrier_passed(int p, int t_begin, int t_end, int lane)
    {
        if (out && (mode & 0x10000)) {
            const long long now = (long long)clock64();
            if (lane == 0) {
                const int grp = (mode & 0x20000) ? min(7, p - t_begin + 1) // (=3: the first seven intervals one by one)
                                                 : min(7, (p - t_begin + 1) * 8 / (t_end - t_begin + 1));
                out[grp] += now - t0;
            }
        }
        lap(kWait);
    }
    __device__ void dump_laps(int lane)
    {
        stage(kWalked);
        if (out && lane == 0 && !(mode & 0x50000))
            for (int i = 0; i < 8; ++i)
                out[i] = lap_sum[i];
    }
    __device__ void dump_stages(int lane)
    {
        if (out && (mode & 0x40000) && lane == 0) {
            const long long end = (long long)clock64();
            for (int s = 0; s < 4; ++s)
                out[s] = at[s + 1] - at[s];
            out[4] = end - at[kWalked];
            out[5] = end - at[kStart];
            out[6] = at[kStart]; // (absolute: a workgroup's start against the others')
            out[7] = end;
        }
    }
};
#else
struct Stamps : StampNames {
    __device__ Stamps(const FactoredPlan &, int, int) {}
    __device__ void stage(Stage) {}
    __device__ void walk_begins() {}
    __device__ void lap(Lap) {}
    __device__ void count_zero_tile() {}
    __device__ void count_skipped_item() {}
    template <int MU>
    __device__ void first_fragments(const double (&)[MU], const double (&)[MU])
    {
    }
    __device__ void barrier_passed(int, int, int, int) {}
    __device__ void dump_laps(int) {}
    __device__ void dump_stages(int) {}
};
#endif

} // namespace covest
