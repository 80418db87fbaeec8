// split.h -- K-split: what split_reads.hip offers abi_split.cpp (covest_split_reads*).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace covest {

constexpr int kSplitMaxGroups = 256;
constexpr int kSplitThreads = 256;
constexpr int kSplitPerLane = 4;                             // reads a lane of the flag and place kernels takes
constexpr int kSplitShare = kSplitThreads * kSplitPerLane;   // reads a workgroup of those kernels owns
constexpr int kSplitScanThreads = 256;
constexpr int kSplitScanPerLane = 4;
constexpr int kSplitScanPass = kSplitScanThreads * kSplitScanPerLane; // pairs of a group's row one pass of its scan holds
static_assert(kSplitShare >= kSplitMaxGroups, "a (count, bases) pair a group and workgroup: 16 bytes a read at the most");

// bytes of device scratch launch_split_reads needs: a (count, bases) pair per group and kSplitShare reads, a pair per
// group, the two totals, and a source offset per read -- 16 * groups / kSplitShare + 8 <= 12 bytes a read, and a
// constant of 16 * (2 * groups + 1) at the most
size_t split_scratch_bytes(int64_t n_reads, int groups);
// The reads of bases / offsets[n_reads + 1] (nullptr: every read read_len bases) in the order of their groups, input
// order within a group, to out_bases / out_offsets[n_reads + 1] (may be nullptr where offsets is) / read_index[n_reads]
// (or nullptr); group_first[groups + 1] = the rank at which each group starts.  Read q is of group (w * groups) >> 32,
// w = word 0 of Philox block (lo32(r), hi32(r), 0, 8), r = first_read + q, key = seed.  n_reads > 0, groups in 1 ..
// kSplitMaxGroups.  Any alignment of bases and out_bases; launches on `stream`, no workgroup waits for another; nothing
// is written outside the stated ranges and `scratch`, which has to stay until the last launch has run.
hipError_t launch_split_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                              int64_t first_read, int groups, uint64_t seed, unsigned char *out_bases,
                              int64_t *out_offsets, int64_t *read_index, int64_t *group_first, void *scratch,
                              hipStream_t stream);

} // namespace covest
