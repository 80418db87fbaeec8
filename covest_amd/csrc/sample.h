// sample.h -- K-sample: what sample_reads.hip offers abi_sample.cpp (covest_sample_reads*; the reference's
// covest/data.py:57-63).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace covest {

constexpr int kSampleShare = 256;          // reads a workgroup of the flag and place kernels owns, one a lane

// bytes of device scratch launch_sample_reads needs for n_reads reads: a (count, bases) pair per kSampleShare reads and
// a source offset per read (the upper bound of the reads kept)
size_t sample_scratch_bytes(int64_t n_reads);
// The kept reads of bases / offsets[n_reads + 1] (nullptr: every read read_len bases), in input order, to out_bases /
// out_offsets[n_kept + 1] (may be nullptr where offsets is) / kept_index[n_kept] (or nullptr); counts[2] = (reads kept,
// bases kept).  Read q is kept iff word 0 of Philox block (lo32(r), hi32(r), 0, 2), r = first_read + q, key = seed, is
// below thr.  Any alignment of bases and out_bases; four launches on `stream` (the last: gather_reads.h), no workgroup
// waits for another; nothing is written outside the stated ranges and `scratch`, which has to stay until the last
// launch has run.
hipError_t launch_sample_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                               int64_t first_read, uint64_t thr, uint64_t seed, unsigned char *out_bases,
                               int64_t *out_offsets, int64_t *kept_index, int64_t *counts, void *scratch,
                               hipStream_t stream);

} // namespace covest
