// sample.h -- K-sample: what sample_reads.hip offers abi_sample.cpp (covest_sample_reads*; the reference's
// covest/data.py:57-63).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace covest {

constexpr int kSampleShare = 256;          // reads a workgroup of the flag and place kernels owns, one a lane
constexpr int kSampleGatherGroups = 2048;  // workgroups that share the gather's tiles: eight on each of 256 CUs

// bytes of device scratch launch_sample_reads needs for n_reads reads: a (count, bases) pair per kSampleShare reads and
// a source offset per read (the upper bound of the reads kept)
size_t sample_scratch_bytes(int64_t n_reads);
// The kept reads of bases / offsets[n_reads + 1] (nullptr: every read read_len bases), in input order, to out_bases /
// out_offsets[n_kept + 1] (may be nullptr where offsets is) / kept_index[n_kept] (or nullptr); counts[2] = (reads kept,
// bases kept).  Read q is kept iff word 0 of Philox block (lo32(r), hi32(r), 0, 2), r = first_read + q, key = seed, is
// below thr.  Any alignment of bases and out_bases; four launches on `stream`, no workgroup waits for another; nothing
// is written outside the stated ranges and `scratch`, which has to stay until the last launch has run.
hipError_t launch_sample_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                               int64_t first_read, uint64_t thr, uint64_t seed, unsigned char *out_bases,
                               int64_t *out_offsets, int64_t *kept_index, int64_t *counts, void *scratch,
                               hipStream_t stream);
// The sampler's last launch on its own, for any table of reads to gather (split_reads.hip): rank q of the
// counts[0] reads (device: counts[2] = (reads, bases in all)) goes from bases + src_off[q] to out_bases +
// out_offsets[q], the output offsets ascending from 0 (nullptr: q * read_len, read_len > 0).  most_bases: an upper
// bound of counts[1] the host knows (> 0), or -1.  Any alignment of both buffers; nothing is written outside
// out_bases[0 .. counts[1]).
hipError_t launch_sample_gather(const unsigned char *bases, const int64_t *counts, const int64_t *out_offsets,
                                int64_t read_len, int64_t most_bases, const int64_t *src_off, unsigned char *out_bases,
                                hipStream_t stream);

} // namespace covest
