// gather_reads.h -- the gather of a table of reads through the tile image: what gather_reads.hip offers the sampler
// (sample_reads.hip) and the split (split_reads.hip), whose last launch and hot path it is (DESIGN.md sections 6m, 6aa).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace covest {

constexpr int kGatherGroups = 2048;  // workgroups that share the gather's tiles: eight on each of 256 CUs

// For any table of reads to gather: rank q of the counts[0] reads (device: counts[2] = (reads, bases in all)) goes from
// bases + src_off[q] to out_bases + out_offsets[q], the output offsets ascending from 0 (nullptr: q * read_len,
// read_len > 0).  most_bases: an upper bound of counts[1] the host knows (> 0), or -1.  Any alignment of both buffers;
// one launch on `stream`; nothing is written outside out_bases[0 .. counts[1]).
hipError_t launch_gather_reads(const unsigned char *bases, const int64_t *counts, const int64_t *out_offsets,
                               int64_t read_len, int64_t most_bases, const int64_t *src_off, unsigned char *out_bases,
                               hipStream_t stream);

} // namespace covest
