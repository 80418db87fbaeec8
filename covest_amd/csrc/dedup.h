// dedup.h -- duplicate reads removed, the first copy kept: what dedup_reads.hip offers abi_dedup.cpp
// (covest_dedup_reads*).  The fingerprint and the table's size: read_fingerprint.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace covest {

constexpr int kDedupShare = 256;           // reads a workgroup of the flag and place kernels owns, one a lane
constexpr int kDedupMaxProbe = 1 << 16;    // slots an insert looks at before it gives up (the read is then kept)

// bytes of device scratch launch_dedup_reads needs for n_reads reads: the table (16 bytes a slot, a power of two of them,
// at least 2 * n_reads), and per read a fingerprint (later its flag), a count of the reads dropped onto it and a source
// offset; a (count, bases) pair per kDedupShare reads
size_t dedup_scratch_bytes(int64_t n_reads);
// Of bases / offsets[n_reads + 1] (nullptr: every read read_len bases), in input order, the reads that are no copy of an
// earlier one -- read r is kept iff the lowest read index m with r's fingerprint key is r itself, or read m is not equal
// to read r (a collision: counted), or r's insert ran out of probes (counted alike) -- to out_bases / out_offsets[n_kept +
// 1] (may be nullptr where offsets is) / kept_index[n_kept] (first_read + index; or nullptr) / copies[n_kept] (1 + the
// reads dropped onto the read; or nullptr); counts[3] = (reads kept, bases kept, reads kept as collided).  Equality: the
// same length and bytes, with reverse_complement also the reverse complement's.  Any alignment of bases and out_bases;
// three memsets and the launches (the last: gather_reads.h) on `stream`, no workgroup waits for another; nothing is
// written outside the stated ranges and `scratch`, which has to stay until the last launch has run.
hipError_t launch_dedup_reads(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                              int64_t first_read, int reverse_complement, int fp_bits, uint64_t seed,
                              unsigned char *out_bases, int64_t *out_offsets, int64_t *kept_index, int32_t *copies,
                              int64_t *counts, void *scratch, hipStream_t stream);

} // namespace covest
