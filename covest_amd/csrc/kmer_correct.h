// kmer_correct.h -- isolated substitutions of reads corrected from the k-mer table (k <= 31, kmer_table.h), read-only on
// the table like kmer_lookup.h.  The rule, per read, last = len - k:
//
//   1. A window s is WEAK when table_find of its key (window_codes + canonical_pair, as in the lookup) is below
//      `cutoff` (the table's 64-bit count; cutoff 0: nothing is weak).  A read shorter than k has no window: its bytes
//      are copied, its row is {0, 0, 0, 0}.
//   2. A RUN is a maximal set of consecutive weak windows [f, l].  Runs are judged independently, each against the
//      ORIGINAL bytes.  Sound because a candidate position of a run lies in that run's windows only (its covering
//      windows are exactly [f, l], 3.), and the windows of two different runs share no candidate position (a shared
//      base would have both runs as its covering windows).  So a correction of one run changes no window of another
//      run: corrections neither see nor disturb one another, whatever their order.
//   3. The CANDIDATE POSITIONS of a run are the bases p whose covering windows [max(0, p - k + 1), min(p, last)] are
//      exactly [f, l]: none if l - f + 1 > k; if f > 0, p = f + k - 1, and only when l == min(p, last); if f == 0 and
//      l < last, p = l; if f == 0 and l == last, every p in [last, min(k - 1, len - 1)].
//   4. An ALTERNATIVE (p, b) is a candidate position and one of the three bases other than the read's own at p; it is
//      VALID when every window of [f, l], with base p replaced by b, has a count >= cutoff.
//   5. Exactly one valid alternative: the run is CORRECTED, byte p of the output is "ACGT"[b] | (old byte & 0x20) (a
//      lower-case read stays lower-case).  More than one: AMBIGUOUS.  None -- runs longer than k and runs without a
//      candidate position among them --: UNFIXABLE.  In the last two cases the bytes stay.
//
// Outputs:
//   out  uint8, indexed like the bases (offsets[r] + i; reads of one length: r * read_len + i): the input except at
//        corrected positions.  EVERY BYTE IS STORED EXACTLY ONCE, by the lane that copies it: a correction is a
//        wave-uniform (position, base) pair that is handed to that lane before it copies the byte (kmer_correct.hip),
//        so no store of one lane is overwritten by another.  `out` may be the very pointer `bases` (in place): then only
//        the corrected bytes are stored, and a byte is stored only after every window that holds it has been read (the
//        copy of bytes 64(c - 1) .. 64c - 1 follows the walk of windows 64c .. 64c + 63), so also in place every run is
//        judged against the original bytes.  Otherwise `out` must not overlap `bases`.
//   fix  uint32[n_reads][4] = {runs, corrected, ambiguous, unfixable}, one 16-byte store by lane 0 (optional: null),
//        runs = corrected + ambiguous + unfixable.
//
// Only isolated substitutions: two errors closer than k + 1 merge into one run longer than k and stay.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace covest {

// Asynchronous on `stream`; the launches are the visits of kmer_plan::for_each_wave_launch, `out` advanced as `bases` is.
hipError_t launch_kmer_correct(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                               int canonical, const KmerTable &t, uint32_t cutoff, unsigned char *out, uint32_t *fix,
                               hipStream_t stream);

} // namespace covest
