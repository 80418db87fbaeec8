"""Take the duplicate reads out of a read set, on the device: the first copy of every read is kept, in input order
(DESIGN.md section 6al).

    reads = simulate_reads(genome, 100, coverage=10, error_rate=0.01, seed=1)
    unique = dedup_reads(reads)
    counts = unique.add_to(KmerCounts(21, canonical=True))
    unique.copies_histogram()      # {1: ..., 2: ...}: kept reads by the number of their copies

    python -m covest_amd.dedup SRC DEST [--reverse-complement]

Two reads are equal if they have the same length and the same bytes; with `reverse_complement` also if one is the reverse
complement of the other (a <-> t, c <-> g in either case, every other byte its own complement; case is not folded).
Candidates are found by a 63-bit fingerprint of the whole read and dropped only after their bytes have been compared
(include/covest_amd.h states the fingerprint and the rule).  One call looks at ONE resident read set: copies in
different batches of a streamed file are not seen.  There is no CPU path: without the library or a HIP device every call
raises CovestHipError.
"""
import ctypes

import numpy as np

from . import _capi
from .kmer_hist import NS_IGNORE, ReadBatches
from .sample import _packed, _write_records
from .simulate import _check_first_read, _check_seed

FP_BITS = 63       # the fingerprint's bits; fewer only make more reads collide (the tests' way into that route)
MAX_ROUNDS = 4     # of dedup_reads: a round more for as long as reads were kept as collided


def _check(seed, first_read, fp_bits=FP_BITS):
    """The argument rules of covest_dedup_reads, before the library is asked (ValueError, as sample.py's)."""
    _check_seed(seed, whole=True)
    first_read = _check_first_read(first_read)
    if isinstance(fp_bits, bool) or int(fp_bits) != fp_bits or not 1 <= fp_bits <= 63:
        raise ValueError("fp_bits must be within 1 .. 63")
    return int(seed), first_read, int(fp_bits)


class DedupReads:
    """What dedup_reads returns: `bases` (the kept reads: (n_kept, L) for reads of one length, else back to back),
    `offsets` (n_kept + 1,) int64, `kept` (n_kept,) int64 global indices, `copies` (n_kept,) int32: 1 + the reads
    dropped onto each kept read; `n_input`, `collided` (reads the first round kept beside a fingerprint collision: the
    later rounds took their copies out), `rounds`, `reverse_complement`, `seed`; for a SimulatedReads input also
    `positions` and `forward` of the kept rows (else None)."""

    def __init__(self, bases, offsets, kept, copies, n_input, collided, rounds, reverse_complement, seed, source=None,
                 first_read=0):
        self.bases = bases
        self.offsets = offsets
        self.kept = kept
        self.copies = copies
        self.n_input = int(n_input)
        self.collided = int(collided)
        self.rounds = int(rounds)
        self.reverse_complement = bool(reverse_complement)
        self.seed = int(seed)
        self.positions = self.forward = None
        if source is not None:
            rows = kept - int(first_read)
            self.positions = source.positions[rows]
            self.forward = source.forward[rows]

    @property
    def n_reads(self):
        return int(self.kept.size)

    @property
    def n_bases(self):
        return int(self.offsets[-1])

    @property
    def duplicate_share(self):
        """The share of the input's reads that were dropped."""
        return (self.n_input - self.n_reads) / self.n_input if self.n_input else 0.0

    def copies_histogram(self):
        """{c: kept reads with c copies (themselves included)}, ascending in c."""
        values, counts = np.unique(self.copies, return_counts=True)
        return {int(v): int(c) for v, c in zip(values, counts)}

    def add_to(self, counts):
        """Count the kept reads' k-mers into a KmerCounts (kmer_hist.py); returns it."""
        if self.n_reads:
            blob = np.ascontiguousarray(self.bases).reshape(-1)
            counts.add_packed(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                              self.offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), self.n_reads, self.n_bases)
        return counts

    def write_fasta(self, path):
        """'>read_{global index}' and the read, a record a kept read."""
        with open(path, "w") as f:
            _write_records(f, np.ascontiguousarray(self.bases).reshape(-1), self.offsets, self.kept)


def _dedup_host(blob, offsets, n, read_len, first_read, reverse_complement, fp_bits, seed, device):
    """covest_dedup_reads on host arrays, one round: (out_bases, out_offsets, kept, copies, collided)."""
    total = int(offsets[-1]) if offsets is not None else n * read_len
    out = np.empty(total, dtype=np.uint8)
    out_offsets = np.empty(n + 1, dtype=np.int64)
    kept = np.empty(n, dtype=np.int64)
    copies = np.empty(n, dtype=np.int32)
    n_kept, n_bases, n_collided = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _capi.check(_capi.lib().covest_dedup_reads(
        int(device), blob.ctypes.data, offsets.ctypes.data if offsets is not None else None, n, int(read_len), first_read,
        1 if reverse_complement else 0, fp_bits, seed, out.ctypes.data, out_offsets.ctypes.data, kept.ctypes.data,
        copies.ctypes.data, ctypes.byref(n_kept), ctypes.byref(n_bases), ctypes.byref(n_collided)), "covest_dedup_reads")
    return out[:n_bases.value], out_offsets[:n_kept.value + 1], kept[:n_kept.value], copies[:n_kept.value], n_collided.value


def _dedup_rounds(blob, offsets, n, read_len, reverse_complement, fp_bits, seed, device):
    """Rounds of the call on its own output, the seed one higher each time, until no read was kept as collided:
    (out_bases, out_offsets, rows kept: indices into the input, copies, collided of round 1, rounds)."""
    rows = np.arange(n, dtype=np.int64)
    copies = None
    first_collided = None
    for rnd in range(MAX_ROUNDS):
        blob, out_offsets, kept, c, collided = _dedup_host(blob, offsets, rows.size, read_len, 0, reverse_complement, fp_bits,
                                                           (seed + rnd) & 0xFFFFFFFFFFFFFFFF, device)
        # A read that a later round drops is equal to an earlier read e that every round so far has held, so it was
        # never the first of its key and no read was ever dropped ONTO it: it stands for itself alone, and the round's
        # count of the reads dropped onto each kept read is what that read's copies grow by.
        copies = c.astype(np.int64) if rnd == 0 else copies[kept] + (c - 1)
        rows = rows[kept]
        offsets = out_offsets if offsets is not None else None
        if first_collided is None:
            first_collided = collided
        if collided == 0:
            return blob, out_offsets, rows, copies, first_collided, rnd + 1
    raise _capi.CovestHipError("dedup_reads: reads still collide after %d rounds" % MAX_ROUNDS)


def dedup_reads(reads, reverse_complement=False, seed=0, first_read=None, device=-1):
    """The reads of `reads` -- a SimulatedReads, an (n, L) uint8 array or a pair (bases, offsets) in the packed layout --
    without their duplicates: exactly one read of every class of equal reads, the first of each, in input order, as a
    DedupReads.  Reads are numbered from `first_read` (default: a SimulatedReads' own first_read, else 0)."""
    blob, offsets, n, read_len, source = _packed(reads)
    if first_read is None:
        first_read = source.first_read if source is not None else 0
    seed, first_read, _ = _check(seed, first_read)
    out, out_offsets, rows, copies, collided, rounds = _dedup_rounds(blob, offsets, n, read_len, reverse_complement, FP_BITS,
                                                                     seed, device)
    if offsets is None:
        out = out.reshape(rows.size, read_len)
    return DedupReads(out, out_offsets, rows + first_read, copies.astype(np.int32), n, collided, rounds, reverse_complement,
                      seed, source, first_read)


def dedup_reads_device(bases_ptr, n_reads, out_bases_ptr, counts_ptr, reverse_complement=False, seed=0, first_read=0,
                       read_len=0, offsets_ptr=None, out_offsets_ptr=None, kept_ptr=None, copies_ptr=None, fp_bits=FP_BITS,
                       stream=None, device=-1):
    """One round between buffers resident in HBM (raw device pointers, e.g. a torch tensor's data_ptr()), asynchronous on
    `stream`: `n_reads` reads at `bases_ptr`, `read_len` bases each unless `offsets_ptr` (n_reads + 1 int64) is given;
    the kept ones to `out_bases_ptr` / `out_offsets_ptr` (n_kept + 1 int64; needed with `offsets_ptr`) / `kept_ptr`
    (n_kept int64, optional) / `copies_ptr` (n_kept int32, optional), all sized for the input; (reads kept, bases kept,
    reads kept as collided) to the three int64 at `counts_ptr`.  Where the third is not 0, duplicates may have survived
    beside the collisions: run the call again on its output with another seed."""
    seed, first_read, fp_bits = _check(seed, first_read, fp_bits)
    if n_reads < 0:
        raise ValueError("n_reads must not be negative")
    if not offsets_ptr and read_len < 0:
        raise ValueError("read_len must not be negative")
    if offsets_ptr and not out_offsets_ptr:
        raise ValueError("reads of their own lengths need out_offsets_ptr")
    if not counts_ptr:
        raise ValueError("counts_ptr must not be null")
    _capi.require_shared_runtime("dedup_reads_device")
    _capi.check(_capi.lib().covest_dedup_reads_device(
        int(device), ctypes.c_void_p(bases_ptr), ctypes.c_void_p(offsets_ptr or 0), int(n_reads), int(read_len), first_read,
        1 if reverse_complement else 0, fp_bits, seed, ctypes.c_void_p(out_bases_ptr), ctypes.c_void_p(out_offsets_ptr or 0),
        ctypes.c_void_p(kept_ptr or 0), ctypes.c_void_p(copies_ptr or 0), ctypes.c_void_p(counts_ptr),
        ctypes.c_void_p(stream or 0)), "covest_dedup_reads_device")


def read_file(src, n_strategy=NS_IGNORE):
    """The reads of `src` (FASTA or FASTQ) through the library's reader, whole, as one resident set: (bases, offsets)."""
    blobs, lens = [], []
    for bases, offsets, n, n_bases in ReadBatches(src, n_strategy):
        blobs.append(np.ctypeslib.as_array(bases, shape=(max(n_bases, 1),))[:n_bases].copy())
        lens.append(np.diff(np.ctypeslib.as_array(offsets, shape=(n + 1,))))
    offsets = np.zeros(sum(a.size for a in lens) + 1, dtype=np.int64)
    if lens:
        np.cumsum(np.concatenate(lens), out=offsets[1:])
    return (np.concatenate(blobs) if blobs else np.zeros(0, dtype=np.uint8)), offsets


def dedup_reads_file(src, dest, reverse_complement=False, seed=0, n_strategy=NS_IGNORE, device=-1):
    """The reads of `src` without their duplicates, written to `dest` as FASTA ('read_{index}': the reader keeps no
    ids; the sequences as the reader preprocesses them).  The file is read whole: the comparison needs the first copy
    resident.  Returns the DedupReads."""
    unique = dedup_reads(read_file(src, n_strategy), reverse_complement=reverse_complement, seed=seed, device=device)
    unique.write_fasta(dest)
    return unique


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Write the reads of SRC without their duplicates to DEST (FASTA): the first "
                                             "copy of every read, in input order.")
    ap.add_argument("src")
    ap.add_argument("dest")
    ap.add_argument("--reverse-complement", action="store_true",
                    help="a read and its reverse complement are copies of one another")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    unique = dedup_reads_file(args.src, args.dest, reverse_complement=args.reverse_complement, seed=args.seed)
    print("%d reads kept, %d dropped, at most %d copies of one read"
          % (unique.n_reads, unique.n_input - unique.n_reads, int(unique.copies.max()) if unique.n_reads else 0))


if __name__ == "__main__":
    main()
