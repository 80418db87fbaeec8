"""Lower the coverage of a read set by a known factor, on the device: the counterpart of the reference's
covest/data.py:57-63 (`sample_reads`) and bin/read_sampler.py.

    reads = simulate_reads(genome, 100, coverage=40, error_rate=0.02, seed=1)
    half = sample_reads(reads, 2, seed=1)
    counts = half.add_to(KmerCounts(21, canonical=True))

    python -m covest_amd.sample SRC DEST -f FACTOR [--seed S]

Every read is kept with probability 1 / factor, and the kept reads come out in input order in the packed layout the
k-mer counter takes.  Where the reference draws from Python's unseeded `random`, read r (its index + `first_read`) is
kept iff word 0 of Philox4x32-10 on the counter (lo32(r), hi32(r), 0, 2), key = seed, is below
floor((1 / factor) * 2^32) (include/covest_amd.h): a run is reproducible, and a chunk sampled with `first_read` set keeps
what the whole run keeps among its rows.  There is no CPU path: without the library or a HIP device every call raises
CovestHipError.
"""
import ctypes
import math

import numpy as np

from . import _capi
from .kmer_hist import NS_IGNORE, KmerCounts, ReadBatches, _bases_and_offsets
from .simulate import SimulatedReads, _check_first_read, _check_seed


def _check(factor, seed, first_read):
    """The argument rules of covest_sample_reads, before the library is asked (ValueError, as simulate.py's)."""
    try:
        factor = float(factor)
    except (TypeError, ValueError):
        raise ValueError("factor must be a number")
    if not (factor >= 1.0) or not math.isfinite(factor):  # (NaN fails the first)
        raise ValueError("factor must be a finite number, at least 1")
    _check_seed(seed, whole=True)
    return factor, int(seed), _check_first_read(first_read)


def threshold(factor):
    """floor((1 / factor) * 2^32): a read is kept iff its word is below it."""
    return int(math.floor((1.0 / float(factor)) * 4294967296.0))


def _packed(reads):
    """(blob, offsets or None, n_reads, read_len, the SimulatedReads or None) of what sample_reads takes."""
    if isinstance(reads, SimulatedReads):
        n, L = reads.bases.shape
        return np.ascontiguousarray(reads.bases).reshape(-1), None, n, L, reads
    if isinstance(reads, tuple) and len(reads) == 2:
        bases, offsets = _bases_and_offsets(*reads)
        return bases, offsets, offsets.size - 1, 0, None
    a = np.asarray(reads)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("reads must be a SimulatedReads, an (n, L) uint8 array or a pair (bases, offsets)")
    return np.ascontiguousarray(a).reshape(-1), None, a.shape[0], a.shape[1], None


class SampledReads:
    """What sample_reads returns: `bases` (the kept reads: (n_kept, L) for reads of one length, else back to back),
    `offsets` (n_kept + 1,) int64, `kept` (n_kept,) int64 global indices, `factor`, `seed`; for a SimulatedReads input
    also `positions` and `forward` of the kept rows (else None)."""

    def __init__(self, bases, offsets, kept, factor, seed, source=None, first_read=0):
        self.bases = bases
        self.offsets = offsets
        self.kept = kept
        self.factor = float(factor)
        self.seed = int(seed)
        self.positions = self.forward = None
        self._source = source
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

    def simulated(self):
        """The sample of a SimulatedReads input as a SimulatedReads of the kept rows (error_free, substitutions)."""
        if self._source is None:
            raise ValueError("the sampled reads were not simulated: their origin is not known")
        s = self._source
        return SimulatedReads(self.bases, self.positions << 1 | self.forward.astype(np.int64), s.genome_len, s.error_rate,
                              s.seed, s.first_read)

    def error_free(self, genome):
        return self.simulated().error_free(genome)

    def substitutions(self, genome):
        return self.simulated().substitutions(genome)

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


def _write_records(f, blob, offsets, kept):
    text = blob.tobytes().decode("ascii")
    for i in range(kept.size):
        f.write(">read_%d\n%s\n" % (kept[i], text[offsets[i]:offsets[i + 1]]))


def _sample_host(blob, offsets, n, read_len, first_read, factor, seed, device):
    """covest_sample_reads on host arrays: (out_bases, out_offsets, kept)."""
    total = int(offsets[-1]) if offsets is not None else n * read_len
    out = np.empty(total, dtype=np.uint8)
    out_offsets = np.empty(n + 1, dtype=np.int64)
    kept = np.empty(n, dtype=np.int64)
    n_kept, n_bases = ctypes.c_int64(), ctypes.c_int64()
    _capi.check(_capi.lib().covest_sample_reads(
        int(device), blob.ctypes.data, offsets.ctypes.data if offsets is not None else None, n, int(read_len),
        first_read, factor, seed, out.ctypes.data, out_offsets.ctypes.data, kept.ctypes.data, ctypes.byref(n_kept),
        ctypes.byref(n_bases)), "covest_sample_reads")
    return out[:n_bases.value], out_offsets[:n_kept.value + 1], kept[:n_kept.value]


def sample_reads(reads, factor, seed=0, first_read=None, device=-1):
    """Keep every read of `reads` -- a SimulatedReads, an (n, L) uint8 array or a pair (bases, offsets) in the packed
    layout -- with probability 1 / factor; the kept reads in input order, as a SampledReads.  Reads are numbered from
    `first_read` (default: a SimulatedReads' own first_read, else 0)."""
    blob, offsets, n, read_len, source = _packed(reads)
    if first_read is None:
        first_read = source.first_read if source is not None else 0
    factor, seed, first_read = _check(factor, seed, first_read)
    out, out_offsets, kept = _sample_host(blob, offsets, n, read_len, first_read, factor, seed, device)
    if offsets is None:
        out = out.reshape(kept.size, read_len)
    return SampledReads(out, out_offsets, kept, factor, seed, source, first_read)


def sample_reads_device(bases_ptr, n_reads, out_bases_ptr, counts_ptr, factor, seed=0, first_read=0, read_len=0,
                        offsets_ptr=None, out_offsets_ptr=None, kept_ptr=None, stream=None, device=-1):
    """The same between buffers resident in HBM (raw device pointers, e.g. a torch tensor's data_ptr()), asynchronous on
    `stream`: `n_reads` reads at `bases_ptr`, `read_len` bases each unless `offsets_ptr` (n_reads + 1 int64) is given;
    the kept ones to `out_bases_ptr` / `out_offsets_ptr` (n_kept + 1 int64; needed with `offsets_ptr`) / `kept_ptr`
    (n_kept int64, optional), all sized for the input; (reads kept, bases kept) to the two int64 at `counts_ptr`."""
    factor, seed, first_read = _check(factor, seed, first_read)
    if n_reads < 0:
        raise ValueError("n_reads must not be negative")
    if not offsets_ptr and read_len < 0:
        raise ValueError("read_len must not be negative")
    if offsets_ptr and not out_offsets_ptr:
        raise ValueError("reads of their own lengths need out_offsets_ptr")
    if not counts_ptr:
        raise ValueError("counts_ptr must not be null")
    _capi.require_shared_runtime("sample_reads_device")
    _capi.check(_capi.lib().covest_sample_reads_device(
        int(device), ctypes.c_void_p(bases_ptr), ctypes.c_void_p(offsets_ptr or 0), int(n_reads), int(read_len), first_read,
        factor, seed, ctypes.c_void_p(out_bases_ptr), ctypes.c_void_p(out_offsets_ptr or 0), ctypes.c_void_p(kept_ptr or 0),
        ctypes.c_void_p(counts_ptr), ctypes.c_void_p(stream or 0)), "covest_sample_reads_device")


# the split's constants (csrc/split.h; tests/test_split_cpu.py compares): the cap on the groups, the reads a workgroup of
# the flag and place kernels owns, and the pairs of a group's row one pass of its scan holds
MAX_GROUPS = 256
SPLIT_SHARE = 1024
SPLIT_SCAN_PASS = 1024


def _check_split(groups, seed, first_read):
    """The argument rules of covest_split_reads, before the library is asked (ValueError)."""
    if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)):
        raise ValueError("groups must be an integer")
    if not 1 <= groups <= MAX_GROUPS:
        raise ValueError("groups must be within 1 .. %d" % MAX_GROUPS)
    _check_seed(seed, whole=True)
    return int(groups), int(seed), _check_first_read(first_read)


class SplitReads:
    """What split_reads returns: the reads in the order of their groups, input order within a group.  `bases` ((n, L)
    for reads of one length, else back to back), `offsets` (n + 1,) int64, `read_index` (n,) int64: the global index of
    the read at each output rank, `group_first` (groups + 1,) int64: the rank at which each group starts; `groups`,
    `seed`."""

    def __init__(self, bases, offsets, read_index, group_first, seed):
        self.bases = bases
        self.offsets = offsets
        self.read_index = read_index
        self.group_first = group_first
        self.groups = int(group_first.size - 1)
        self.seed = int(seed)

    @property
    def n_reads(self):
        return int(self.read_index.size)

    def group(self, g):
        """The reads of group g: rows of `bases` for reads of one length, else (bases, offsets from 0)."""
        if not 0 <= g < self.groups:
            raise IndexError("group %r of %d" % (g, self.groups))
        lo, hi = int(self.group_first[g]), int(self.group_first[g + 1])
        if self.bases.ndim == 2:
            return self.bases[lo:hi]
        return self.bases[self.offsets[lo]:self.offsets[hi]], self.offsets[lo:hi + 1] - self.offsets[lo]


def _split_host(blob, offsets, n, read_len, first_read, groups, seed, device, want_bases=True):
    """covest_split_reads on host arrays: (out_bases, out_offsets, read_index, group_first)."""
    total = int(offsets[-1] - offsets[0]) if offsets is not None else n * read_len
    out = np.empty(total if want_bases else 0, dtype=np.uint8)
    out_offsets = np.empty(n + 1, dtype=np.int64)
    index = np.empty(n, dtype=np.int64)
    first = np.empty(groups + 1, dtype=np.int64)
    _capi.check(_capi.lib().covest_split_reads(
        int(device), blob.ctypes.data if blob is not None else None, offsets.ctypes.data if offsets is not None else None,
        n, int(read_len), first_read, groups, seed, out.ctypes.data, out_offsets.ctypes.data, index.ctypes.data,
        first.ctypes.data), "covest_split_reads")
    return out, out_offsets, index, first


def read_groups(n_reads, groups, seed=0, first_read=0, device=-1):
    """The group of each of `n_reads` reads numbered from `first_read`, as covest_split_reads deals them: an (n_reads,)
    int64 array.  One device call on reads of no bases (the rule does not look at them): its read_index and
    group_first turned round."""
    groups, seed, first_read = _check_split(groups, seed, first_read)
    if int(n_reads) != n_reads or n_reads < 0:
        raise ValueError("n_reads must not be negative")
    n = int(n_reads)
    _, _, index, first = _split_host(None, None, n, 0, first_read, groups, seed, device, want_bases=False)
    out = np.empty(n, dtype=np.int64)
    out[index - first_read] = np.repeat(np.arange(groups, dtype=np.int64), np.diff(first))
    return out


def split_reads(reads, groups, seed=0, first_read=None, device=-1):
    """Deal the reads of `reads` -- a SimulatedReads, an (n, L) uint8 array or a pair (bases, offsets) in the packed
    layout -- into `groups` seeded groups (1 .. 256) and return them group by group, in input order within a group, as a
    SplitReads.  Read r (its index + `first_read`; default: a SimulatedReads' own first_read, else 0) is of group
    (w * groups) >> 32, w = word 0 of Philox4x32-10 on the counter (lo32(r), hi32(r), 0, 8), key = seed
    (include/covest_amd.h)."""
    groups, seed, first = _check_split(groups, seed, 0 if first_read is None else first_read)
    blob, offsets, n, read_len, source = _packed(reads)
    if first_read is None and source is not None:
        first = int(source.first_read)
    out, out_offsets, index, group_first = _split_host(blob, offsets, n, read_len, first, groups, seed, device)
    if offsets is None:
        out = out.reshape(n, read_len)
    return SplitReads(out, out_offsets, index, group_first, seed)


def split_reads_device(bases_ptr, n_reads, out_bases_ptr, group_first_ptr, groups, seed=0, first_read=0, read_len=0,
                       offsets_ptr=None, out_offsets_ptr=None, read_index_ptr=None, stream=None, device=-1):
    """The same between buffers resident in HBM (raw device pointers, e.g. a torch tensor's data_ptr()), asynchronous on
    `stream`: `n_reads` reads at `bases_ptr`, `read_len` bases each unless `offsets_ptr` (n_reads + 1 int64) is given;
    the reads in group order to `out_bases_ptr` / `out_offsets_ptr` (n_reads + 1 int64; needed with `offsets_ptr`) /
    `read_index_ptr` (n_reads int64, optional); the ranks at which the groups start to the groups + 1 int64 at
    `group_first_ptr`."""
    groups, seed, first_read = _check_split(groups, seed, first_read)
    if n_reads < 0:
        raise ValueError("n_reads must not be negative")
    if not offsets_ptr and read_len < 0:
        raise ValueError("read_len must not be negative")
    if offsets_ptr and not out_offsets_ptr:
        raise ValueError("reads of their own lengths need out_offsets_ptr")
    if not group_first_ptr:
        raise ValueError("group_first_ptr must not be null")
    _capi.require_shared_runtime("split_reads_device")
    _capi.check(_capi.lib().covest_split_reads_device(
        int(device), ctypes.c_void_p(bases_ptr), ctypes.c_void_p(offsets_ptr or 0), int(n_reads), int(read_len), first_read,
        groups, seed, ctypes.c_void_p(out_bases_ptr), ctypes.c_void_p(out_offsets_ptr or 0),
        ctypes.c_void_p(read_index_ptr or 0), ctypes.c_void_p(group_first_ptr), ctypes.c_void_p(stream or 0)),
        "covest_split_reads_device")


class _DeviceArena:
    """The device buffers of sampled_histogram, through the HIP runtime the library is bound to (already mapped into
    the process): they grow on demand and go with the arena."""

    def __init__(self, who="sampled_histogram"):
        self.who = who
        _capi.lib()
        mapped = _capi.hip_runtimes_mapped()
        if mapped is not None and len(mapped) > 1:
            # torch came after the library was loaded and brought a runtime of its own: the library is
            # bound to the other one
            mapped = [p for p in mapped if "torch" not in p]
            if len(mapped) != 1:
                raise _capi.CovestHipError(who + ": cannot tell which of the HIP runtimes of this process "
                                           "the library is bound to -- `import torch` before the first covest_amd call")
        try:
            self.hip = ctypes.CDLL(mapped[0] if mapped else "libamdhip64.so")
        except OSError as e:
            raise _capi.CovestHipError("%s: cannot reach the HIP runtime: %s" % (who, e))
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
        self.hip.hipFree.argtypes = [vp]
        self.hip.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
        for fn in (self.hip.hipMalloc, self.hip.hipFree, self.hip.hipMemcpy):
            fn.restype = ctypes.c_int
        self.bufs = {}

    def _ok(self, rc, what):
        if rc != 0:
            raise _capi.CovestHipError("%s: %s failed (HIP error %d)" % (self.who, what, rc))

    def reserve(self, name, n_bytes):
        ptr, cap = self.bufs.get(name, (None, 0))
        if n_bytes > cap:
            if ptr:
                self._ok(self.hip.hipFree(ptr), "hipFree")
                del self.bufs[name]
            p = ctypes.c_void_p()
            self._ok(self.hip.hipMalloc(ctypes.byref(p), max(int(n_bytes), 256)), "hipMalloc")
            self.bufs[name] = (p.value, max(int(n_bytes), 256))
        return self.bufs[name][0]

    def upload(self, name, host_ptr, n_bytes):
        ptr = self.reserve(name, n_bytes)
        if n_bytes:
            self._ok(self.hip.hipMemcpy(ptr, host_ptr, n_bytes, 1), "hipMemcpy to the device")  # (waits)
        return ptr

    def download(self, name, array):
        self._ok(self.hip.hipMemcpy(array.ctypes.data, self.bufs[name][0], array.nbytes, 2), "hipMemcpy from the device")

    def close(self):
        for ptr, _ in self.bufs.values():
            self.hip.hipFree(ptr)  # (waits for the device)
        self.bufs = {}


def sampled_histogram(fname, k, factor, seed=0, canonical=False, n_strategy=NS_IGNORE, batch_bases=1 << 26):
    """The k-mer histogram of the reads of `fname` sampled at `factor`: the loop of kmer_hist.main with the sampler
    between reader and counter.  Each batch goes up once, is sampled on the device (first_read = reads seen so far) and
    counted from where the sampler left it; only the two counts come back.  The result does not depend on
    `batch_bases`."""
    factor, seed, _ = _check(factor, seed, 0)
    counts = KmerCounts(k, canonical=canonical)
    arena = None
    try:
        arena = _DeviceArena()
        seen = 0
        pair = np.zeros(2, dtype=np.int64)
        for bases, offsets, n, n_bases in ReadBatches(fname, n_strategy, batch_bases=batch_bases):
            d_in = arena.upload("in", ctypes.cast(bases, ctypes.c_void_p), n_bases)
            d_off = arena.upload("offsets", ctypes.cast(offsets, ctypes.c_void_p), 8 * (n + 1))
            d_out = arena.reserve("out", n_bases)
            d_out_off = arena.reserve("out_offsets", 8 * (n + 1))
            d_counts = arena.reserve("counts", 16)
            sample_reads_device(d_in, n, d_out, d_counts, factor, seed=seed, first_read=seen, offsets_ptr=d_off,
                                out_offsets_ptr=d_out_off)
            arena.download("counts", pair)  # (the null stream: waits for the sampler)
            seen += n
            n_kept, kept_bases = int(pair[0]), int(pair[1])
            if n_kept:
                counts._reserve_for(kept_bases + n_kept)  # k-mers the batch can add: sum(max(len - k + 1, 1))
                counts.add_device(d_out, n_kept, 0, d_offsets_ptr=d_out_off, reserve=False)
        return counts.histogram()  # (waits for the counter)
    finally:
        counts.close()
        if arena is not None:
            arena.close()


def sample_reads_file(src, dest, factor, seed=0, n_strategy=NS_IGNORE, batch_bases=1 << 26, device=-1):
    """The reference's sample_reads / bin/read_sampler.py over the library's reader: the reads of `src` (FASTA or FASTQ)
    kept with probability 1 / factor, written to `dest` as FASTA.  Two divergences, both stated: a record is named
    'read_{global index}' (the reader keeps no ids), and its sequence is as the reader preprocesses it (lower case,
    `n_strategy` applied).  Returns (reads seen, reads kept)."""
    factor, seed, _ = _check(factor, seed, 0)
    seen = n_kept = 0
    with open(dest, "w") as f:
        for bases, offsets, n, n_bases in ReadBatches(src, n_strategy, batch_bases=batch_bases):
            blob = np.ctypeslib.as_array(bases, shape=(max(n_bases, 1),))[:n_bases]
            offs = np.ctypeslib.as_array(offsets, shape=(n + 1,))
            out, out_offsets, kept = _sample_host(blob, offs, n, 0, seen, factor, seed, device)
            _write_records(f, out, out_offsets, kept)
            seen += n
            n_kept += kept.size
    return seen, n_kept


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Keep every read of SRC with probability 1 / FACTOR; write them to DEST (FASTA).")
    ap.add_argument("src")
    ap.add_argument("dest")
    ap.add_argument("-f", "--factor", type=float, required=True)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    seen, kept = sample_reads_file(args.src, args.dest, args.factor, seed=args.seed)
    print("%d of %d reads kept" % (kept, seen))


if __name__ == "__main__":
    main()
