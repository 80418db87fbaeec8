"""k-mer abundance histogram on the GPU: the counterpart of the reference's bin/kmer_hist.py
(BASELINE.json config 5).

Same functions, same argument meaning: `preprocess` (:44-54), `compute_counts(seq,
prev_counts=None, k=20)` (:34-41), `compute_histogram(counts)` (:57-64), `main` (:77-89), plus
the 2-bit hash helpers (:14-31).  The `counts` object is a hash table in HBM behind the C ABI
(covest_kmer_* in include/covest_amd.h) instead of a Python dict; every k-mer is counted by the
HIP kernel kmer_count.hip.  There is no CPU fallback.

Differences from the reference, all deliberate and listed in DESIGN.md:
  * `main` passes its `k` on (the reference's main ignores -k and always counts 20-mers, :81);
  * `canonical=True` (jellyfish -C: a k-mer and its reverse complement are one key) is offered
    because BASELINE.json's config 5 asks for it; the default is the reference's forward strand;
  * k <= 255: k <= 31 packs key and empty marker into one 64-bit word (kmer_count.hip, the fast path); larger k takes
    keys of 2, 4 or 8 words (kmer_wide.hip) -- the reference's Python integers have no limit; counts are 64-bit.
"""
import ctypes
import random
from os import path

import numpy as np

from . import _capi

NS_IGNORE = 0
NS_SINGLE = 1
NS_RANDOM = 2

_CODES = {'a': 0, 'c': 1, 'g': 2, 't': 3}
_VALID = np.zeros(256, dtype=bool)
for _ch in "acgtACGT":
    _VALID[ord(_ch)] = True


def single_hash(b):
    """bin/kmer_hist.py:14-15."""
    return _CODES[b]


def hash_kmer(kmer):
    """bin/kmer_hist.py:18-23."""
    h = 0
    for b in kmer:
        h <<= 2
        h |= single_hash(b)
    return h


def rehash(old_hash, b, k):
    """bin/kmer_hist.py:26-31."""
    h = old_hash & ((1 << (2 * k - 2)) - 1)
    h <<= 2
    h |= single_hash(b)
    return h


def preprocess(seq, nstrategy=NS_IGNORE):
    """bin/kmer_hist.py:44-54 (host string work, as in the reference)."""
    seq = str(seq).lower()
    if nstrategy == NS_IGNORE:
        seq = seq.replace('n', '')
    elif nstrategy == NS_SINGLE:
        seq = seq.replace('n', 'a')
    elif nstrategy == NS_RANDOM:
        seq = ''.join(random.choice(['a', 'c', 'g', 't']) if b == 'n' else b for b in seq)
    else:
        raise ValueError('Invalid N strategy')
    return seq


def scatter_rate(slots, ops=1 << 28, device=0):
    """Returning 64-bit atomic adds per second at pseudo-random places of a `slots`-word array on this device
    (covest_kmer_scatter_rate): the measured roof of pass 1 of the partitioned path."""
    out = ctypes.c_double()
    _capi.check(_capi.lib().covest_kmer_scatter_rate(int(device), int(slots), int(ops), ctypes.byref(out)),
                "covest_kmer_scatter_rate")
    return out.value


NO_WINDOW = 0xFFFFFFFF  # in the flat abundance array: no window starts at this base


def _bases_and_offsets(bases, offsets):
    """The rule of a pair (bases, offsets) in the packed layout, and the pair as contiguous uint8 and int64 arrays: the
    bases one-dimensional uint8, the offsets n_reads + 1 integers that ascend from a non-negative start and do not reach
    beyond the bases (ValueError)."""
    bases, offsets = np.asarray(bases), np.asarray(offsets)
    if bases.dtype != np.uint8 or bases.ndim != 1:
        raise ValueError("bases must be a one-dimensional uint8 array")
    if offsets.ndim != 1 or offsets.size < 1 or offsets.dtype.kind not in "iu":
        raise ValueError("offsets must be a one-dimensional integer array of n_reads + 1 entries")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets[0] < 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must ascend from a non-negative start")
    if offsets[-1] > bases.size:
        raise ValueError("offsets reach beyond the bases")
    return np.ascontiguousarray(bases), offsets


def _packed_reads(reads):
    """(bases uint8[...], offsets int64[n + 1]) of what KmerCounts.lookup takes: a list of strings, a pair (bases,
    offsets), an (n, L) uint8 array or an object that carries one as `.bases` (SimulatedReads).  ValueError for
    malformed arrays, KeyError for a base outside acgt -- both before the library is asked."""
    if hasattr(reads, "bases") and getattr(reads.bases, "ndim", 0) == 2:
        reads = reads.bases
    if isinstance(reads, np.ndarray):
        if reads.dtype != np.uint8 or reads.ndim != 2:
            raise ValueError("reads as one array must be (n, L) uint8")
        blob = np.ascontiguousarray(reads).reshape(-1)
        offsets = np.arange(reads.shape[0] + 1, dtype=np.int64) * reads.shape[1]
    elif isinstance(reads, tuple) and len(reads) == 2 and not isinstance(reads[0], str):
        blob, offsets = _bases_and_offsets(*reads)
    else:
        reads = [r if isinstance(r, str) else str(r) for r in reads]
        lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
        offsets = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        try:
            blob = np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8)
        except UnicodeEncodeError:
            raise KeyError("base outside acgt")
    used = blob[int(offsets[0]):int(offsets[-1])]
    if used.size and not _VALID[used].all():
        raise KeyError("base outside acgt")  # single_hash raises KeyError (bin/kmer_hist.py:15)
    return blob, offsets


def _read_weights(weights, n_reads):
    """The uint32 array of KmerCounts.add_weighted: one weight a read, whole numbers in 0 .. 2^32 - 1; ValueError before
    the library is asked."""
    w = np.asarray(weights)
    if w.ndim != 1 or w.size != n_reads:
        raise ValueError("weights must be a one-dimensional array of one entry per read")
    if w.size and w.dtype.kind not in "iu":
        raise ValueError("weights must be integers")
    if w.size and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF):
        raise ValueError("weights must be within 0 .. 2^32 - 1")
    return np.ascontiguousarray(w, dtype=np.uint32)


MAX_INFLUENCE_COLUMNS = 8      # csrc/kmer_influence.h kInfluenceMaxCols
MAX_INFLUENCE_WINDOWS = 4096   # ... kInfluenceMaxWindows


def _influence_table(table):
    """The (n_rows, n_cols) float64 table of KmerCounts.read_influence, C-contiguous; ValueError before the library is
    asked."""
    table = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    if table.ndim != 2 or table.shape[0] < 1 or not 1 <= table.shape[1] <= MAX_INFLUENCE_COLUMNS:
        raise ValueError("table must be (n_rows, n_cols) with at least one row and 1 .. %d columns" % MAX_INFLUENCE_COLUMNS)
    return table


def _or_minus_one(column):
    out = column.astype(np.int64)
    out[column == NO_WINDOW] = -1
    return out


class ReadAbundances:
    """What KmerCounts.lookup returns.  `abundance`: the flat uint32 array indexed like the bases from offsets[0] on
    (None with per_window=False) -- at a window's first base min(count, 0xFFFFFFFE), NO_WINDOW at the last k - 1 bases
    of a read; `offsets` (n + 1,) int64 from 0; `windows(i)`: the valid entries of read i; per read, int64 with -1 for
    "none": `min_abundance` (no window), `weak` (never -1), `first_weak` / `last_weak` (window indices; no weak
    window); `score` (float64, None without weights); `k`, `cutoff`."""

    def __init__(self, k, offsets, abundance, summary, score, cutoff):
        self.k = int(k)
        self.offsets = offsets
        self.abundance = abundance
        self.summary = summary
        self.score = score
        self.cutoff = int(cutoff)
        self.min_abundance = _or_minus_one(summary[:, 0])
        self.weak = summary[:, 1].astype(np.int64)
        self.first_weak = _or_minus_one(summary[:, 2])
        self.last_weak = _or_minus_one(summary[:, 3])

    @property
    def n_reads(self):
        return self.offsets.size - 1

    @property
    def n_windows(self):
        """Windows per read: max(length - k + 1, 0)."""
        return np.maximum(np.diff(self.offsets) - self.k + 1, 0)

    def windows(self, i):
        if self.abundance is None:
            raise ValueError("the lookup was made with per_window=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.abundance[a:max(a, b - self.k + 1)]


class CorrectedReads:
    """What KmerCounts.correct returns.  `bases`: the flat uint8 array of the reads after correction, indexed from
    offsets[0] on; `offsets` (n + 1,) int64 from 0; per read, int64: `runs` of weak windows, and how many of them were
    `corrected`, `ambiguous`, `unfixable` (runs is their sum); `changed`: the flat positions where `bases` differs from
    the input; `strings()`: the reads as strings; `k`, `cutoff`."""

    def __init__(self, k, bases, offsets, fix, changed, cutoff):
        self.k = int(k)
        self.bases = bases
        self.offsets = offsets
        self.fix = fix
        self.changed = changed
        self.cutoff = int(cutoff)
        self.runs, self.corrected, self.ambiguous, self.unfixable = (fix[:, j].astype(np.int64) for j in range(4))

    @property
    def n_reads(self):
        return self.offsets.size - 1

    def strings(self):
        text = self.bases.tobytes().decode("ascii")
        return [text[int(a):int(b)] for a, b in zip(self.offsets[:-1], self.offsets[1:])]


class KmerCounts:
    """The `counts` of compute_counts: an open-addressing table in HBM (covest_kmer*)."""

    def __init__(self, k=20, canonical=False, device=-1, min_slots=1 << 16):
        self.k = int(k)
        self.canonical = bool(canonical)
        self._distinct = 0  # slots OCCUPIED when last measured (the distinct k-mers, until something is removed)
        self._added = 0     # k-mer occurrences inserted since: _distinct + _added bounds the occupied slots
        self._partitioned = False  # the counter holds a count_reads_device result (no table to ask for its occupancy)
        h = ctypes.c_void_p()
        _capi.check(_capi.lib().covest_kmer_create(self.k, 1 if canonical else 0, int(min_slots),
                                                   int(device), ctypes.byref(h)), "covest_kmer_create")
        self._handle = h

    def close(self):
        if getattr(self, "_handle", None) is not None:
            _capi.lib().covest_kmer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def slots(self):
        return int(_capi.lib().covest_kmer_slots(self._handle))

    def _measure(self):
        """(keys held, slots occupied) as the table has them now.  Only a removal makes the two differ, and only the
        one-word table (k <= 31) can be removed from: elsewhere both are the distinct count."""
        if self.k > 31 or self._partitioned:
            distinct = self.stats()[1]
            return distinct, distinct
        return self.occupancy()

    def _reserve_for(self, n_new):
        """Keep the table at most half full of OCCUPIED slots -- of distinct k-mers, as long as nothing was removed; a
        key whose count a removal brought to 0 still takes its slot.  The occupied slots are bounded by what was
        measured last plus every occurrence inserted since; only when that bound no longer fits is the table asked
        (one small kernel).  Where the slots occupied now and the batch fit, nothing happens.  Else the keys of count
        0 are let go: by compact() where the keys HELD and the batch fit the table as it is, else by a reserve for the
        keys held plus the batch about to be added (its rehash takes the held keys alone) -- never for the cumulative
        number of occurrences (10 Gbp of reads of a 100 Mbp genome need a table for ~1e8 k-mers, not 1e10)."""
        n_new = int(n_new)
        if 2 * (self._distinct + self._added + n_new) + 1024 > self.slots:
            held, occupied = self._measure()
            self._distinct, self._added = occupied, 0
            if 2 * (occupied + n_new) + 1024 > self.slots:
                if held < occupied and 2 * (held + n_new) + 1024 <= self.slots:
                    _capi.check(_capi.lib().covest_kmer_compact(self._handle), "covest_kmer_compact")
                else:
                    _capi.check(_capi.lib().covest_kmer_reserve(self._handle, 2 * (held + n_new) + 1024),
                                "covest_kmer_reserve")
                self._distinct = held
        self._added += n_new

    def _update_host(self, name, blob, offsets, weights=None):
        """A host form of covest_kmer_{add,remove}[_weighted] by its C name: packed reads (_packed_reads), and a uint32
        weight a read (_read_weights) where the form is weighted."""
        u8p, i64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)   # (covest_kmer_add's prototype is typed)
        args = (self._handle, blob.ctypes.data_as(u8p), offsets.ctypes.data_as(i64p), offsets.size - 1)
        if weights is not None:
            args += (ctypes.c_void_p(weights.ctypes.data),)
        _capi.check(getattr(_capi.lib(), name)(*args), name)
        return self

    def _update_device(self, name, d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream, d_weights_ptr=None, weighted=False):
        """A device form of covest_kmer_{add,remove}[_weighted]_device by its C name: raw device pointers, asynchronous
        on `stream`.  `weighted` says whether the C function takes weights at all; a weighted form is handed a null
        `d_weights_ptr` as it comes (the library refuses it by name), so the pointer cannot stand in for the flag."""
        _capi.require_shared_runtime("KmerCounts." + name[len("covest_kmer_"):])
        args = (self._handle, ctypes.c_void_p(d_bases_ptr), ctypes.c_void_p(d_offsets_ptr or 0), int(n_reads), int(read_len))
        if weighted:
            args += (ctypes.c_void_p(d_weights_ptr or 0),)
        _capi.check(getattr(_capi.lib(), name)(*args, ctypes.c_void_p(stream or 0)), name)
        return self

    def add_reads(self, reads):
        """Count the k-mers of preprocessed reads (only a/c/g/t, either case) in one launch."""
        reads = [r if isinstance(r, str) else str(r) for r in reads]
        if not reads:
            return self
        lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
        offsets = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        blob = np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8)
        if blob.size and not _VALID[blob].all():
            raise KeyError("base outside acgt")  # single_hash raises KeyError (bin/kmer_hist.py:15)
        self._reserve_for(int(np.maximum(lens - self.k + 1, 1).sum()))
        return self._update_host("covest_kmer_add", np.ascontiguousarray(blob), offsets)

    def add_packed(self, bases, offsets, n_reads, n_bases):
        """Preprocessed reads in the packed host layout of covest_kmer_add (ctypes pointers: the bases back to
        back, offsets[n_reads + 1]) -- what ReadBatches yields."""
        if n_reads <= 0:
            return self
        # k-mers the batch can add: sum(max(len - k + 1, 1)) <= n_bases + n_reads
        self._reserve_for(int(n_bases) + int(n_reads))
        _capi.check(_capi.lib().covest_kmer_add(self._handle, bases, offsets, int(n_reads)), "covest_kmer_add")
        return self

    def add_device(self, d_bases_ptr, n_reads, read_len, d_offsets_ptr=None, stream=None, reserve=True):
        """Reads already resident in HBM (raw device pointers); asynchronous on `stream`.
        reserve=False: the caller sized the table for the DISTINCT k-mers it expects (an
        overflow is reported by the next histogram call)."""
        n_new = int(n_reads) * max(int(read_len) - self.k + 1, 1)
        if reserve:
            self._reserve_for(n_new)
        else:  # still occurrences inserted since the last measurement: later batches must see them in the bound
            self._added += n_new
        return self._update_device("covest_kmer_add_device", d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream)

    def add_weighted(self, reads, weights):
        """Count the k-mers of `reads` -- what lookup takes: a list of preprocessed strings, a pair (bases, offsets), an
        (n, L) uint8 array -- with every occurrence of read r added weights[r] times (covest_kmer_add_weighted): a weight
        of 0 adds nothing and creates no key, all weights 1 is add_reads.  `weights`: n integers in 0 .. 2^32 - 1.  The
        table is sized as for the unweighted add: weights never add distinct keys."""
        blob, offsets = _packed_reads(reads)
        n = offsets.size - 1
        weights = _read_weights(weights, n)
        if not n:
            return self
        self._reserve_for(int(np.maximum(np.diff(offsets) - self.k + 1, 1).sum()))
        return self._update_host("covest_kmer_add_weighted", blob, offsets, weights)

    def add_weighted_device(self, d_bases_ptr, n_reads, read_len, d_weights_ptr, d_offsets_ptr=None, stream=None,
                            reserve=True):
        """add_device with a weight per read resident in HBM (`d_weights_ptr`: n_reads uint32, aligned to 4 bytes;
        covest_kmer_add_weighted_device): asynchronous on `stream`, where the weights are read -- a
        bootstrap_weights_device on the same stream needs no synchronisation before it.  `reserve` as add_device's."""
        n_new = int(n_reads) * max(int(read_len) - self.k + 1, 1)
        if reserve:
            self._reserve_for(n_new)
        else:
            self._added += n_new
        return self._update_device("covest_kmer_add_weighted_device", d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream,
                                   d_weights_ptr, weighted=True)

    def remove(self, reads):
        """Take the k-mers of `reads` -- what lookup takes -- out of the table again (covest_kmer_remove; k <= 31):
        add_reads' inverse.  No key is cleared: a key nothing supports any more keeps its slot with a count of 0, is no
        longer held (stats(), len(), histogram(), lookup) and still occupied (occupancy()).  Removing what was never
        added is an UNDERFLOW: this call, and every later histogram() and host-form call until clear(), raises
        CovestHipError with "underflow"; the counts are then unspecified."""
        blob, offsets = _packed_reads(reads)
        return self._update_host("covest_kmer_remove", blob, offsets) if offsets.size > 1 else self

    def remove_weighted(self, reads, weights):
        """remove with every occurrence of read r taken out weights[r] times (covest_kmer_remove_weighted):
        add_weighted's inverse.  A weight of 0 takes nothing out, also of a read that was never added."""
        blob, offsets = _packed_reads(reads)
        weights = _read_weights(weights, offsets.size - 1)
        return self._update_host("covest_kmer_remove_weighted", blob, offsets, weights) if offsets.size > 1 else self

    def remove_device(self, d_bases_ptr, n_reads, read_len, d_offsets_ptr=None, stream=None):
        """add_device's inverse for reads resident in HBM (raw device pointers; covest_kmer_remove_device): asynchronous
        on `stream`, which must be the stream of the adds it takes back (or ordered after them by the caller).  It does
        not look at the underflow state: the next histogram() reports it."""
        return self._update_device("covest_kmer_remove_device", d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream)

    def remove_weighted_device(self, d_bases_ptr, n_reads, read_len, d_weights_ptr, d_offsets_ptr=None, stream=None):
        """remove_device with a weight per read resident in HBM (`d_weights_ptr`: n_reads uint32, aligned to 4 bytes;
        covest_kmer_remove_weighted_device): the weights are read on `stream`."""
        return self._update_device("covest_kmer_remove_weighted_device", d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream,
                                   d_weights_ptr, weighted=True)

    def replace_reads(self, before, after, changed):
        """The reads `before` replaced by `after` in the table, where `changed` flags them: two read sets of equal shape
        (as many reads, each as long as its partner; what lookup takes) and one flag (0 / 1, or bool) per read.  It is
        remove_weighted(before, changed), then add_weighted(after, changed): where the two sets differ in the flagged
        reads only, the table then equals a fresh count of `after`.  correct()'s output and its per-read `corrected`
        > 0 feed it directly.  ValueError, before the library is asked, for sets of different shape and for flags that
        are not one 0 / 1 per read."""
        blob_b, off_b = _packed_reads(before)
        blob_a, off_a = _packed_reads(after)
        if off_b.size != off_a.size or (np.diff(off_b) != np.diff(off_a)).any():
            raise ValueError("replace_reads: before and after must be read sets of equal shape")
        flags = np.asarray(changed)
        if flags.dtype == np.bool_:
            flags = flags.astype(np.uint32)
        flags = _read_weights(flags, off_b.size - 1)
        if flags.size and int(flags.max()) > 1:
            raise ValueError("replace_reads: changed must be one flag (0 or 1) per read")
        self.remove_weighted((blob_b, off_b), flags)
        return self.add_weighted((blob_a, off_a), flags)

    def occupancy(self):
        """(keys held, slots occupied) (covest_kmer_occupancy; k <= 31): held = with a count of at least 1, what
        stats() and len() speak of; occupied = slots that carry a key at all, what bounds how full the table is.  They
        differ only after a removal."""
        out = (ctypes.c_int64 * 2)()
        _capi.check(_capi.lib().covest_kmer_occupancy(self._handle, out), "covest_kmer_occupancy")
        return int(out[0]), int(out[1])

    def compact(self):
        """Rehash into a table of the same size (covest_kmer_compact; k <= 31): the keys of count 0 go, occupied ==
        held afterwards."""
        _capi.check(_capi.lib().covest_kmer_compact(self._handle), "covest_kmer_compact")
        self._distinct, self._added = self.occupancy()[1], 0
        return self

    def count_reads_device(self, d_bases_ptr, n_reads, read_len, d_offsets_ptr=None, n_bases=None, stream=None):
        """ALL the k-mers of reads resident in HBM into this (emptied) counter -- the loop of main,
        bin/kmer_hist.py:77-89 -- by the partitioned path where it applies (covest_kmer_count_reads_device: k = 19..31,
        no read shorter than k, buckets that fit the device), else through the table (clear + add_device).  Afterwards
        the counter answers histogram() / len() exactly; after the partitioned path it holds no dict to add to
        (clear() first).  Returns the name of the path taken."""
        n_bases = int(n_bases if n_bases is not None else int(n_reads) * max(int(read_len), 0))
        _capi.require_shared_runtime("KmerCounts.count_reads_device")
        rc = _capi.lib().covest_kmer_count_reads_device(
            self._handle, ctypes.c_void_p(d_bases_ptr), ctypes.c_void_p(d_offsets_ptr or 0), int(n_reads), int(read_len),
            n_bases, ctypes.c_void_p(stream or 0))
        if rc == 0:
            self._distinct = self._added = 0
            self._partitioned = True
            return "partitioned"
        if rc not in (_capi.COVEST_E_UNSUPPORTED, _capi.COVEST_E_NOMEM):
            _capi.check(rc, "covest_kmer_count_reads_device")
        self.why_not_partitioned = _capi.last_error()
        self.clear(stream)
        if d_offsets_ptr:
            self._reserve_for(n_bases + int(n_reads))
            self.add_device(d_bases_ptr, n_reads, 0, d_offsets_ptr=d_offsets_ptr, stream=stream, reserve=False)
        else:
            self.add_device(d_bases_ptr, n_reads, read_len, stream=stream)
        return "table"

    def lookup(self, reads, cutoff=0, weights=None, per_window=True):
        """The abundance the table holds for every k-mer of `reads` (covest_kmer_lookup_reads; k <= 31, read-only) ->
        ReadAbundances.  `reads`: a list of preprocessed strings (KeyError for a base outside acgt, like add_reads) or a
        pair (bases, offsets) in the packed layout.  `cutoff`: a window is weak when its abundance is below it (0: none
        is).  `weights`: a table of doubles; the score of a read is the sum over its windows of
        weights[min(abundance, len(weights) - 1)], in a fixed order (the same bits on every run).  per_window=False:
        only the per-read summaries come back.  A read shorter than k has no window (the key add_reads counts for it is
        not looked up)."""
        blob, offsets = _packed_reads(reads)
        cutoff = int(cutoff)
        if not 0 <= cutoff <= 0xFFFFFFFF:
            raise ValueError("cutoff must fit 32 bits, not negative")
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
            if weights.ndim != 1 or weights.size < 1 or weights.size >= 1 << 31:
                raise ValueError("weights must be a one-dimensional table of at least one number")
        n = offsets.size - 1
        n_pos = int(offsets[-1] - offsets[0])
        abundance = np.empty(n_pos, dtype=np.uint32) if per_window else None
        summary = np.empty((n, 4), dtype=np.uint32)
        score = np.empty(n, dtype=np.float64) if weights is not None else None
        if n:
            def ptr(a):
                return ctypes.c_void_p(a.ctypes.data if a is not None else 0)
            _capi.check(_capi.lib().covest_kmer_lookup_reads(
                self._handle, ptr(blob), ptr(offsets), n, cutoff, ptr(weights), 0 if weights is None else weights.size,
                ptr(abundance), ptr(summary), ptr(score)), "covest_kmer_lookup_reads")
        return ReadAbundances(self.k, offsets - offsets[0], abundance, summary, score, cutoff)

    def lookup_device(self, d_bases_ptr, n_reads, read_len, d_offsets_ptr=None, cutoff=0, d_weights_ptr=None, n_weights=0,
                      d_abundance_ptr=None, d_summary_ptr=None, d_score_ptr=None, stream=None):
        """The same for reads resident in HBM into device arrays (raw pointers; covest_kmer_lookup_reads_device):
        asynchronous on `stream`, which must be the stream of the adds it is to see (or ordered after them by the
        caller).  Every output is optional; `d_abundance_ptr` is indexed like the bases, `d_summary_ptr` holds
        uint32[n_reads][4] (16-byte aligned), `d_score_ptr` doubles.  It does not look at the overflow flag."""
        _capi.require_shared_runtime("KmerCounts.lookup_device")
        _capi.check(_capi.lib().covest_kmer_lookup_reads_device(
            self._handle, ctypes.c_void_p(d_bases_ptr), ctypes.c_void_p(d_offsets_ptr or 0), int(n_reads), int(read_len),
            int(cutoff), ctypes.c_void_p(d_weights_ptr or 0), int(n_weights), ctypes.c_void_p(d_abundance_ptr or 0),
            ctypes.c_void_p(d_summary_ptr or 0), ctypes.c_void_p(d_score_ptr or 0), ctypes.c_void_p(stream or 0)),
            "covest_kmer_lookup_reads_device")
        return self

    def correct(self, reads, cutoff):
        """Isolated substitutions of `reads` corrected from the table (covest_kmer_correct_reads; k <= 31, read-only on
        the table) -> CorrectedReads.  `reads`: what lookup takes.  A window is weak when its abundance is below
        `cutoff`; for every run of weak windows the other three bases are tried at the position(s) the run names, and
        the base is replaced when exactly one alternative lifts every window of the run to the cutoff (the rule:
        include/covest_amd.h).  Two errors closer than k + 1 merge into one run and stay."""
        blob, offsets = _packed_reads(reads)
        cutoff = int(cutoff)
        if not 0 <= cutoff <= 0xFFFFFFFF:
            raise ValueError("cutoff must fit 32 bits, not negative")
        n = offsets.size - 1
        before = blob[int(offsets[0]):int(offsets[-1])]
        out = np.empty(before.size, dtype=np.uint8)
        fix = np.zeros((n, 4), dtype=np.uint32)
        if n:
            _capi.check(_capi.lib().covest_kmer_correct_reads(
                self._handle, ctypes.c_void_p(blob.ctypes.data), ctypes.c_void_p(offsets.ctypes.data), n, cutoff,
                ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(fix.ctypes.data)), "covest_kmer_correct_reads")
        return CorrectedReads(self.k, out, offsets - offsets[0], fix, np.flatnonzero(out != before), cutoff)

    def correct_device(self, d_bases_ptr, n_reads, read_len, d_out_ptr, d_offsets_ptr=None, cutoff=0, d_fix_ptr=None,
                       stream=None):
        """The same for reads resident in HBM into device arrays (raw pointers; covest_kmer_correct_reads_device):
        asynchronous on `stream`, which must be the stream of the adds it is to see (or ordered after them by the
        caller).  `d_out_ptr` is indexed like the bases and may be `d_bases_ptr` itself (in place); otherwise the two
        must not overlap.  `d_fix_ptr` (optional) holds uint32[n_reads][4] = {runs, corrected, ambiguous, unfixable},
        16-byte aligned.  It does not look at the overflow flag."""
        _capi.require_shared_runtime("KmerCounts.correct_device")
        _capi.check(_capi.lib().covest_kmer_correct_reads_device(
            self._handle, ctypes.c_void_p(d_bases_ptr), ctypes.c_void_p(d_offsets_ptr or 0), int(n_reads), int(read_len),
            int(cutoff), ctypes.c_void_p(d_out_ptr or 0), ctypes.c_void_p(d_fix_ptr or 0), ctypes.c_void_p(stream or 0)),
            "covest_kmer_correct_reads_device")
        return self

    def read_influence(self, reads, table):
        """What deleting each read alone does to a sum over the distinct k-mers (covest_kmer_read_influence; k <= 31,
        read-only) -> float64 (n, n_cols + 1).  `reads`: what lookup takes.  `table`: (n_rows, n_cols) doubles, 1 <=
        n_cols <= 8, row i the value at abundance i, abundances beyond the last row take the last row.  Column c of row
        r is the sum over the DISTINCT keys x of read r of table[a_x - m_x][c] - table[a_x][c], a_x the table's count
        and m_x the windows of r with key x; the last column is the number of windows.  A read shorter than k gives
        zeros; a read with more than MAX_INFLUENCE_WINDOWS windows raises CovestHipError (the compare is quadratic).
        The sums are made in a fixed order: the same bits on every run (covest_amd.influence)."""
        blob, offsets = _packed_reads(reads)
        table = _influence_table(table)
        n = offsets.size - 1
        rows = np.zeros((n, table.shape[1] + 1), dtype=np.float64)
        if n:
            _capi.check(_capi.lib().covest_kmer_read_influence(
                self._handle, ctypes.c_void_p(blob.ctypes.data), ctypes.c_void_p(offsets.ctypes.data), n,
                ctypes.c_void_p(table.ctypes.data), table.shape[0], table.shape[1], ctypes.c_void_p(rows.ctypes.data)),
                "covest_kmer_read_influence")
        return rows

    def read_influence_device(self, d_bases_ptr, n_reads, read_len, d_table_ptr, n_rows, n_cols, d_rows_ptr,
                              d_offsets_ptr=None, stream=None):
        """The same for reads resident in HBM into a device array (raw pointers; covest_kmer_read_influence_device):
        asynchronous on `stream`, which must be the stream of the adds it is to see (or ordered after them by the
        caller).  `d_table_ptr`: double[n_rows][n_cols]; `d_rows_ptr`: double[n_reads][n_cols + 1], both aligned to 8
        bytes.  With offsets a read of more than MAX_INFLUENCE_WINDOWS windows gets NaN in its value columns; reads of
        one length that long are refused.  It does not look at the overflow flag."""
        _capi.require_shared_runtime("KmerCounts.read_influence_device")
        _capi.check(_capi.lib().covest_kmer_read_influence_device(
            self._handle, ctypes.c_void_p(d_bases_ptr), ctypes.c_void_p(d_offsets_ptr or 0), int(n_reads), int(read_len),
            ctypes.c_void_p(d_table_ptr or 0), int(n_rows), int(n_cols), ctypes.c_void_p(d_rows_ptr or 0),
            ctypes.c_void_p(stream or 0)), "covest_kmer_read_influence_device")
        return self

    def join_histogram(self, other, rows, cols):
        """This counter joined with `other` (a KmerCounts of the same k, canonical flag and device; k <= 31) on their
        keys (covest_kmer_join_histogram; read-only on both) -> int64 (rows, cols): entry [i][j] is the number of keys
        held by at least one of the two whose count here, clipped to rows - 1, is i and whose count in `other`, clipped
        to cols - 1, is j.  Row 0: the keys of `other` alone; column 0: the keys of this counter alone.  rows * cols is
        at most 2^22.  Integer counts: the same result on every run (covest_amd.copy_spectrum)."""
        rows, cols = int(rows), int(cols)
        if not isinstance(other, KmerCounts):
            raise TypeError("join_histogram joins two KmerCounts")
        out = np.zeros((rows, cols) if rows >= 1 and cols >= 1 and rows * cols <= 1 << 22 else (1, 1), dtype=np.int64)
        _capi.check(_capi.lib().covest_kmer_join_histogram(
            self._handle, other._handle, rows, cols, ctypes.c_void_p(out.ctypes.data)), "covest_kmer_join_histogram")
        return out

    def join_histogram_device(self, other, rows, cols, d_out_ptr, stream=None):
        """The same into a device array (raw pointer; covest_kmer_join_histogram_device): asynchronous on `stream`,
        which must be the stream of the adds into BOTH counters that it is to see (or ordered after them by the
        caller).  `d_out_ptr`: int64[rows][cols], aligned to 8 bytes; the call zeroes it on `stream` first.  It does
        not look at an overflow flag."""
        if not isinstance(other, KmerCounts):
            raise TypeError("join_histogram_device joins two KmerCounts")
        _capi.require_shared_runtime("KmerCounts.join_histogram_device")
        _capi.check(_capi.lib().covest_kmer_join_histogram_device(
            self._handle, other._handle, int(rows), int(cols), ctypes.c_void_p(d_out_ptr or 0),
            ctypes.c_void_p(stream or 0)), "covest_kmer_join_histogram_device")
        return self

    def memory_limit(self, max_bytes):
        """Bytes the partitioned path may allocate for its buckets' records (0: no cap but the free device memory); a
        count_reads_device that would pass it takes the table path instead (covest_kmer_memory_limit)."""
        _capi.check(_capi.lib().covest_kmer_memory_limit(self._handle, int(max_bytes)), "covest_kmer_memory_limit")
        return self

    def partition_info(self):
        """How the last partitioned count went (covest_kmer_partition_info), as a dict."""
        out = (ctypes.c_int64 * 8)()
        _capi.check(_capi.lib().covest_kmer_partition_info(self._handle, out), "covest_kmer_partition_info")
        names = ("buckets", "minimizer", "sampled_1_in", "room_records", "overflowed_records", "buckets_by_workgroup",
                 "buckets_through_table", "records")
        info = dict(zip(names, list(out)))
        ms = (ctypes.c_double * 4)()
        _capi.check(_capi.lib().covest_kmer_partition_ms(self._handle, ms), "covest_kmer_partition_ms")
        info["ms"] = dict(zip(("place", "scatter", "count", "table"), [round(v, 4) for v in ms]))
        return info

    def clear(self, stream=None):
        """Drop every count but keep the table (a fresh `defaultdict(int)` of the same size)."""
        self._distinct = self._added = 0
        self._partitioned = False
        _capi.check(_capi.lib().covest_kmer_clear(self._handle, ctypes.c_void_p(stream or 0)),
                    "covest_kmer_clear")

    def stats(self):
        """(max count + 1, distinct k-mers): the keys HELD -- with a count of at least 1 (occupancy())."""
        need, distinct = ctypes.c_int64(), ctypes.c_int64()
        _capi.check(_capi.lib().covest_kmer_histogram(self._handle, None, 0, ctypes.byref(need),
                                                      ctypes.byref(distinct)), "covest_kmer_histogram")
        return need.value, distinct.value

    def histogram(self):
        need, _ = self.stats()
        out = np.zeros(need, dtype=np.int64)
        _capi.check(_capi.lib().covest_kmer_histogram(
            self._handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), need, None, None),
            "covest_kmer_histogram")
        return out.tolist()

    def __len__(self):
        return self.stats()[1]


def compute_counts(seq, prev_counts=None, k=20, canonical=False):
    """bin/kmer_hist.py:34-41.  `seq` may also be a list of reads (one launch for all)."""
    counts = KmerCounts(k, canonical=canonical) if prev_counts is None else prev_counts
    counts.add_reads([seq] if isinstance(seq, str) else list(seq))
    return counts


def compute_histogram(counts):
    """bin/kmer_hist.py:57-64: [number of k-mers seen i times for i in 0..max count]."""
    return counts.histogram()


class ReadBatches:
    """load_reads + preprocess (bin/kmer_hist.py:67-74, :44-54) in the library's C++ reader (csrc/reads_io.cpp):
    iterating yields (bases_ptr, offsets_ptr, n_reads, n_bases) batches in the packed layout covest_kmer_add takes
    -- no per-read work in Python.  The pointers are the reader's own buffers, valid until the next batch."""

    def __init__(self, fname, n_strategy=NS_IGNORE, batch_bases=1 << 26, seed=0):
        if n_strategy not in (NS_IGNORE, NS_SINGLE, NS_RANDOM):
            raise ValueError('Invalid N strategy')
        self.batch_bases = int(batch_bases)
        h = ctypes.c_void_p()
        _capi.check(_capi.lib().covest_reads_open(str(fname).encode(), int(n_strategy), int(seed), ctypes.byref(h)),
                    "covest_reads_open")
        self._handle = h

    def close(self):
        if getattr(self, "_handle", None) is not None:
            _capi.lib().covest_reads_close(self._handle)
            self._handle = None

    __del__ = close

    @property
    def bytes_read(self):
        return int(_capi.lib().covest_reads_bytes(self._handle))

    def _next(self):
        """One covest_reads_next call: (bases, offsets, n_reads, n_bases), or an exception instance."""
        L = _capi.lib()
        bases = ctypes.POINTER(ctypes.c_uint8)()
        offsets = ctypes.POINTER(ctypes.c_int64)()
        n = ctypes.c_int64()
        rc = L.covest_reads_next(self._handle, self.batch_bases, ctypes.byref(bases), ctypes.byref(offsets),
                                 ctypes.byref(n))
        if rc != 0:
            msg = _capi.last_error()  # (thread-local in the library: read it on the thread that made the call)
            if rc == _capi.COVEST_E_INVALID and "outside acgtn" in msg:
                return KeyError(msg)  # single_hash raises KeyError (bin/kmer_hist.py:15)
            return _capi.CovestHipError("covest_reads_next failed (%d): %s" % (rc, msg))
        return bases, offsets, n.value, int(offsets[n.value])

    def __iter__(self):
        """Batches in file order.  The reader keeps two batch buffers, so the NEXT batch is parsed on a helper
        thread (the library's own threads do the work; ctypes releases the GIL) while the caller -- the GPU --
        is busy with the one just handed out."""
        import concurrent.futures
        with concurrent.futures.ThreadPoolExecutor(max_workers=1) as pool:
            pending = pool.submit(self._next)
            while True:
                got = pending.result()
                if isinstance(got, Exception):
                    raise got
                if got[2] == 0:
                    return
                pending = pool.submit(self._next)  # fills the OTHER buffer: `got` stays valid until the call after
                yield got


def load_reads(fname, n_strategy=None):
    """Sequences of a FASTA or FASTQ file, one str per record (bin/kmer_hist.py:67-74; the reference delegates the
    parsing to Bio.SeqIO).  With n_strategy they come preprocessed (:44-54).  Kept for callers that want strings:
    `main` feeds the packed batches of ReadBatches to the counter directly."""
    if n_strategy is None:  # the records as they stand (the reader always applies preprocess): parsed here
        _, ext = path.splitext(fname)
        fastq = ext in ('.fq', '.fastq')
        with open(fname) as f:
            if fastq:
                for i, line in enumerate(f):
                    if i % 4 == 1:
                        yield line.strip()
            else:
                chunk, seen = [], False
                for line in f:
                    if line.startswith('>'):
                        if seen:
                            yield ''.join(chunk)
                        chunk, seen = [], True
                    elif seen:
                        chunk.append(''.join(line.split()))
                if seen:
                    yield ''.join(chunk)
        return
    for bases, offsets, n, n_bases in ReadBatches(fname, n_strategy, batch_bases=1 << 24):
        blob = ctypes.string_at(bases, n_bases).decode("ascii")
        for i in range(n):
            yield blob[offsets[i]:offsets[i + 1]]


def main(fname, out_fname, k, n_strategy, canonical=False, batch=1 << 26):
    """bin/kmer_hist.py:77-89.  The file is parsed and preprocessed by the C++ reader, `batch` bases per launch."""
    counts = KmerCounts(k, canonical=canonical)
    for bases, offsets, n, n_bases in ReadBatches(fname, n_strategy, batch_bases=batch):
        counts.add_packed(bases, offsets, n, n_bases)
    hist = compute_histogram(counts)
    if out_fname:
        with open(out_fname, 'w') as f:
            for i, v in enumerate(hist):
                f.write('{} {}\n'.format(i, v))
    else:
        print(hist)
    return hist
