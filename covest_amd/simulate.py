"""Sequencing reads of known coverage and error rate, simulated on the device: the counterpart of the reference's
tools/simulator/generate_sequence.py and tools/simulator/read_simulator.py:60-88.

    genome = random_genome(200_000, seed=1)
    reads = simulate_reads(genome, 100, coverage=20, error_rate=0.02, seed=1)
    counts = reads.add_to(KmerCounts(21, canonical=True))

Where the reference draws from Python's unseeded `random`, every byte here is a stated function of (seed, read index,
base index) through Philox4x32-10 (include/covest_amd.h), so a run is reproducible and any chunk of reads
(`first_read`, `n_reads`) equals the same rows of the whole run.  The genome is a/c/g/t in either case: -s, the IUPAC
substitution of :34-57, is not built.  The output is the layout KmerCounts.add_device and count_reads_device take.
There is no CPU path: without the library or a HIP device every call raises CovestHipError.

A random genome has no repeats; `repeat_genome` builds one whose k-mers have a prescribed copy-number distribution
(DESIGN.md section 6n), and `genome_spectrum` / `spectrum_to_q` measure the truth of the repeat model's (q1, q2, q)
from the genome itself:

    rg = repeat_genome(300_000, 250, q1=0.7, q2=0.5, q=0.5, seed=1)
    reads = simulate_reads(rg.bases, 100, coverage=20, error_rate=0.01, seed=1, both_strands=False)
    q1, q2, q = spectrum_to_q(genome_spectrum(rg, 21))
"""
import ctypes
import math

import numpy as np

from . import _capi

_VALID = np.zeros(256, dtype=bool)
for _ch in "acgtACGT":
    _VALID[ord(_ch)] = True
_COMPLEMENT = np.zeros(256, dtype=np.uint8)
for _a, _b in zip("ACGT", "TGCA"):
    _COMPLEMENT[ord(_a)] = ord(_b)


def _genome_bytes(genome):
    """A genome given as str, bytes or a uint8 array, as a contiguous uint8 array (not validated)."""
    if isinstance(genome, str):
        genome = genome.encode("ascii")
    if isinstance(genome, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(genome), dtype=np.uint8)
    a = np.asarray(genome)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("genome must be a str, bytes or a one-dimensional uint8 array")
    return np.ascontiguousarray(a)


def _check_seed(seed, whole=False):
    """A seed is the 64-bit key of the stream; `whole`: a number that is no integer is refused too, not truncated."""
    if (whole and int(seed) != seed) or not (0 <= seed < 1 << 64):
        raise ValueError("seed must fit 64 bits")


def _check_first_read(first_read):
    """The index of a call's first read, as an int: a whole number, not negative."""
    if int(first_read) != first_read or first_read < 0:
        raise ValueError("first_read must not be negative")
    return int(first_read)


def _check(read_length, genome_len, n_reads, first_read, error_rate, seed):
    """The argument rules of covest_simulate_reads, before the library is asked (ValueError, as the models' arguments)."""
    if int(read_length) != read_length or read_length < 1:
        raise ValueError("read_length must be a positive integer")
    if genome_len <= read_length:  # randrange(genome_size - read_length) of an empty range (read_simulator.py:75)
        raise ValueError("the genome must be longer than a read")
    if n_reads < 0 or first_read < 0:
        raise ValueError("n_reads and first_read must not be negative")
    if not (0.0 <= error_rate <= 1.0):  # (NaN fails both)
        raise ValueError("error_rate must be in [0, 1]")
    _check_seed(seed)


def _n_reads(coverage, genome_len, read_length, n_reads):
    if n_reads is not None:
        return int(n_reads)
    if coverage is None:
        raise ValueError("give coverage or n_reads")
    if not (coverage >= 0 and math.isfinite(coverage)):
        raise ValueError("coverage must be a finite number, not negative")
    return int(round((coverage * genome_len) / float(read_length)))  # read_simulator.py:72


def random_genome(n, seed, device=-1):
    """`n` random bases (upper-case ASCII, a uint8 array): generate_sequence.py, seeded."""
    n, seed = int(n), int(seed)
    if n < 0:
        raise ValueError("n must not be negative")
    _check_seed(seed)
    out = np.empty(n, dtype=np.uint8)
    _capi.check(_capi.lib().covest_random_genome(int(device), n, seed, out.ctypes.data), "covest_random_genome")
    return out


def random_genome_device(ptr, n, seed, stream=None, device=-1):
    """The same into `n` bytes of device memory at `ptr` (a raw pointer, e.g. a torch tensor's data_ptr());
    asynchronous on `stream`."""
    _capi.require_shared_runtime("random_genome_device")
    _capi.check(_capi.lib().covest_random_genome_device(int(device), int(n), int(seed), ctypes.c_void_p(ptr),
                                                        ctypes.c_void_p(stream or 0)), "covest_random_genome_device")


def simulate_reads_device(genome_ptr, genome_len, read_length, n_reads, bases_ptr, error_rate=0.0, seed=0, first_read=0,
                          both_strands=True, origin_ptr=None, stream=None, device=-1):
    """Reads [first_read, first_read + n_reads) into n_reads * read_length bytes of device memory at `bases_ptr` from a
    genome resident at `genome_ptr` (raw device pointers); `origin_ptr`: n_reads int64 records pos << 1 | forward.
    Asynchronous on `stream`.  The genome's bytes are not validated here (any byte is taken for some base)."""
    _check(read_length, int(genome_len), int(n_reads), int(first_read), float(error_rate), int(seed))
    _capi.require_shared_runtime("simulate_reads_device")
    _capi.check(_capi.lib().covest_simulate_reads_device(
        int(device), ctypes.c_void_p(genome_ptr), int(genome_len), int(read_length), int(first_read), int(n_reads),
        float(error_rate), int(seed), 1 if both_strands else 0, ctypes.c_void_p(bases_ptr),
        ctypes.c_void_p(origin_ptr or 0), ctypes.c_void_p(stream or 0)), "covest_simulate_reads_device")


class SimulatedReads:
    """What simulate_reads returns: `bases` (n, L) uint8 upper-case ASCII, `positions` (n,) int64 starts in the genome,
    `forward` (n,) bool (False: the read is the reverse complement of the slice), and the settings that made them."""

    def __init__(self, bases, origin, genome_len, error_rate, seed, first_read):
        self.bases = bases
        self.positions = origin >> 1
        self.forward = (origin & 1).astype(bool)
        self.genome_len = int(genome_len)
        self.error_rate = float(error_rate)
        self.seed = int(seed)
        self.first_read = int(first_read)

    @property
    def n_reads(self):
        return self.bases.shape[0]

    @property
    def read_length(self):
        return self.bases.shape[1]

    @property
    def true_coverage(self):
        """Bases read per base of the genome: n_reads * read_length / genome_len (the `coverage` asked for, after the
        rounding of the read count, read_simulator.py:72)."""
        return self.n_reads * self.read_length / self.genome_len

    def error_free(self, genome):
        """The reads before their substitutions (the reference's -f output, :83-85): the slices of `genome` at
        `positions`, reverse-complemented where `forward` is False.  Host arithmetic."""
        g = _genome_bytes(genome) & 0xDF  # upper case
        twin = g[self.positions[:, None] + np.arange(self.read_length)[None, :]]
        back = ~self.forward
        twin[back] = _COMPLEMENT[twin[back][:, ::-1]]
        return twin

    def substitutions(self, genome):
        """The realised number of substituted bases (host arithmetic)."""
        return int(np.count_nonzero(self.bases != self.error_free(genome)))

    def write_fasta(self, path, genome_id="simulated"):
        """The reference's output file: '>read_{id}_{i}-{pos}' and the read (read_simulator.py:81-82)."""
        with open(path, "w") as f:
            for i in range(self.n_reads):
                f.write(">read_%s_%d-%d\n" % (genome_id, self.first_read + i, self.positions[i]))
                f.write(self.bases[i].tobytes().decode("ascii"))
                f.write("\n")

    def add_to(self, counts):
        """Count the reads' k-mers into a KmerCounts (kmer_hist.py); returns it."""
        n, L = self.bases.shape
        if n:
            offsets = np.arange(n + 1, dtype=np.int64) * L
            blob = np.ascontiguousarray(self.bases).reshape(-1)
            counts.add_packed(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                              offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, n * L)
        return counts


def simulate_reads(genome, read_length, coverage=None, error_rate=0.0, seed=0, n_reads=None, first_read=0,
                   both_strands=True, device=-1):
    """`n_reads` reads (default: int(round(coverage * len(genome) / read_length)), read_simulator.py:72) of
    `read_length` bases from uniformly drawn places of `genome` (str, bytes or uint8 array of a/c/g/t in either case),
    from either strand unless both_strands is False, each base substituted with probability `error_rate` by one of the
    other three.  Reads are numbered from `first_read`: a chunk equals the same rows of the whole run."""
    g = _genome_bytes(genome)
    seed, first_read, error_rate = int(seed), int(first_read), float(error_rate)
    _check(read_length, g.size, 0, first_read, error_rate, seed)
    read_length = int(read_length)
    n = _n_reads(coverage, g.size, read_length, n_reads)
    if n < 0:
        raise ValueError("n_reads and first_read must not be negative")
    if g.size and not _VALID[g].all():
        raise ValueError("genome byte outside acgtACGT")
    bases = np.empty((n, read_length), dtype=np.uint8)
    origin = np.empty(n, dtype=np.int64)
    _capi.check(_capi.lib().covest_simulate_reads(
        int(device), g.ctypes.data, g.size, read_length, first_read, n, error_rate, seed, 1 if both_strands else 0,
        bases.ctypes.data, origin.ctypes.data), "covest_simulate_reads")
    return SimulatedReads(bases, origin, g.size, error_rate, seed, first_read)


# ---- repeat-bearing genomes ---------------------------------------------------------------------
MAX_COPIES_LIMIT = 1 << 20


def _check_plan_args(n_units, q1, q2, q, seed, max_copies):
    """The argument rules of covest_repeat_plan, before the library is asked."""
    if int(n_units) != n_units or n_units < 0:
        raise ValueError("n_units must be an integer, not negative")
    for name, v in (("q1", q1), ("q2", q2), ("q", q)):
        if not (0.0 <= v <= 1.0):  # (NaN fails both)
            raise ValueError("%s must be in [0, 1]" % name)
    if int(max_copies) != max_copies or not (1 <= max_copies <= MAX_COPIES_LIMIT):
        raise ValueError("max_copies must be in 1 .. 2^20")
    _check_seed(seed)


def _check_genome_args(n, unit_len, n_units, divergence, seed):
    """The argument rules of covest_repeat_genome, before the library is asked."""
    if int(unit_len) != unit_len or not (1 <= unit_len < 1 << 31):
        raise ValueError("unit_len must be a positive integer that fits 31 bits")
    if int(n) != n or n < 0:
        raise ValueError("n must be an integer, not negative")
    if n_units < 0 or n > n_units * int(unit_len):
        raise ValueError("n is more than n_units * unit_len")
    if not (0.0 <= divergence <= 1.0):
        raise ValueError("divergence must be in [0, 1]")
    _check_seed(seed)


def repeat_plan(n_units, q1, q2, q, seed, max_copies=64, both_orientations=True):
    """(plan, n_families): which family each of `n_units` units copies and which way round, `plan[u] = family << 1 |
    forward` (int64).  Family f has o copies with the repeat model's probability b_o(q1, q2, q) (o = max_copies takes
    the rest); the units are shuffled, and reverse-complemented at random unless both_orientations is False.  Host
    arithmetic of the library (covest_repeat_plan): needs no device."""
    q1, q2, q, seed = float(q1), float(q2), float(q), int(seed)
    _check_plan_args(n_units, q1, q2, q, seed, max_copies)
    n_units = int(n_units)
    plan = np.empty(n_units, dtype=np.int64)
    n_families = ctypes.c_int64(0)
    _capi.check(_capi.lib().covest_repeat_plan(n_units, q1, q2, q, int(max_copies), seed, 1 if both_orientations else 0,
                                               plan.ctypes.data, ctypes.byref(n_families)), "covest_repeat_plan")
    return plan, int(n_families.value)


class RepeatGenome:
    """What repeat_genome returns: `bases` (n,) uint8 upper-case ASCII (simulate_reads takes it as it is), `plan`
    (n_units,) int64 = family << 1 | forward, `unit_len`, `family_of_unit`, `forward`, and the settings that made it."""

    def __init__(self, bases, plan, unit_len, divergence, seed):
        self.bases = bases
        self.plan = plan
        self.unit_len = int(unit_len)
        self.family_of_unit = plan >> 1
        self.forward = (plan & 1).astype(bool)
        self.divergence = float(divergence)
        self.seed = int(seed)

    def __len__(self):
        return self.bases.size

    @property
    def n_units(self):
        """Units the genome holds (the last may be cut): ceil(n / unit_len)."""
        return -(-self.bases.size // self.unit_len)

    def copies(self):
        """{family id: copies of it among the genome's units} -- the copy numbers realised in the plan."""
        ids, counts = np.unique(self.family_of_unit[:self.n_units], return_counts=True)
        return dict(zip(ids.tolist(), counts.tolist()))


def repeat_genome_device(plan_ptr, n_units, unit_len, n, out_ptr, divergence=0.0, seed=0, stream=None, device=-1):
    """`n` bases into device memory at `out_ptr` (any alignment) from a plan of `n_units` int64 entries resident at
    `plan_ptr` (raw device pointers); asynchronous on `stream`.  The plan is not looked at here: its entries must not be
    negative, and (family + 1) * unit_len must fit 63 bits."""
    _check_genome_args(n, unit_len, int(n_units), float(divergence), int(seed))
    _capi.require_shared_runtime("repeat_genome_device")
    _capi.check(_capi.lib().covest_repeat_genome_device(
        int(device), ctypes.c_void_p(plan_ptr), int(n_units), int(unit_len), int(n), float(divergence), int(seed),
        ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)), "covest_repeat_genome_device")


def repeat_genome(n, unit_len, q1=None, q2=None, q=None, seed=0, divergence=0.0, max_copies=64, both_orientations=True,
                  plan=None, device=-1):
    """A genome of `n` bases made of units of `unit_len` bases, each a copy of a family (forward or
    reverse-complemented) with every base then substituted with probability `divergence`.  The plan is
    repeat_plan(ceil(n / unit_len), q1, q2, q, seed, max_copies, both_orientations) unless `plan` is given (an int64
    array of family << 1 | forward, at least ceil(n / unit_len) entries: a tandem array, one family everywhere, ...);
    then q1, q2 and q are not used."""
    seed, divergence = int(seed), float(divergence)
    if plan is None:
        if int(unit_len) != unit_len or unit_len < 1 or int(n) != n or n < 0:
            raise ValueError("n must be a non-negative and unit_len a positive integer")
        if q1 is None or q2 is None or q is None:
            raise ValueError("give q1, q2 and q, or a plan")
        _check_plan_args(-(-int(n) // int(unit_len)), float(q1), float(q2), float(q), seed, max_copies)
        _check_genome_args(n, unit_len, -(-int(n) // int(unit_len)), divergence, seed)
        plan, _ = repeat_plan(-(-int(n) // int(unit_len)), q1, q2, q, seed, max_copies, both_orientations)
    else:
        plan = np.ascontiguousarray(np.asarray(plan), dtype=np.int64)
        if plan.ndim != 1:
            raise ValueError("plan must be one-dimensional")
        _check_genome_args(n, unit_len, plan.size, divergence, seed)
        if plan.size and int(plan.min()) < 0:
            raise ValueError("negative plan entry")
        if plan.size and (int(plan.max()) >> 1) > ((1 << 63) - 1) // int(unit_len) - 1:
            raise ValueError("family id times unit_len leaves 63 bits")
    n, unit_len = int(n), int(unit_len)
    out = np.empty(n, dtype=np.uint8)
    _capi.check(_capi.lib().covest_repeat_genome(int(device), plan.ctypes.data, plan.size, unit_len, n, divergence, seed,
                                                 out.ctypes.data), "covest_repeat_genome")
    return RepeatGenome(out, plan, unit_len, divergence, seed)


_SPECTRUM_WINDOW = 1 << 16  # k-mer starts a window of genome_spectrum holds


def genome_spectrum(genome, k, canonical=False, device=-1):
    """The genome's own copy-number spectrum {o: distinct k-mers occurring o times} (a k-mer and its reverse complement
    taken together if `canonical`), counted on the device with KmerCounts.  The genome (a RepeatGenome, str, bytes or
    uint8 array of a/c/g/t) is handed over as overlapping windows of up to 65 536 + k - 1 bases, a window a read, so
    every k-mer start falls in exactly one window."""
    g, k = _spectrum_genome(genome, k)
    if g.size - k + 1 <= 0:
        return {}
    counts = genome_counts(g, k, canonical=canonical, device=device)
    try:
        hist = counts.histogram()
    finally:
        counts.close()
    return {o: int(v) for o, v in enumerate(hist) if o > 0 and v > 0}


def _spectrum_genome(genome, k):
    g = genome.bases if isinstance(genome, RepeatGenome) else _genome_bytes(genome)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    if g.size and not _VALID[g].all():
        raise ValueError("genome byte outside acgtACGT")
    return g, k


def genome_counts(genome, k, canonical=False, device=-1):
    """The table genome_spectrum counts and closes, left open: a KmerCounts that holds every k-mer of the genome with
    the number of its copies -- the other side of KmerCounts.join_histogram and of covest_amd.copy_spectrum.  The same
    overlapping windows of up to 65 536 + k - 1 bases, a window a read; a genome shorter than k gives an empty counter.
    The caller closes it."""
    from .kmer_hist import KmerCounts
    g, k = _spectrum_genome(genome, k)
    counts = KmerCounts(k, canonical=canonical, device=device)
    n_starts = g.size - k + 1
    if n_starts <= 0:
        return counts
    starts = np.arange(0, n_starts, _SPECTRUM_WINDOW, dtype=np.int64)
    lens = np.minimum(_SPECTRUM_WINDOW, n_starts - starts) + (k - 1)  # every window holds a k-mer
    offsets = np.zeros(starts.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    blob = np.concatenate([g[a:a + m] for a, m in zip(starts.tolist(), lens.tolist())])
    try:
        counts.add_packed(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                          offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), starts.size, blob.size)
    except Exception:
        counts.close()
        raise
    return counts


def spectrum_to_q(spectrum):
    """(q1, q2, q) of the repeat model that a copy-number spectrum {o: N_o} realises: q1 = N_1 / N, q2 = N_2 /
    (N - N_1), q = N_{>=3} / sum_{o>=3} (o - 2) N_o -- the maximum-likelihood rate of the geometric tail b_o ~
    q (1 - q)^(o - 3).  A component whose denominator is 0 is None."""
    total = one = two = more = weight = 0
    for o, v in spectrum.items():
        o, v = int(o), int(v)
        if o < 1 or v < 0:
            raise ValueError("a spectrum maps copy numbers >= 1 to counts >= 0")
        total += v
        if o == 1:
            one += v
        elif o == 2:
            two += v
        else:
            more += v
            weight += (o - 2) * v
    return (one / total if total else None, two / (total - one) if total - one else None,
            more / weight if weight else None)
