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
    if not (0 <= seed < 1 << 64):
        raise ValueError("seed must fit 64 bits")


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
    if not (0 <= seed < 1 << 64):
        raise ValueError("seed must fit 64 bits")
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
