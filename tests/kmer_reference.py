"""A second, independent restatement of the k-mer histogram (bin/kmer_hist.py of the reference), and the inputs
the width tests count.  TEST INFRASTRUCTURE ONLY.

It shares no code with oracle/kmer_oracle.py and works another way: no shifting and masking, but string slices and
Python integers, so it holds for any k.
  * a read is translated to base-4 digits (a=0 c=1 g=2 t=3, either case);
  * a window's key is int(digits[s:s+k], 4); a read shorter than k gives the value of what there is, 0 if empty;
  * canonical: the smaller of that and the same slice of the reversed, complemented digit string.  For a read
    shorter than k the reverse complement is taken over k positions of the zero-extended code (the absent leading
    digits are 0 = 'a', their complement 3 = 't' ends up in the LOW digits) -- what the oracle and the kernels do.
Windows are tallied as digit strings first and converted once per distinct string: the reads of the tests come from
a small genome, so that is a few thousand conversions a call.

tests/test_kmer_reference_cpu.py holds it against the oracle and against the reference's own golden vectors;
tests/test_gpu_kmer_widths.py holds the device against it.
"""
import functools
import random
from collections import Counter

NS_IGNORE, NS_SINGLE = 0, 1

_DIGITS = str.maketrans("acgtACGT", "01230123")
_COMPLEMENT = str.maketrans("0123", "3210")
_COMPLEMENT_BASES = str.maketrans("acgtACGT", "tgcaTGCA")


def preprocess(seq, nstrategy=NS_IGNORE):
    """bin/kmer_hist.py:44-54 without the random strategy."""
    seq = seq.lower()
    if nstrategy == NS_IGNORE:
        return seq.replace("n", "")
    if nstrategy == NS_SINGLE:
        return seq.replace("n", "a")
    raise ValueError("Invalid N strategy")


def _digits(read):
    d = read.translate(_DIGITS)
    if d.strip("0123"):
        raise KeyError("base outside acgt")
    return d


def _key(window, k, canonical):
    """The key of a digit string of at most k digits."""
    key = int(window, 4) if window else 0
    if canonical:
        key = min(key, int(window[::-1].translate(_COMPLEMENT) + "3" * (k - len(window)), 4))
    return key


def count(reads, k, canonical=False):
    """{key: occurrences} over all windows of all (preprocessed) reads."""
    windows = Counter()
    for read in reads:
        d = _digits(read)
        if len(d) < k:
            windows[d] += 1
        else:
            windows.update(d[s:s + k] for s in range(len(d) - k + 1))
    keys = Counter()
    for window, n in windows.items():  # (different strings can be one key: strands, short reads)
        keys[_key(window, k, canonical)] += n
    return keys


def histogram(reads, k, canonical=False):
    """(count-of-counts list indexed 0 .. max count -- [0] when nothing was counted --, distinct keys)."""
    keys = count(reads, k, canonical)
    if not keys:
        return [0], 0
    per_count = Counter(keys.values())
    return [per_count.get(i, 0) for i in range(max(per_count) + 1)], len(keys)


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of tests/test_gpu_kmer_widths.py.  Every builder is a pure function of its arguments (seeded generators),
# so the CPU test, the GPU tests and the GPU tests' child process all see the same reads.

GENOME_LEN = 3000


def revcomp(read):
    return read[::-1].translate(_COMPLEMENT_BASES)


def _random_bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def genome(max_run=None):
    """3 000 random bases; with `max_run`, no base repeats more than that many times in a row."""
    rng = random.Random(20240917)
    g = list(_random_bases(rng, GENOME_LEN))
    if max_run:
        for i in range(max_run, len(g)):
            if all(g[j] == g[i] for j in range(i - max_run, i)):
                g[i] = "ACGT"[("ACGT".index(g[i]) + 1 + rng.randrange(3)) % 4]
    return "".join(g)


def genome_reads(rng, n, length, max_run=None):
    g = genome(max_run)
    return [g[s:s + length] for s in (rng.randrange(len(g) - length + 1) for _ in range(n))]


def sweep_lengths(k):
    return [0, 1, k - 1, k, k + 1, k + 2, k + 3, k + 4, k + 62, k + 63, k + 64, k + 65, k + 127, k + 128, k + 129,
            2 * k + 200]


@functools.lru_cache(maxsize=None)
def sweep_reads(k):
    """(a): six reads of each of sweep_lengths(k) from the genome (duplicates and overlaps are wanted), the reverse
    complement of every third, half of them lower-cased, shuffled so that every batch holds every length."""
    rng = random.Random(1000 + k)
    reads = [r for length in sweep_lengths(k) for r in genome_reads(rng, 6, length)]
    reads += [revcomp(r) for r in reads[::3]]
    rng.shuffle(reads)
    return tuple(r.lower() if i % 2 else r for i, r in enumerate(reads))


def sweep_batches(k):
    """The three batches of (a): a sixth, a third and a half of the reads -- the later ones meet a table that holds
    keys already and has to grow with them in it."""
    reads = sweep_reads(k)
    a, b = len(reads) // 6, len(reads) // 2
    return [list(reads[:a]), list(reads[a:b]), list(reads[b:])]


def probe_positions(k):
    """(b): the ends of the k-mer and both sides of every 32-base (one 64-bit word) boundary, as indices into the
    k-mer AND mirrored (k - 1 - p): base p sits 2(k - 1 - p) bits up in the forward code and 2p bits up in the
    reverse complement's, so both have to straddle the words."""
    ps = {0, 1, k - 2, k - 1}
    for m in range(1, k // 32 + 2):
        ps.update((32 * m - 1, 32 * m, 32 * m + 1))
    ps = {p for p in ps if 0 <= p < k}
    return sorted(ps | {k - 1 - p for p in ps})


PALINDROME_K = (2, 4, 32, 64, 128, 254)


@functools.lru_cache(maxsize=None)
def probe_reads(k):
    """(b): per position p a random k-mer B and B' = B with base p replaced, each as a read of k bases, as the last
    window behind a random 67-base prefix and as the first window before a random 67-base suffix.  For the k of
    PALINDROME_K also a reverse-palindromic k-mer and a pair B, revcomp(B) as separate reads."""
    rng = random.Random(5000 + k)
    reads = []
    for p in probe_positions(k):
        b = _random_bases(rng, k)
        other = "ACGT"[("ACGT".index(b[p]) + 1 + rng.randrange(3)) % 4]
        for kmer in (b, b[:p] + other + b[p + 1:]):
            reads += [kmer, _random_bases(rng, 67) + kmer, kmer + _random_bases(rng, 67)]
    if k in PALINDROME_K:
        half = _random_bases(rng, k // 2)
        b = _random_bases(rng, k)
        reads += [half + revcomp(half), b, revcomp(b)]
    return tuple(reads)


LANES_K = (31, 32, 63, 64, 127, 128, 255)


@functools.lru_cache(maxsize=None)
def lanes_reads(k):
    """(c): reads whose windows are all one key (poly-A, poly-T; canonical: the same key) or two (AC repeats) --
    every lane of a wave inserts the same new key at once -- beside ten genome reads."""
    rng = random.Random(7000 + k)
    return tuple(["A" * (k + 200), "AC" * (k // 2 + 110), "T" * (k + 70)] + genome_reads(rng, 10, k + 40))


BINS_K = (5, 40, 130)
BINS_COUNTS = (4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def bins_reads(k):
    """(d): three keys counted 4095, 4096 and 4097 times (both sides of the histogram kernel's 4096 LDS bins), and
    200 genome reads of k + 40 bases.  The genome is the one without runs of more than four equal bases, so that at
    k = 5 no genome read holds one of the three keys."""
    rng = random.Random(9000 + k)
    reads = [base * (k + n - 1) for base, n in zip("ACG", BINS_COUNTS)]
    return tuple(reads + genome_reads(rng, 200, k + 40, max_run=4))


DEVICE_K = (12, 13, 31, 32, 63, 64, 127, 128, 255)


def device_lengths(k):
    return [k, k + 1, k + 64, k + 129]


def device_fixed_reads(k, length):
    """(e): 300 reads of one length."""
    return genome_reads(random.Random(11000 + 1000 * k + length), 300, length)


def device_ragged_reads(k):
    """(e): 300 reads of 0 .. k + 130 bases, an empty one and one of k - 1 bases among them."""
    rng = random.Random(13000 + k)
    reads = [genome_reads(rng, 1, rng.randrange(k + 131))[0] for _ in range(298)]
    reads.insert(100, "")
    reads.insert(200, genome_reads(rng, 1, k - 1)[0])
    return reads


FILE_K = (40, 150)
FASTA_LINE = 60


def fasta_records():
    """(f): records of a FASTA file as (header, sequence with Ns): long ones with single Ns and runs of them, a
    repeated one, one with lower-case bases, one of Ns only, one shorter than either k of FILE_K."""
    rng = random.Random(15000)
    records = []
    for i, length in enumerate((400, 397, 241, 640, 30, 152)):
        seq = list(genome_reads(rng, 1, length)[0])
        for _ in range(length // 80):
            at = rng.randrange(length)
            seq[at:at + rng.choice((1, 1, 3))] = "N" * rng.choice((1, 1, 2))
        records.append(("r%d" % i, "".join(seq)))
    records.append(("again", records[0][1]))
    records.append(("lower", records[3][1].lower()))
    records.append(("only_n", "N" * 70))
    return records


def fasta_text():
    lines = []
    for name, seq in fasta_records():
        lines.append(">" + name)
        lines += [seq[i:i + FASTA_LINE] for i in range(0, len(seq), FASTA_LINE)]
    return "\n".join(lines) + "\n"
