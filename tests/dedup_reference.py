"""The duplicate remover restated in numpy (not collected): the fingerprint of csrc/read_fingerprint.h with uint64
arrays, and the rule of include/covest_amd.h (section "duplicate reads removed") as a plain loop.  Every comparison
against it is exact.  `dictionary` is the independent oracle: the first read of every class of equal reads, by a dict of
byte strings -- what the rule gives where no two different reads share a key."""
import numpy as np

M64 = (1 << 64) - 1
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ((b"a", b"t"), (b"c", b"g"), (b"A", b"T"), (b"C", b"G")):
    _COMP[_a[0]], _COMP[_b[0]] = _b[0], _a[0]


def mix64(z):
    """The finaliser of SplitMix64 on a uint64 array (or scalar)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def salt_of(seed):
    return int(mix64(np.uint64((seed + 0x9E3779B97F4A7C15) & M64)))


def revcomp(read):
    """The reverse complement of a read (bytes or uint8 array), as a uint8 array."""
    return _COMP[np.frombuffer(bytes(read), dtype=np.uint8)][::-1].copy()


def F(read, seed):
    """F(x) = mix64(mix64(S(x) + seed) + len(x)), S(x) = sum over j of mix64(salt + 256 j + x[j]) mod 2^64."""
    x = np.frombuffer(bytes(read), dtype=np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        terms = mix64(np.uint64(salt_of(seed)) + np.uint64(256) * np.arange(x.size, dtype=np.uint64) + x)
        s = int(terms.sum(dtype=np.uint64)) if x.size else 0
    inner = int(mix64(np.uint64((s + seed) & M64)))
    return int(mix64(np.uint64((inner + x.size) & M64)))


def key(read, seed=0, reverse_complement=False, fp_bits=63):
    f = F(read, seed)
    if reverse_complement:
        f = min(f, F(revcomp(read), seed))
    return f & ((1 << fp_bits) - 1)


def equal(x, y, reverse_complement=False):
    x, y = bytes(x), bytes(y)
    return x == y or (bool(reverse_complement) and x == bytes(revcomp(y)))


def split(bases, offsets=None):
    """The reads as a list of byte strings: an (n, L) array, or (bases, offsets)."""
    if offsets is None:
        return [bytes(r) for r in np.asarray(bases, dtype=np.uint8)]
    blob = np.asarray(bases, dtype=np.uint8).tobytes()
    return [blob[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def dedup(reads, fp_bits=63, seed=0, reverse_complement=False):
    """The rule as a plain loop over a list of byte strings: (kept: indices, copies of the kept, collided)."""
    rep = {}
    keys = [key(r, seed, reverse_complement, fp_bits) for r in reads]
    for i, k in enumerate(keys):
        rep.setdefault(k, i)           # the lowest index of every key
    kept, dropped_on, collided = [], [0] * len(reads), 0
    for i, k in enumerate(keys):
        m = rep[k]
        if m == i:
            kept.append(i)
        elif not equal(reads[i], reads[m], reverse_complement):
            kept.append(i)
            collided += 1
        else:
            dropped_on[m] += 1
    return (np.array(kept, dtype=np.int64), np.array([1 + dropped_on[i] for i in kept], dtype=np.int32), collided)


def dictionary(reads, reverse_complement=False):
    """(kept, copies) with one read of every class of equal reads, the first of each: a dict of byte strings, of the
    smaller of a read and its reverse complement where those are equal too."""
    first, count = {}, {}
    for i, r in enumerate(reads):
        r = bytes(r)
        c = min(r, bytes(revcomp(r))) if reverse_complement else r
        first.setdefault(c, i)
        count[c] = count.get(c, 0) + 1
    order = sorted(first.items(), key=lambda item: item[1])
    return (np.array([i for _, i in order], dtype=np.int64), np.array([count[c] for c, _ in order], dtype=np.int32))


def pack(reads):
    """(bases, offsets) of a list of byte strings."""
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    return np.frombuffer(b"".join(bytes(r) for r in reads), dtype=np.uint8).copy(), offsets


# ---- the shapes the tests share ------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"acgt", dtype=np.uint8)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1023, 1024, 1031)  # (256, 1024: the load width changes)


def random_reads(n, length, seed, alphabet=ACGT):
    rng = np.random.default_rng(seed)
    return [bytes(r) for r in rng.choice(alphabet, size=(n, length))]


def with_copies(n, length, share, seed, rc_copies=False):
    """n reads of `length` bases of which `share` are copies of other reads, anywhere; the first read is copied at the
    last index.  rc_copies: every other copy is the reverse complement of its original."""
    rng = np.random.default_rng(seed)
    n_orig = n - int(round(n * share))
    orig = random_reads(n_orig, length, seed + 1)
    reads = orig + [orig[i] for i in rng.integers(0, n_orig, size=n - n_orig - 1)]
    if rc_copies:
        reads[n_orig::2] = [bytes(revcomp(r)) for r in reads[n_orig::2]]
    tail = [reads[i] for i in rng.permutation(np.arange(1, len(reads)))]
    return [reads[0]] + tail + [reads[0]]


def ragged(seed, per_length=6, alphabet=ACGT):
    """Reads of every length of LENGTHS in one blob, shuffled, each length with a copy of one of its reads: the odd
    lengths put the reads' starts at every byte alignment mod 16."""
    rng = np.random.default_rng(seed)
    reads = []
    for length in LENGTHS:
        group = random_reads(per_length, length, seed + length, alphabet)
        reads += group + [group[0]]
    return [reads[i] for i in rng.permutation(len(reads))]
