"""The read simulator's random stream restated in numpy (TEST INFRASTRUCTURE ONLY; not collected).

Written from the definition in include/covest_amd.h / DESIGN.md section 6l, not from the kernel:
  Philox4x32-10 (Random123): M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85; a round takes
  (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then k0 += W0, k1 += W1;
  key = (seed & 0xffffffff, seed >> 32).
  genome base i: counter (lo32(i>>2), hi32(i>>2), 0, 1), word i & 3, "ACGT"[word >> 30].
  read r: header counter (lo32(r), hi32(r), 0, 0) -> w0..w3; pos = mulhi64(w0 | w1 << 32, genome_len - read_len);
          forward if w2 & 1 or both_strands is off, else the reverse complement.
  base i of the read as oriented: counter (lo32(r), hi32(r), 1 + (i >> 2), 0), w = word i & 3; substituted iff
          w < floor(error_rate * 2^32) by the base of code (code + 1 + w % 3) & 3 with A, C, G, T = 0, 1, 2, 3.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.zeros(256, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (broadcast against each other): four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m0, m1, mask, s32 = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_scalar(counter, key):
    """One block, plain Python integers: ((c0, c1, c2, c3), (k0, k1)) -> four words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed)
    return seed & MASK, seed >> 32


def split64(x):
    """(lo32, hi32) of 64-bit indices (Python integers, a list of them or an array): two uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64)
    return x & np.uint64(MASK), x >> np.uint64(32)


def _words(blocks, word):
    """Pick out[word] per element from the four arrays of philox()."""
    return np.choose(np.asarray(word, dtype=np.intp), blocks)


def random_genome(n, seed):
    i = np.arange(int(n), dtype=np.uint64)
    out = philox(*split64(i >> np.uint64(2)), 0, 1, *_key(seed))
    w = _words(out, (i & np.uint64(3)))
    return ACGT[(w >> np.uint64(30)).astype(np.intp)]


def headers(genome_len, read_len, first_read, n_reads, seed, both_strands=True):
    """(pos, forward) of reads first_read .. first_read + n_reads: int64 and bool arrays."""
    r = [int(first_read) + i for i in range(int(n_reads))]
    lo, hi = split64(r)
    w0, w1, w2, _ = philox(lo, hi, 0, 0, *_key(seed))
    span = int(genome_len) - int(read_len)
    pos = np.array([((int(a) | (int(b) << 32)) * span) >> 64 for a, b in zip(w0, w1)], dtype=np.int64)
    forward = (w2 & np.uint64(1)).astype(bool) if both_strands else np.ones(len(r), dtype=bool)
    return pos, forward, lo, hi


def simulate(genome, read_len, first_read, n_reads, error_rate, seed, both_strands=True):
    """(bases (n, L) uint8 upper-case ASCII, origin (n,) int64 = pos << 1 | forward)."""
    g = np.frombuffer(genome.encode() if isinstance(genome, str) else bytes(genome), dtype=np.uint8)
    n, L = int(n_reads), int(read_len)
    pos, forward, lo, hi = headers(g.size, L, first_read, n, seed, both_strands)
    i = np.arange(L)
    code = _CODE[g[pos[:, None] + i[None, :]]].astype(np.int64)                    # the forward slices
    code = np.where(forward[:, None], code, 3 - code[:, ::-1])                      # ... as oriented
    out = philox(lo[:, None], hi[:, None], (1 + (i >> 2))[None, :], 0, *_key(seed))
    w = _words(out, np.broadcast_to((i & 3)[None, :], (n, L)))
    thr = int(np.floor(float(error_rate) * 2.0 ** 32))
    hit = w < np.uint64(thr)
    sub = (code + 1 + (w % np.uint64(3)).astype(np.int64)) & 3
    code = np.where(hit, sub, code)
    origin = (pos << 1) | forward.astype(np.int64)
    return ACGT[code], origin, hit, (w % np.uint64(3)).astype(np.int64)


def reads_and_origin(genome, read_len, first_read, n_reads, error_rate, seed, both_strands=True):
    bases, origin, _, _ = simulate(genome, read_len, first_read, n_reads, error_rate, seed, both_strands)
    return bases, origin
