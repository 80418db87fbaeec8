"""The read sampler on the device (sample_reads.hip through covest_amd.sample and the C ABI) against its numpy
restatement (tests/sample_reference.py): kept reads, offsets and indices equal bit for bit, whatever the read lengths,
the number of reads, the alignment of either buffer, the factor or the chunk of the run; nothing written outside the
stated ranges; the sample counted without leaving HBM; the file loop independent of its batch size; and one whole
estimate from a sampled read set held against the sample's own truth.

Host forms run in this process (numpy buffers).  What needs device buffers of a chosen alignment runs in ONE fresh child
process with torch imported first (one HIP runtime a process), as tests/test_gpu_simulate.py does.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_reference as kr
import sample_reference as ref

pytestmark = pytest.mark.gpu

SEED = (0x5a3d << 32) | 0x0badcafe   # both key words in use
LENGTHS = (0, 1, 2, 5, 16, 17, 100, 4095, 4096, 4097, 10000)


def ragged(n, seed=20241018):
    """(bases, offsets) of n reads whose lengths are drawn from LENGTHS at a fixed numpy seed."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(LENGTHS, size=n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(offsets[-1])), offsets


def pick_seed(n, factor, want):
    """The first seed for which the restatement's mask of n reads satisfies `want`."""
    for seed in range(1, 4000):
        if want(ref.keep_mask(0, n, factor, seed)):
            return seed
    raise AssertionError("no seed found")


def check_host(bases, offsets, factor, seed, first_read=0):
    """sample_reads on a pair against the restatement; returns the SampledReads."""
    from covest_amd import sample
    got = sample.sample_reads((bases, offsets), factor, seed=seed, first_read=first_read)
    want = ref.sample(bases, offsets, first_read, factor, seed)
    assert np.array_equal(got.bases, want[0]) and np.array_equal(got.offsets, want[1]) and np.array_equal(got.kept, want[2])
    assert got.n_reads == want[2].size and got.n_bases == want[0].size
    return got


@pytest.mark.parametrize("factor", [1, 2, 16])
def test_variable_lengths(hip_lib, factor):
    bases, offsets = ragged(600)
    got = check_host(bases, offsets, factor, SEED)
    if factor == 1:  # everything kept: the output is the input, offsets included
        assert np.array_equal(got.bases, bases) and np.array_equal(got.offsets, offsets)
        assert np.array_equal(got.kept, np.arange(600))


def test_runs_of_empty_reads_and_ends(hip_lib):
    rng = np.random.default_rng(1)
    lens = np.concatenate([rng.choice([3, 100], size=40), np.zeros(1000, dtype=np.int64), rng.choice([0, 7, 5000], size=40)])
    offsets = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(offsets[-1]))
    check_host(bases, offsets, 1, SEED)
    check_host(bases, offsets, 2, SEED)
    empties = (np.zeros(0, dtype=np.uint8), np.zeros(1001, dtype=np.int64))   # nothing but 1 000 empty reads
    for factor in (1, 2):
        got = check_host(*empties, factor, SEED)
        assert got.n_bases == 0 and (got.n_reads == 1000 or factor == 2)
    n = lens.size
    both = pick_seed(n, 2, lambda m: m[0] and m[-1])
    neither = pick_seed(n, 2, lambda m: not m[0] and not m[-1])
    assert check_host(bases, offsets, 2, both).kept[[0, -1]].tolist() == [0, n - 1]
    got = check_host(bases, offsets, 2, neither)
    assert got.kept[0] > 0 and got.kept[-1] < n - 1
    # one read only, kept and dropped; no read at all
    one = (bases[:100].copy(), np.array([0, 100], dtype=np.int64))
    assert check_host(*one, 2, pick_seed(1, 2, lambda m: m[0])).n_reads == 1
    assert check_host(*one, 2, pick_seed(1, 2, lambda m: not m[0])).n_reads == 0
    got = check_host(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), 2, SEED)
    assert got.n_reads == 0 and got.offsets.tolist() == [0]


def test_nothing_kept(hip_lib):
    bases, offsets = ragged(1000, seed=5)
    seed = pick_seed(1000, 1e12, lambda m: not m.any())
    got = check_host(bases, offsets, 1e12, seed)
    assert got.n_reads == 0 and got.n_bases == 0 and got.offsets.tolist() == [0]


@pytest.mark.parametrize("first_read", [(1 << 32) - 3, 1 << 40])
def test_read_index_beyond_32_bits(hip_lib, first_read):
    bases, offsets = ragged(1000, seed=6)
    check_host(bases, offsets, 2, SEED, first_read)
    # the high word counts: the reads at index 2^32 and beyond are not kept as those whose index has the same low word
    base = max(first_read, 1 << 32)
    skip = base - first_read
    rest = (bases[offsets[skip]:], offsets[skip:] - offsets[skip])
    high = check_host(*rest, 2, SEED, base)
    low = check_host(*rest, 2, SEED, base & 0xffffffff)
    assert not np.array_equal(high.kept - base, low.kept - (base & 0xffffffff))


def test_chunks_equal_the_whole_run(hip_lib):
    from covest_amd import sample
    n, L, first = 50_000, 20, 12345
    reads = np.random.default_rng(7).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, L))
    whole = sample.sample_reads(reads, 2, seed=SEED, first_read=first)
    want = ref.sample(reads, L, first, 2, SEED)
    assert np.array_equal(whole.bases.reshape(-1), want[0]) and np.array_equal(whole.kept, want[2])
    assert np.array_equal(whole.offsets, want[1])
    for cut in (1, 255, 256, 49_999):
        a = sample.sample_reads(reads[:cut], 2, seed=SEED, first_read=first)
        b = sample.sample_reads(reads[cut:], 2, seed=SEED, first_read=first + cut)
        assert np.array_equal(np.concatenate([a.bases, b.bases]), whole.bases), cut
        assert np.array_equal(np.concatenate([a.kept, b.kept]), whole.kept), cut
        assert np.array_equal(np.concatenate([a.offsets, b.offsets[1:] + a.offsets[-1]]), whole.offsets), cut


def test_simulated_reads_in(hip_lib):
    from covest_amd import sample, simulate as sim
    g = sim.random_genome(20_000, 3)
    reads = sim.simulate_reads(g, 100, n_reads=3000, error_rate=0.05, seed=3, first_read=77)
    got = sample.sample_reads(reads, 2, seed=3)          # numbered from the reads' own first_read
    rows = np.flatnonzero(ref.keep_mask(77, 3000, 2, 3))
    assert np.array_equal(got.kept, rows + 77) and np.array_equal(got.bases, reads.bases[rows])
    assert np.array_equal(got.positions, reads.positions[rows]) and np.array_equal(got.forward, reads.forward[rows])
    twin = reads.error_free(g)[rows]
    assert np.array_equal(got.error_free(g), twin)
    assert got.substitutions(g) == int(np.count_nonzero(reads.bases[rows] != twin))
    # sampling with the reads' own seed is independent of their content: about half the substitutions stay
    assert 0.4 < got.substitutions(g) / reads.substitutions(g) < 0.6


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import numpy as np
import kmer_reference as kr
import sample_reference as ref
import sim_reference as sr
from covest_amd import kmer_hist as kh, sample, simulate as sim
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
SEED = (0x5a3d << 32) | 0x0badcafe
PAT, WPAT = 0xA5, -0x0123456789abcdef
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
rng = np.random.default_rng(99)


def run(blob, offsets, L, n, first, factor, seed, s_shift, d_shift, where):
    # one device call between sentinels, every output against the restatement; returns (n_kept, bases_kept)
    total = blob.size
    src = torch.full((64 + s_shift + total + 64,), PAT, dtype=torch.uint8, device=dev)
    src[64 + s_shift:64 + s_shift + total] = torch.from_numpy(blob).to(dev)
    dst = torch.full((64 + d_shift + total + 64,), PAT, dtype=torch.uint8, device=dev)
    d_out_off = torch.full((n + 3,), WPAT, dtype=torch.int64, device=dev)
    d_kept = torch.full((n + 2,), WPAT, dtype=torch.int64, device=dev)
    d_counts = torch.full((4,), WPAT, dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
    sample.sample_reads_device(src.data_ptr() + 64 + s_shift, n, dst.data_ptr() + 64 + d_shift, d_counts.data_ptr() + 8, factor,
                               seed=seed, first_read=first, read_len=L, offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                               out_offsets_ptr=d_out_off.data_ptr() + 8, kept_ptr=d_kept.data_ptr() + 8, stream=stream)
    torch.cuda.synchronize()
    layout = offsets if offsets is not None else L if L > 0 else np.zeros(n + 1, dtype=np.int64)
    want_bases, want_off, want_kept = ref.sample(blob, layout, first, factor, seed)
    c, o, k, b, s = d_counts.cpu().numpy(), d_out_off.cpu().numpy(), d_kept.cpu().numpy(), dst.cpu().numpy(), src.cpu().numpy()
    nk, nb = want_kept.size, want_bases.size
    assert c.tolist() == [WPAT, nk, nb, WPAT], ("counts", where, c)
    assert np.array_equal(o[1:nk + 2], want_off) and o[0] == WPAT and (o[nk + 2:] == WPAT).all(), ("offsets", where)
    assert np.array_equal(k[1:nk + 1], want_kept) and k[0] == WPAT and (k[nk + 1:] == WPAT).all(), ("kept", where)
    at = 64 + d_shift
    assert np.array_equal(b[at:at + nb], want_bases), ("bases", where)
    assert (b[:at] == PAT).all() and (b[at + nb:] == PAT).all(), ("stray byte", where)
    assert (s[:64 + s_shift] == PAT).all() and (s[64 + s_shift + total:] == PAT).all(), ("source", where)
    return nk, nb


# fixed length: every read length and read count at every factor; source and destination 0, 1 and 7 bytes off a 16-byte
# boundary, never the same for both
SHIFTS = ((0, 1), (1, 7), (7, 0), (0, 7), (1, 0), (7, 1))
case = 0
for L in (1, 3, 4, 15, 16, 17, 100, 101):
    for n in (1, 2, 255, 256, 257, 70001):
        blob = rng.choice(ACGT, size=n * L)
        for factor in (1, 2, 16):
            for s_shift, d_shift in (SHIFTS if n == 257 else (SHIFTS[case % 6],)):
                run(blob, None, L, n, 3, factor, SEED, s_shift, d_shift, (L, n, factor, s_shift, d_shift))
            case += 1
run(np.zeros(0, np.uint8), None, 0, 300, 3, 2, SEED, 1, 7, "fixed length 0")
print("fixed ok")

# variable length at every pair of alignments; the offsets array is read on the device only
lens = rng.choice((0, 1, 2, 5, 16, 17, 100, 4095, 4096, 4097, 10000), size=700)
lens[300:560] = 0                                     # a run of empty reads longer than a workgroup has lanes
offsets = np.zeros(701, dtype=np.int64); np.cumsum(lens, out=offsets[1:])
blob = rng.choice(ACGT, size=int(offsets[-1]))
for factor in (1, 2, 16, 1e12):
    for s_shift, d_shift in SHIFTS:
        run(blob, offsets, 0, 700, (1 << 32) - 100, factor, SEED, s_shift, d_shift, ("ragged", factor, s_shift, d_shift))
# a source that does not start at offset 0 of its buffer
run(np.concatenate([np.full(37, 0x58, np.uint8), blob]), offsets + 37, 0, 700, 0, 2, SEED, 7, 1, "offsets from 37")
# n_reads == 0: counts (0, 0), out_offsets[0] = 0, nothing else
d_counts = torch.full((4,), WPAT, dtype=torch.int64, device=dev)
d_o = torch.full((3,), WPAT, dtype=torch.int64, device=dev)
sample.sample_reads_device(0, 0, 0, d_counts.data_ptr() + 8, 2, read_len=5, out_offsets_ptr=d_o.data_ptr() + 8, stream=stream)
torch.cuda.synchronize()
assert d_counts.cpu().tolist() == [WPAT, 0, 0, WPAT] and d_o.cpu().tolist() == [WPAT, 0, WPAT], "n_reads == 0"
print("variable ok")

# the scan's carry from pass to pass: one pass of sample_scan holds 4096 workgroups' pairs, 1 048 576 reads -- exactly one
# pass, one pair in the second, one more workgroup and a read; reads of length 1, then lengths of 0, 1 and 2, so that
# the two halves of the pair carry different sums
import time
t0 = time.perf_counter()
PASS = 4096 * 256
for n in (PASS, PASS + 1, PASS + 257):
    ones = rng.choice(ACGT, size=n)
    for factor in (2, 16):
        run(ones, None, 1, n, 3, factor, SEED, 1, 7, ("scan passes", n, factor))
short = np.zeros(PASS + 2, dtype=np.int64); np.cumsum(rng.choice((0, 1, 2), size=PASS + 1), out=short[1:])
nk, nb = run(rng.choice(ACGT, size=int(short[-1])), short, 0, PASS + 1, 3, 2, SEED, 7, 1, "scan passes, ragged")
assert nk != nb, "the two halves of the pair carry the same sum"
print("scan passes ok, %.2f s" % (time.perf_counter() - t0))

# host form and device form agree
got = sample.sample_reads((blob, offsets), 2, seed=SEED, first_read=5)
want = ref.sample(blob, offsets, 5, 2, SEED)
assert np.array_equal(got.bases, want[0]) and np.array_equal(got.offsets, want[1]) and np.array_equal(got.kept, want[2])
print("host form ok")

# genome -> simulate -> sample -> counter, the bases never leaving HBM
G, n, L, k = 20000, 6000, 100, 21
d_genome = torch.empty(G, dtype=torch.uint8, device=dev)
sim.random_genome_device(d_genome.data_ptr(), G, SEED, stream=stream)
d_reads = torch.empty(n * L, dtype=torch.uint8, device=dev)
sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_reads.data_ptr(), error_rate=0.02, seed=SEED, stream=stream)
d_half = torch.empty(n * L, dtype=torch.uint8, device=dev)
d_counts = torch.zeros(2, dtype=torch.int64, device=dev)
sample.sample_reads_device(d_reads.data_ptr(), n, d_half.data_ptr(), d_counts.data_ptr(), 2, seed=SEED, read_len=L, stream=stream)
n_kept, n_bases = d_counts.cpu().tolist()
rows = sr.reads_and_origin(sr.random_genome(G, SEED), L, 0, n, 0.02, SEED)[0]
rows = rows[ref.keep_mask(0, n, 2, SEED)]
assert n_kept == rows.shape[0] and n_bases == rows.size, "sample of simulated reads"
want_reads = [row.tobytes().decode() for row in rows]
for canonical in (True, False):
    want_hist, want_distinct = kr.histogram(want_reads, k, canonical)
    c = kh.KmerCounts(k, canonical=canonical)
    c.add_device(d_half.data_ptr(), n_kept, L, stream=stream)
    torch.cuda.synchronize()
    assert c.histogram() == want_hist and len(c) == want_distinct, ("add_device", canonical)
    c.close()
    c = kh.KmerCounts(k, canonical=canonical)
    path = c.count_reads_device(d_half.data_ptr(), n_kept, L, stream=stream)
    assert c.histogram() == want_hist and len(c) == want_distinct, ("count_reads_device", canonical, path)
    c.close()
print("counter ok")

# one input beyond 2^32 bytes: the simulator's 4.4e9-base run at factor 64
n, L, m = 44_000_000, 100, 1_000_000
big = torch.empty(n * L, dtype=torch.uint8, device=dev)
sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, big.data_ptr(), error_rate=0.01, seed=SEED, stream=stream)
out = torch.empty(n * L, dtype=torch.uint8, device=dev)
d_kept = torch.empty(n, dtype=torch.int64, device=dev)
sample.sample_reads_device(big.data_ptr(), n, out.data_ptr(), d_counts.data_ptr(), 64, seed=SEED, read_len=L,
                           kept_ptr=d_kept.data_ptr(), stream=stream)
n_kept, n_bases = d_counts.cpu().tolist()
assert n_bases == n_kept * L and abs(n_kept - n / 64) < 6 * (n / 64) ** 0.5, ("large run counts", n_kept)
tail = np.flatnonzero(ref.keep_mask(n - m, m, 64, SEED)) + (n - m)
kept = d_kept[n_kept - tail.size - 1:n_kept].cpu().numpy()
assert np.array_equal(kept[1:], tail) and kept[0] < n - m, "large run kept"
last = d_kept[n_kept - 1000:n_kept]
src_rows = big.view(n, L)[last].cpu().numpy()
assert np.array_equal(out[(n_kept - 1000) * L:n_kept * L].cpu().numpy().reshape(1000, L), src_rows), "large run rows"
first_rows = big.view(n, L)[d_kept[:1000]].cpu().numpy()
assert np.array_equal(out[:1000 * L].cpu().numpy().reshape(1000, L), first_rows), "large run first rows"
del big, out, d_kept
print("large run ok")
print("device forms ok")
"""


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): every fixed read length and read count at three factors and six pairs of
    alignments, ragged reads with a long run of empty ones, nothing written outside the stated ranges, read counts at
    and just beyond one pass of the scan (its carry, bit for bit), the sample into the k-mer counter through add_device and count_reads_device, and a 4.4e9-base input at factor 64."""
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "device forms ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


@functools.lru_cache(maxsize=None)
def fasta_reads():
    """3 000 reads of mixed lengths from kmer_reference's genome, some empty, some with N: (text, preprocessed reads)."""
    import random
    rng = random.Random(77)
    lines, reads = [], []
    for i in range(3000):
        length = rng.choice((0, 0, 5, 20, 21, 22, 60, 100, 150, 400))
        seq = list(kr.genome_reads(rng, 1, length)[0]) if length else []
        if seq and i % 7 == 0:
            seq[rng.randrange(len(seq))] = "N"
        seq = "".join(seq)
        lines.append(">r%d" % i)
        lines += [seq[j:j + 60] for j in range(0, len(seq), 60)]
        reads.append(kr.preprocess(seq))
    return "\n".join(lines) + "\n", tuple(reads)


def test_sampled_histogram_and_file(hip_lib, tmp_path):
    from covest_amd import kmer_hist as kh, sample
    text, reads = fasta_reads()
    src = tmp_path / "reads.fa"
    src.write_text(text)
    k, factor, seed = 21, 2, 5
    mask = ref.keep_mask(0, len(reads), factor, seed)
    kept_reads = [r for r, m in zip(reads, mask) if m]
    want = kr.histogram(kept_reads, k, canonical=True)[0]
    for batch_bases in (400, 1 << 12, 1 << 26):
        got = sample.sampled_histogram(str(src), k, factor, seed=seed, canonical=True, batch_bases=batch_bases)
        assert got == want, batch_bases
    dest = tmp_path / "sampled.fa"
    assert sample.sample_reads_file(str(src), str(dest), factor, seed=seed, batch_bases=1 << 12) == (len(reads), len(kept_reads))
    names = [line[1:] for line in dest.read_text().splitlines() if line.startswith(">")]
    assert names == ["read_%d" % i for i in np.flatnonzero(mask)]
    back = []
    for bases, offsets, n, n_bases in kh.ReadBatches(str(dest), kh.NS_IGNORE):
        import ctypes
        blob = ctypes.string_at(bases, n_bases).decode("ascii")
        back += [blob[offsets[i]:offsets[i + 1]] for i in range(n)]
    assert back == kept_reads


# ---- closing the loop ------------------------------------------------------------------------------------------------
# profiles/sample_recovery.txt (tools/sample_recovery.py): the largest relative deviation of the estimate from the
# SAMPLE's truth over seeds 1..8 on an MI355X, per quantity.  The test (seed 0, not among them) allows twice that -- the
# spread of eight draws understates the tail -- and never more than the caps of DESIGN.md section 6l.
RECORDED_MAX_DEVIATION = None
CAPS = {"coverage": 0.05, "error_rate": 0.15, "genome_size": 0.05, "genome_size_reads": 0.05}


def test_estimate_recovers_the_samples_truth(hip_lib):
    from sample_recovery import recover
    got = recover(0)
    for q, (truth, est, dev) in got.items():
        print("%-18s truth %.6g estimate %.6g relative deviation %.4f" % (q, truth, est, dev))
    for q, (truth, est, dev) in got.items():
        bound = CAPS[q] if RECORDED_MAX_DEVIATION is None else min(2 * RECORDED_MAX_DEVIATION[q], CAPS[q])
        assert dev <= bound, (q, truth, est, dev)
