"""The correction of isolated substitutions on the device (kmer_correct.hip through KmerCounts.correct and the C ABI)
against its plain Python restatement (tests/correct_reference.py): the output bytes equal byte for byte and the rows
{runs, corrected, ambiguous, unfixable} word for word, whatever the key width, the shape of the reads, where a run lies
in the wave's chunks of 64 windows, the fill of the table or the alignment of the caller's buffers.

Host forms run in this process.  What needs device buffers runs in ONE fresh child process with torch imported first (one
HIP runtime a process), as tests/test_gpu_lookup.py does.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import correct_reference as cr
import kmer_reference as kr
import lookup_reference as lr

pytestmark = pytest.mark.gpu

CUTOFF = 2


def check_equal(got, want, where, before=None):
    """A CorrectedReads against cr.correct's (out, offsets, fix, strings): every byte, every word."""
    out, offsets, fix, strings = want
    assert np.array_equal(got.offsets, offsets), where
    assert got.bases.dtype == np.uint8 and np.array_equal(got.bases, out), where
    assert got.fix.dtype == np.uint32 and np.array_equal(got.fix, fix), where
    for j, name in enumerate(("runs", "corrected", "ambiguous", "unfixable")):
        column = getattr(got, name)
        assert column.dtype == np.int64 and np.array_equal(column, fix[:, j]), (where, name)
    assert got.strings() == list(strings), where
    if before is not None:
        flat = np.frombuffer("".join(before).encode(), dtype=np.uint8)
        assert np.array_equal(got.changed, np.flatnonzero(flat != out)), where
        assert got.changed.size == int(fix[:, 1].sum()), where  # one byte a corrected run, and no other


def planted(read, *positions):
    """`read` with another base, in the same case, at each of `positions`."""
    r = list(read)
    for n, p in enumerate(positions):
        at = "ACGT".index(r[p].upper())
        r[p] = chr(ord("ACGT"[(at + 1 + (p + n) % 3) % 4]) | (ord(r[p]) & 0x20))
    return "".join(r)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 12, 13, 31])
def test_exact(hip_lib, k, canonical):
    """Every key width's paths (k = 12: no first slot; 13: the smallest with one; 31: the widest word) on the reads of
    the lookup's test: lengths 0, 1, k - 1, k, k + 62 .. k + 65, k + 127 .. k + 129 in mixed case, keys that collide in
    the first slot (probe_reads), and reads of 0 .. k + 130 bases of which many windows are absent or counted once:
    runs of every length and place, most of them unfixable (the planted tests below hold the corrections)."""
    from covest_amd.kmer_hist import KmerCounts
    batches = kr.sweep_batches(k) + [list(kr.probe_reads(k))]
    counted = [r for b in batches for r in b]
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        for b in batches:
            counts.add_reads(b)
        reads = counted + kr.device_ragged_reads(k)
        want = cr.correct(reads, kr.count(counted, k, canonical), k, canonical, CUTOFF)
        assert (k == 1 or want[2][:, 0].any()) and (np.diff(want[1]) < k).any()  # runs; reads without a window
        check_equal(counts.correct(reads, CUTOFF), want, (k, canonical), reads)
    finally:
        counts.close()


PLANT_K = 21


@functools.lru_cache(maxsize=None)
def genome_counts(k, canonical=True):
    return kr.count([kr.genome()] * 3, k, canonical)


@functools.lru_cache(maxsize=None)
def genome_counter(k=PLANT_K, canonical=True):
    """A KmerCounts that holds the genome three times; shared, never closed before the process ends."""
    from covest_amd.kmer_hist import KmerCounts
    return KmerCounts(k, canonical=canonical).add_reads([kr.genome()] * 3)


def planted_cases(k):
    """(reads, positions planted per read, clean reads): one substitution at the ends of the read and of its first and
    last window; where the run ends at window 63 or 127 (closed in the next chunk from the codes of the one before),
    straddles 63 | 64 and 127 | 128, and starts at 64 and 128; reads of fewer than 2k - 1 bases (the whole read is one run
    and several positions are tried); in both cases of the letters."""
    g = kr.genome()
    reads, where, clean = [], [], []
    for start, length in ((100, k + 140), (700, k + 64), (1300, k + 63)):
        read = g[start:start + length]
        ps = {0, 1, k - 2, k - 1, k, length - k - 1, length - k, length - k + 1, length - 1}
        ps |= {63, 64, 70, 63 + k - 1, 64 + k - 1, 127, 128, 135, 127 + k - 1, 128 + k - 1}
        for n, p in enumerate(sorted(p for p in ps if 0 <= p < length)):
            r = read.lower() if n % 2 else read
            reads.append(planted(r, p))
            where.append((p,))
            clean.append(r)
    for length in (k, k + 1, 2 * k - 3, 2 * k - 2, 2 * k - 1):
        read = g[2000:2000 + length]
        for p in sorted({0, length // 2, length - k, min(k - 1, length - 1), length - 1}):
            reads.append(planted(read, p))
            where.append((p,))
            clean.append(read)
    return reads, where, clean


@pytest.mark.parametrize("k,canonical", [(12, True), (13, False), (PLANT_K, True), (31, True), (31, False)])
def test_one_substitution_at_every_kind_of_position(hip_lib, k, canonical):
    reads, where, clean = planted_cases(k)
    want = cr.correct(reads, genome_counts(k, canonical), k, canonical, CUTOFF)
    got = genome_counter(k, canonical).correct(reads, CUTOFF)
    check_equal(got, want, "planted", reads)
    inner = 0
    for read, (p,), original, fixed, row in zip(reads, where, clean, got.strings(), got.fix.tolist()):
        if k - 1 <= p <= len(read) - k:  # an inner position: a run of k windows with both neighbours strong
            assert fixed == original and row == [1, 1, 0, 0], (p, len(read))
            inner += 1
        assert row[0] == 1, (p, len(read))
    assert inner >= 20
    # the same reads as reads of one blob at offsets that start at 3
    blob = np.frombuffer(("NNN" + "".join(reads) + "N").encode(), dtype=np.uint8)
    check_equal(genome_counter(k, canonical).correct((blob, want[1] + 3), CUTOFF), want, "offsets from 3")


def test_two_substitutions_by_distance(hip_lib):
    """k - 1 and k apart: one merged run of 2k - 1 and 2k windows, unfixable, bytes unchanged; k + 1 apart: one strong
    window between, both corrected.  Once inside a chunk, once across windows 63 | 64."""
    k = PLANT_K
    read = kr.genome()[400:400 + 3 * k + 80]
    reads, rows = [], []
    for first in (k + 3, 50):
        for d, row in ((k - 1, [1, 0, 0, 1]), (k, [1, 0, 0, 1]), (k + 1, [2, 2, 0, 0])):
            reads.append(planted(read, first, first + d))
            rows.append(row)
    want = cr.correct(reads, genome_counts(k), k, True, CUTOFF)
    assert want[2].tolist() == rows
    got = genome_counter().correct(reads, CUTOFF)
    check_equal(got, want, "two substitutions", reads)
    for fixed, before, row in zip(got.strings(), reads, rows):
        assert fixed == (read if row[1] else before)


def test_ambiguity_by_construction(hip_lib):
    from covest_amd.kmer_hist import KmerCounts
    k = PLANT_K
    g = kr.genome()
    x, y = g[:40], g[41:90]
    read = x + "g" + y
    for counted, row, fixed in (([x + "a" + y, x + "c" + y], [1, 0, 1, 0], read), ([x + "a" + y], [1, 1, 0, 0], x + "a" + y)):
        counts = KmerCounts(k, canonical=True).add_reads(counted * 3)
        try:
            got = counts.correct([read, read.upper()], CUTOFF)
            want = cr.correct([read, read.upper()], kr.count(counted * 3, k, True), k, True, CUTOFF)
            check_equal(got, want, row)
            assert got.fix.tolist() == [row, row] and got.strings() == [fixed, fixed[:40] + fixed[40].upper() + fixed[41:]]
        finally:
            counts.close()


def test_cutoff_zero_changes_nothing(hip_lib):
    reads, _, _ = planted_cases(PLANT_K)
    got = genome_counter().correct(reads + ["", "acg"], 0)
    assert got.strings() == reads + ["", "acg"] and not got.fix.any() and got.changed.size == 0


def add_without_reserve(counts, reads):
    """covest_kmer_add as it stands: the table keeps the size it was created with."""
    from covest_amd import _capi
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    _capi.check(_capi.lib().covest_kmer_add(counts._handle, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(reads)),
                "covest_kmer_add")


def test_full_table_and_after_reserve(hip_lib):
    """A 1 024-slot table at the contract's limit (500 distinct 21-mers, no reserve): trial keys probe through a full
    neighbourhood; then the same answers from the 4 096-slot table covest_kmer_reserve re-inserted them into."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    g = kr.genome()
    counted = [g[:520], g[100:300], g[250:520].lower(), kr.revcomp(g[40:90])]
    reads = [planted(g[100:300], 60), planted(g[250:520].lower(), 3, 150), planted(g[:520], 200, 215), g[1000:1100],
             planted(kr.revcomp(g[40:90]), 49), "", g[:20]]
    table = kr.count(counted, k, True)
    assert len(table) == 500
    want = cr.correct(reads, table, k, True, CUTOFF)
    assert want[2][:, 1].sum() >= 3 and want[2][:, 3].sum() >= 2
    counts = KmerCounts(k, canonical=True, min_slots=1024)
    try:
        add_without_reserve(counts, counted)
        assert counts.slots == 1024 and len(counts) == 500
        check_equal(counts.correct(reads, CUTOFF), want, "1024 slots", reads)
        _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 4096), "covest_kmer_reserve")
        assert counts.slots == 4096 and len(counts) == 500
        check_equal(counts.correct(reads, CUTOFF), want, "4096 slots", reads)
    finally:
        counts.close()


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import random
import numpy as np
import kmer_reference as kr
import correct_reference as cr
from covest_amd import _capi, kmer_hist as kh
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
k, CUTOFF = 21, 2
table = kr.count([kr.genome()] * 2, k, True)
d_genome = torch.from_numpy(np.frombuffer(kr.genome().encode(), dtype=np.uint8).copy()).to(dev)
counts = kh.KmerCounts(k, canonical=True, min_slots=1 << 14)
for _ in range(2):
    counts.add_device(d_genome.data_ptr(), 1, len(kr.genome()), stream=stream, reserve=False)
PAT8, PAT32 = 0x5A, 0xA5A5A5A5
PAD = 16


def run(reads, fixed_len, shift, out_shift=1, want_fix=True, in_place=False):
    # the device form on `reads` whose bases start `shift` bytes into an aligned buffer, `out` starting PAD + out_shift
    # bytes into another (in place: the bases themselves): (out, fix or None); canaries either side of both checked
    blob = np.frombuffer(("N" * shift + "".join(reads) + "N" * PAD).encode(), dtype=np.uint8).copy()
    d_bases = torch.from_numpy(blob).to(dev)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    d_offsets = torch.from_numpy(offsets).to(dev)
    n, n_pos = len(reads), int(offsets[-1])
    lead = PAD + out_shift
    o = torch.full((lead + n_pos + PAD,), PAT8, dtype=torch.uint8, device=dev)
    f = torch.from_numpy(np.full(PAD + 4 * n + PAD, PAT32, dtype=np.uint32).view(np.int32)).to(dev)
    counts.correct_device(d_bases.data_ptr() + shift, n, fixed_len if fixed_len is not None else 0,
                          d_bases.data_ptr() + shift if in_place else o.data_ptr() + lead,
                          d_offsets_ptr=None if fixed_len is not None else d_offsets.data_ptr(), cutoff=CUTOFF,
                          d_fix_ptr=f.data_ptr() + 4 * PAD if want_fix else None, stream=stream)
    torch.cuda.synchronize()
    o, f, b = o.cpu().numpy(), f.cpu().numpy().view(np.uint32), d_bases.cpu().numpy()
    where = (len(reads), fixed_len, shift, out_shift, want_fix, in_place)
    assert (f[:PAD] == PAT32).all() and (f[PAD + 4 * n:] == PAT32).all(), ("stray fix", where)
    if not want_fix:
        assert (f == PAT32).all(), ("fix written though null", where)
    if in_place:
        assert (o == PAT8).all(), ("out written though in place", where)
        assert (b[:shift] == ord("N")).all() and (b[shift + n_pos:] == ord("N")).all(), ("stray bases", where)
        got = b[shift:shift + n_pos]
    else:
        assert (o[:lead] == PAT8).all() and (o[lead + n_pos:] == PAT8).all(), ("stray out", where)
        assert np.array_equal(b, blob), ("bases written", where)
        got = o[lead:lead + n_pos]
    return got, f[PAD:PAD + 4 * n].reshape(n, 4) if want_fix else None


def same(got, want, where):
    assert np.array_equal(got[0], want[0]), ("out", where)
    if got[1] is not None:
        assert np.array_equal(got[1], want[2]), ("fix", where)


def planted(read, *positions):
    r = list(read)
    for n, p in enumerate(positions):
        at = "ACGT".index(r[p].upper())
        r[p] = chr(ord("ACGT"[(at + 1 + (p + n) % 3) % 4]) | (ord(r[p]) & 0x20))
    return "".join(r)


rng = random.Random(99)
# reads of their own lengths (an empty one, one shorter than k), substitutions planted in most; d_bases at byte offsets
# 0, 1, 3 and out at 0, 1, 2, 3 past its canary; fix null; in place
ragged = [planted(r, len(r) // 3) for r in kr.genome_reads(rng, 2, k + 70)] + ["", kr.genome()[:k - 1], "ACGT" * 30]
ragged += [planted(r.lower() if n % 2 else r, 5 + 31 * n, 2 * k + 190 - 17 * n)
           for n, r in enumerate(kr.genome_reads(rng, 5, 2 * k + 200))]
want = cr.correct(ragged, table, k, True, CUTOFF)
assert want[2][:, 1].sum() >= 8 and want[2][:, 3].sum() >= 1, want[2]
for shift, out_shift in ((0, 0), (1, 1), (3, 2), (1, 3)):
    same(run(ragged, None, shift, out_shift), want, ("ragged", shift, out_shift))
same(run(ragged, None, 1, 1, want_fix=False), want, "ragged, fix null")
same(run(ragged, None, 3, in_place=True), want, "ragged, in place")
same(run(ragged, None, 0, want_fix=False, in_place=True), want, "ragged, in place, fix null")
print("device form ok")

# reads of one length without offsets against the same reads with them: every shape of the wave
for length in (k, k + 63, k + 64, k + 65, 2 * k + 200, k - 1):
    for n in (1, 3, 4, 5):
        reads = [planted(r, (7 * i + length // 2) % length) for i, r in enumerate(kr.genome_reads(rng, n, length))]
        want = cr.correct(reads, table, k, True, CUTOFF)
        same(run(reads, length, 3), want, ("fixed", length, n))
        same(run(reads, None, 3), want, ("offsets", length, n))
        same(run(reads, length, 1, in_place=True), want, ("fixed, in place", length, n))
print("fixed length ok")

# statuses that need device buffers
L = _capi.lib()
INVALID, UNSUPPORTED = _capi.COVEST_E_INVALID, _capi.COVEST_E_UNSUPPORTED
d_reads = torch.from_numpy(np.frombuffer("".join(kr.genome_reads(rng, 300, 100)).encode(), dtype=np.uint8).copy()).to(dev)
d_out = torch.zeros(300 * 100 + 64, dtype=torch.uint8, device=dev)
d_fix = torch.zeros(4 * 300 + 4, dtype=torch.int32, device=dev)


def call(c, bases, n, read_len, out, fix, offsets=None):
    return L.covest_kmer_correct_reads_device(c._handle if c is not None else None, bases, offsets, n, read_len, 2, out,
                                              fix, stream)


B, O, F = d_reads.data_ptr(), d_out.data_ptr(), d_fix.data_ptr()
assert call(None, B, 300, 100, O, F) == INVALID
assert call(counts, B, -1, 100, O, F) == INVALID
assert call(counts, B, 300, -1, O, F) == INVALID
assert call(counts, B, 300, 100, None, F) == INVALID                                   # a null out
assert call(counts, None, 300, 100, O, F) == INVALID
assert call(counts, B, 300, 100, O, F + 4) == INVALID and "16" in _capi.last_error()   # fix rows are 16-byte stores
assert call(counts, B, 300, 100, B + 1, F) == INVALID and "overlap" in _capi.last_error()
assert call(counts, B + 100, 299, 100, B, F) == INVALID
assert call(counts, None, 0, 100, None, F) == 0                                        # no reads: OK, nothing touched
torch.cuda.synchronize()
assert not d_out.cpu().numpy().any() and not d_fix.cpu().numpy().any(), "a refused or empty call wrote something"
wide = kh.KmerCounts(32)
assert call(wide, B, 300, 100, O, F) == UNSUPPORTED
wide.close()
bulk = kh.KmerCounts(k, canonical=True)
path = bulk.count_reads_device(B, 300, 100, stream=stream)
assert path == "partitioned", (path, getattr(bulk, "why_not_partitioned", None))
assert call(bulk, B, 300, 100, O, F) == INVALID and "covest_kmer_count_reads_device result" in _capi.last_error()
bulk.clear(stream)
bulk.add_device(B, 300, 100, stream=stream)
bulk.correct_device(B, 300, 100, O, cutoff=1, d_fix_ptr=F, stream=stream)   # every k-mer was counted: nothing is weak
torch.cuda.synchronize()
assert np.array_equal(d_out.cpu().numpy()[:30000], d_reads.cpu().numpy()) and not d_out.cpu().numpy()[30000:].any()
assert not d_fix.cpu().numpy().any()
bulk.close()
counts.close()
print("statuses ok")
print("correct device forms ok")
"""


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): d_bases at byte offsets 0, 1 and 3, out at odd byte alignments with canaries
    either side of out and fix, fix null, in place (out == bases) giving the same bytes and touching nothing else, reads
    of one length against the same reads with offsets, and every status that needs device buffers."""
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "correct device forms ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


def test_statuses(hip_lib):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    blob = np.frombuffer(b"ACGT" * 20, dtype=np.uint8)
    offsets = np.array([0, 80], dtype=np.int64)
    out = np.zeros(80, dtype=np.uint8)
    fix = np.full((1, 4), 7, dtype=np.uint32)

    def call(counts, n, out_array, fix_array):
        return hip_lib.covest_kmer_correct_reads(
            counts._handle if counts is not None else None, blob.ctypes.data, offsets.ctypes.data, n, 2,
            out_array.ctypes.data if out_array is not None else None,
            fix_array.ctypes.data if fix_array is not None else None)
    wide, counts = KmerCounts(32), KmerCounts(21)
    try:
        assert call(wide, 1, out, fix) == _capi.COVEST_E_UNSUPPORTED
        with pytest.raises(_capi.CovestHipError, match=r"\(-5\)"):
            wide.correct(["ACGT" * 20], 2)
        assert call(counts, -1, out, fix) == _capi.COVEST_E_INVALID
        assert call(None, 1, out, fix) == _capi.COVEST_E_INVALID
        assert call(counts, 1, None, fix) == _capi.COVEST_E_INVALID           # a null out
        assert call(counts, 0, out, fix) == 0 and not out.any() and (fix == 7).all()  # no reads: OK, nothing written
        assert call(counts, 1, out, None) == 0 and np.array_equal(out, blob)  # fix is optional
        out[:] = 0
        assert call(counts, 1, out, fix) == 0                                 # an empty table: one run of 60 windows
        assert np.array_equal(out, blob) and fix.tolist() == [[1, 0, 0, 1]]
    finally:
        wide.close()
        counts.close()


def test_overflowed_table_is_refused_by_the_host_form(hip_lib):
    """The sticky overflow flag: the counts are partial, so the host form answers COVEST_E_NOMEM."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    counts = KmerCounts(21, min_slots=1024)
    try:
        with pytest.raises(_capi.CovestHipError, match=r"\(-4\)"):
            add_without_reserve(counts, [kr.genome()])  # 2 980 distinct 21-mers into 1 024 slots
        with pytest.raises(_capi.CovestHipError, match=r"\(-4\)"):
            counts.correct([kr.genome()[:100]], 2)
    finally:
        counts.close()


# ---- the simulated case of DESIGN.md section 6af on the device ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_case():
    """(genome, SimulatedReads, KmerCounts that hold them) of lookup_reference.CASE, made on the device; shared."""
    from covest_amd import kmer_hist as kh, simulate as sim
    c = lr.CASE
    genome = sim.random_genome(c["genome_len"], c["seed"])
    reads = sim.simulate_reads(genome, c["read_len"], n_reads=c["n_reads"], error_rate=c["error_rate"], seed=c["seed"])
    return genome, reads, reads.add_to(kh.KmerCounts(c["k"], canonical=True))


def test_simulated_case(hip_lib):
    """Count, correct at cutoff 3, recount: the pinned figures of tests/test_correct_cpu.py, from the device."""
    from covest_amd.kmer_hist import KmerCounts
    c, want = lr.CASE, cr.CASE_EXPECTED
    genome, reads, counts = device_case()
    truth = reads.error_free(genome)
    assert np.array_equal(reads.bases, lr.simulated_case()[1]) and np.array_equal(truth, cr.simulated_case_truth())
    got = counts.correct(reads, c["cutoff"])
    out, fix, strings = cr.simulated_case_corrected()
    assert np.array_equal(got.bases.reshape(out.shape), out) and np.array_equal(got.fix, fix)
    totals = [int(getattr(got, name).sum()) for name in ("runs", "corrected", "ambiguous", "unfixable")]
    assert totals == [want[name] for name in ("runs", "corrected", "ambiguous", "unfixable")] == [1624, 1402, 0, 222]
    figures = cr.recovery_figures(reads.bases, got.bases.reshape(out.shape), truth)
    print("wrong bases %d -> %d, reads with a wrong base %d -> %d, miscorrections %d, reads made worse %d" % figures)
    assert figures == (1851, 449, 1396, 218, 0, 0)
    histogram = counts.histogram()
    assert (len(counts), int(histogram[1])) == (want["distinct_before"], want["singletons_before"]) == (26989, 20329)
    recount = KmerCounts(c["k"], canonical=True)
    try:
        recount.add_reads(got.strings())
        assert got.strings() == list(strings)
        histogram = recount.histogram()
        assert (len(recount), int(histogram[1])) == (want["distinct_after"], want["singletons_after"]) == (10260, 4235)
    finally:
        recount.close()


def test_end_to_end(hip_lib):
    """The same reads' histogram fitted by the basic model at sample factor 1, correct_reads at level 0.5: the cutoff
    is the posterior's, the reads and rows equal the restatement's at that cutoff, and print_output carries the record."""
    from covest_amd import constants, correct_reads, posterior_classes, print_output
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    c = lr.CASE
    k, read_len = c["k"], c["read_len"]
    _, reads, counts = device_case()
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, k, read_len, sample_factor=1)
    assert sample_factor == 1
    model = select_model("basic")(k, read_len, hist, tail, max_error=constants.MAX_ERRORS)
    guess = [guess_c, guess_e]
    estimate, success = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage(guess)
    fixed = correct_reads(model, estimate, counts, reads, level=0.5)
    print("estimate", list(estimate), "fitted cutoff", fixed.cutoff)
    assert 2 <= fixed.cutoff < 30 * 48 / 64  # above the errors (abundance 1), below the genomic mode
    assert fixed.cutoff == posterior_classes(model, estimate).error_cutoff(0.5) and fixed.level == 0.5
    out, fix, strings = cr.simulated_case_corrected(fixed.cutoff)
    assert np.array_equal(fixed.bases.reshape(out.shape), out) and np.array_equal(fixed.fix, fix)
    assert fixed.strings() == list(strings)
    assert fixed.corrected_share == float(((fix[:, 0] > 0) & (fix[:, 1] == fix[:, 0])).mean())
    assert fixed.unresolved_share == float((fix[:, 1] < fix[:, 0]).mean())
    at_three = correct_reads(model, estimate, counts, reads, cutoff=3)
    assert at_three.cutoff == 3 and np.array_equal(at_three.fix, cr.simulated_case_corrected(3)[1])
    plain = print_output(hist_orig, model, success, sample_factor, estimate, guess, silent=True)
    record = print_output(hist_orig, model, success, sample_factor, estimate, guess, silent=True, corrections=fixed)
    names = ("cutoff", "reads", "runs", "corrected", "ambiguous", "unfixable")
    assert set(record) - set(plain) == {"corrections_" + name for name in names}
    assert {key: record[key] for key in plain} == plain
    assert [record["corrections_" + name] for name in names] == [fixed.cutoff, c["n_reads"]] + fix.sum(axis=0).tolist()
    with pytest.raises(ValueError):
        correct_reads(model, estimate, counts, reads, level=0.0)  # no key's erroneous share is below 0
