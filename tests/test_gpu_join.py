"""Two k-mer tables joined on the device (kmer_join.hip through KmerCounts.join_histogram and the C ABI) against the
restatement of the definition (tests/join_reference.py over tests/kmer_reference.py): every cell equal, whatever the key
width, the sizes and fills of the two tables, the key sets, the clips and the place of the LDS rectangle's edge.

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

import join_reference as jr
import kmer_reference as kr

pytestmark = pytest.mark.gpu

LDS = (256, 16)   # csrc/kmer_join.h kLdsRows, kLdsCols (tests/test_join_cpu.py runs the header itself)


@functools.lru_cache(maxsize=None)
def counted(k, canonical, seed, n=300, which=0):
    return kr.count(jr.noisy_reads(seed, n=n, which=which), k, canonical)


def add_without_reserve(counts, reads):
    """covest_kmer_add as it stands: the table keeps the size it was created with."""
    from covest_amd import _capi
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    _capi.check(_capi.lib().covest_kmer_add(counts._handle, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(reads)),
                "covest_kmer_add")


def clipped(hist, n):
    """A count-of-counts list as the row (column) sums of a matrix of n rows (columns): index 0 left out."""
    out = [0] * n
    for c, v in enumerate(hist):
        if c > 0:
            out[min(c, n - 1)] += v
    return out[1:] if n > 1 else []


def check(a, b, ref_a, ref_b, shapes, where):
    """a.join_histogram(b) against the restatement at every shape, and the identities against the counters' own
    histograms (code that existed before the join)."""
    hist_a, hist_b = a.histogram(), b.histogram()
    for rows, cols in list(shapes) + [jr.unclipped_shape(ref_a, ref_b)]:
        got = a.join_histogram(b, rows, cols)
        assert got.dtype == np.int64 and got.shape == (rows, cols), where
        assert np.array_equal(got, jr.join(ref_a, ref_b, rows, cols)), (where, rows, cols)
        assert got.sum() == len(set(ref_a) | set(ref_b)), (where, rows, cols)
        if rows > 1:
            assert got[1:].sum(axis=1).tolist() == clipped(hist_a, rows), (where, rows, cols)
        if cols > 1:
            assert got[:, 1:].sum(axis=0).tolist() == clipped(hist_b, cols), (where, rows, cols)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 12, 13, 21, 31])
def test_key_widths(hip_lib, k, canonical):
    """k = 5 and 12: no first slot; 13: the smallest with one; 21: the common case; 31: the top of one word.  Two read
    sets of one genome with 2 % substitutions: shared keys, keys of either side alone, keys that share minimizers."""
    from covest_amd.kmer_hist import KmerCounts
    reads_a, reads_b = jr.noisy_reads(1), jr.noisy_reads(2)
    ref_a, ref_b = counted(k, canonical, 1), counted(k, canonical, 2)
    a, b = KmerCounts(k, canonical=canonical, min_slots=1024), KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        a.add_reads(reads_a)
        b.add_reads(reads_b)
        full = jr.join(ref_a, ref_b, *jr.unclipped_shape(ref_a, ref_b))
        assert full[1:, 1:].sum() > 0 and (k == 5 or (full[0].sum() > 0 and full[1:, 0].sum() > 0))
        check(a, b, ref_a, ref_b, [(3, 2), LDS], (k, canonical))
        check(b, a, ref_b, ref_a, [(2, 7)], (k, canonical, "swapped"))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("k", [12, 21])
def test_table_sizes(hip_lib, k):
    """Both tables near half full at 2^10 slots; A at 2^10 with B at 2^14 and the reverse; one table grown by
    covest_kmer_reserve after its adds.  Each table is walked and probed with its own log2_slots."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    few_a, few_b = jr.noisy_reads(3, n=7), jr.noisy_reads(4, n=7)          # about 500 keys each
    many = jr.noisy_reads(5, n=220)                                         # a third of 2^14 slots
    ref_few_a, ref_few_b, ref_many = counted(k, True, 3, 7), counted(k, True, 4, 7), counted(k, True, 5, 220)
    assert 400 <= len(ref_few_a) <= 620 and 400 <= len(ref_few_b) <= 620 and 4500 <= len(ref_many) <= 8100

    def table(reads, min_slots):
        c = KmerCounts(k, canonical=True, min_slots=min_slots)
        add_without_reserve(c, reads)
        assert c.slots == min_slots
        return c
    small_a, small_b, big = table(few_a, 1 << 10), table(few_b, 1 << 10), table(many, 1 << 14)
    try:
        check(small_a, small_b, ref_few_a, ref_few_b, [(4, 4)], (k, "2^10 with 2^10"))
        check(small_a, big, ref_few_a, ref_many, [(4, 4)], (k, "2^10 with 2^14"))
        check(big, small_a, ref_many, ref_few_a, [(4, 4)], (k, "2^14 with 2^10"))
        _capi.check(hip_lib.covest_kmer_reserve(small_b._handle, 1 << 12), "covest_kmer_reserve")
        assert small_b.slots == 1 << 12
        check(small_a, small_b, ref_few_a, ref_few_b, [(4, 4)], (k, "2^10 with one grown to 2^12"))
        check(small_b, big, ref_few_b, ref_many, [(4, 4)], (k, "grown with 2^14"))
    finally:
        for c in (small_a, small_b, big):
            c.close()


def test_key_sets(hip_lib):
    """The same reads on both sides (nothing off the diagonal), disjoint genomes, one side empty, both; reads shorter
    than k on one side, whose one key is a key like any other."""
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads = jr.noisy_reads(1)
    ref = counted(k, True, 1)
    other = counted(k, True, 6, 300, 1)
    assert not set(ref) & set(other)
    short = [jr.genome(0)[:k - 1], jr.genome(0)[100:100 + k - 1], "", jr.genome(0)[40:45], jr.genome(0)[:k - 1]]
    ref_short = kr.count(list(reads[:40]) + short, k, True)
    assert len(ref_short) > len(kr.count(reads[:40], k, True))
    a, same, apart, empty, empty2, with_short = (KmerCounts(k, canonical=True, min_slots=1024) for _ in range(6))
    try:
        a.add_reads(reads)
        same.add_reads(reads)
        apart.add_reads(jr.noisy_reads(6, which=1))
        with_short.add_reads(list(reads[:40]) + short)
        check(a, same, ref, ref, [(5, 5)], "A = B")
        full = a.join_histogram(same, *jr.unclipped_shape(ref, ref))
        assert full.sum() == np.trace(full) == len(ref)
        check(a, apart, ref, other, [(5, 5)], "disjoint")
        assert a.join_histogram(apart, 9, 9)[1:, 1:].sum() == 0
        check(a, empty, ref, {}, [(5, 5), (1, 1)], "B empty")
        check(empty, a, {}, ref, [(5, 5), (1, 1)], "A empty")
        for rows, cols in ((1, 1), (3, 4), LDS, (LDS[0] + 1, LDS[1] + 1)):
            assert not a.join_histogram(empty, rows, cols)[:, 1:].any()
            assert not empty.join_histogram(empty2, rows, cols).any(), "both empty"
        check(with_short, a, ref_short, ref, [(5, 5)], "short reads in A")
        check(a, with_short, ref, ref_short, [(5, 5)], "short reads in B")
    finally:
        for c in (a, same, apart, empty, empty2, with_short):
            c.close()


@functools.lru_cache(maxsize=None)
def weighted_case(k):
    """A: 300 reads, the first added 70 000 times, the second 13 times and the third 300 times (add_weighted)."""
    reads = jr.noisy_reads(7)
    weights = np.ones(len(reads), dtype=np.uint32)
    weights[0], weights[1], weights[2] = 70000, 13, 300
    expanded = kr.count(reads, k, True)
    for r, w in ((reads[0], 70000 - 1), (reads[1], 13 - 1), (reads[2], 300 - 1)):
        for key, n in kr.count([r], k, True).items():
            expanded[key] += n * w
    return reads, weights, expanded


def test_clips_and_the_lds_edge(hip_lib):
    """rows, cols of 1, 2, exactly the LDS rectangle, one more than it, and unclipped, with counts far beyond any
    private bin on one side (weights 13 and 70 000; 300: beyond the rectangle's rows, short of the clip) and, from 700
    reads, counts beyond the rectangle's columns on the other."""
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads, weights, ref_a = weighted_case(k)
    ref_b = counted(k, True, 8, 700)
    rows_full, cols_full = jr.unclipped_shape(ref_a, ref_b)
    assert rows_full > 70000 and cols_full > LDS[1] + 1 and rows_full * cols_full <= 1 << 22
    assert any(LDS[0] <= n < 70000 for n in ref_a.values()) and max(ref_b.values()) > LDS[1]
    a, b = KmerCounts(k, canonical=True, min_slots=1024), KmerCounts(k, canonical=True, min_slots=1024)
    try:
        a.add_weighted(reads, weights)
        b.add_reads(jr.noisy_reads(8, n=700))
        shapes = [(1, 1), (1, 2), (2, 1), (2, 2), (1, cols_full), (rows_full, 1), LDS, (LDS[0] + 1, LDS[1] + 1),
                  (LDS[0], LDS[1] + 1), (LDS[0] + 1, LDS[1]), (LDS[0] - 1, LDS[1] - 1), (14, 70001)]
        check(a, b, ref_a, ref_b, shapes, "weighted A")          # (and unclipped: check adds it)
        check(b, a, ref_b, ref_a, [(LDS[1], LDS[0]), (LDS[1] + 1, LDS[0] + 1), (2, 2)], "weighted B")
    finally:
        a.close()
        b.close()


def test_occurrences_against_lookup(hip_lib):
    """sum over a and o >= 1 of a N[a][o] -- the occurrences in A's reads of keys B holds -- is the number of windows
    for which B.lookup(reads) answers an abundance of 1 or more: A counted from those reads, every read at least k long,
    the matrix unclipped."""
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads = jr.noisy_reads(1)
    assert min(len(r) for r in reads) >= k
    ref_a, ref_b = counted(k, True, 1), counted(k, True, 2)
    a, b = KmerCounts(k, canonical=True, min_slots=1024), KmerCounts(k, canonical=True, min_slots=1024)
    try:
        a.add_reads(reads)
        b.add_reads(jr.noisy_reads(2))
        got = a.join_histogram(b, *jr.unclipped_shape(ref_a, ref_b))
        abundance = b.lookup(reads).abundance
        windows = abundance[abundance != 0xFFFFFFFF]
        assert windows.size == sum(len(r) - k + 1 for r in reads)
        assert int((np.arange(got.shape[0]) @ got[:, 1:]).sum()) == int((windows >= 1).sum()) > 0
        assert int((np.arange(got.shape[0]) @ got[:, 0])) == int((windows == 0).sum()) > 0
    finally:
        a.close()
        b.close()


def test_refusals(hip_lib):
    """Every status of the host form, and of the device form where no device buffer is needed, with the call's name in
    the message."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    out = np.zeros(16, dtype=np.int64)
    a, b, wide, k20, forward = KmerCounts(21), KmerCounts(21), KmerCounts(32), KmerCounts(20), KmerCounts(21, canonical=False)
    canon = KmerCounts(21, canonical=True)

    def host(x, y, rows=4, cols=4, ptr=out.ctypes.data):
        return hip_lib.covest_kmer_join_histogram(x._handle if x is not None else None, y._handle if y is not None else None,
                                                  rows, cols, ptr)

    def device(x, y, rows=4, cols=4, ptr=None):
        return hip_lib.covest_kmer_join_histogram_device(x._handle if x is not None else None,
                                                         y._handle if y is not None else None, rows, cols, ptr, None)

    def refused(rc, code, name, *words):
        text = _capi.last_error()
        assert rc == code and text.startswith(name + ":") and all(w in text for w in words), (rc, text)
    try:
        for call, name in ((host, "covest_kmer_join_histogram"), (device, "covest_kmer_join_histogram_device")):
            refused(call(None, b), _capi.COVEST_E_INVALID, name, "null counter")
            refused(call(a, None), _capi.COVEST_E_INVALID, name, "null counter")
            refused(call(a, a), _capi.COVEST_E_INVALID, name, "same counter")
            refused(call(wide, b), _capi.COVEST_E_UNSUPPORTED, name, "at most 31")
            refused(call(a, wide), _capi.COVEST_E_UNSUPPORTED, name, "at most 31")
            refused(call(wide, k20), _capi.COVEST_E_UNSUPPORTED, name, "at most 31")
            refused(call(a, k20), _capi.COVEST_E_INVALID, name, "differ in k")
            refused(call(canon, forward), _capi.COVEST_E_INVALID, name, "canonical")
            for rows, cols in ((0, 4), (4, 0), (-1, 4), (4, -1), (2049, 2048), ((1 << 22) + 1, 1), (1, (1 << 22) + 1),
                               (1 << 40, 1 << 40), (-(1 << 63), -(1 << 63))):
                refused(call(a, b, rows, cols), _capi.COVEST_E_INVALID, name, "2^22")
            refused(call(a, b, 4, 4, None), _capi.COVEST_E_INVALID, name, "output")
        assert host(a, b) == 0 and not out.any()
        if _capi.device_count() >= 2:
            elsewhere = KmerCounts(21, device=1)
            refused(host(a, elsewhere), _capi.COVEST_E_INVALID, "covest_kmer_join_histogram", "device")
            elsewhere.close()
        closed = KmerCounts(21)
        closed.close()
        with pytest.raises(_capi.CovestHipError, match="null counter"):
            a.join_histogram(closed, 2, 2)
        with pytest.raises(TypeError):
            a.join_histogram("reads", 2, 2)
        with pytest.raises(_capi.CovestHipError, match="2\\^22"):
            a.join_histogram(b, 2049, 2048)
    finally:
        for c in (a, b, wide, k20, forward, canon):
            c.close()


def test_overflow_is_sticky_in_the_host_form(hip_lib):
    """The host form answers COVEST_E_NOMEM while either counter carries an overflow, until that counter is cleared."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    k = 12
    reads = jr.noisy_reads(5, n=40)
    assert len(kr.count(reads, k, True)) > 1024 + 200
    full, ok = KmerCounts(k, canonical=True, min_slots=1024), KmerCounts(k, canonical=True, min_slots=1024)
    out = np.zeros(4, dtype=np.int64)
    try:
        with pytest.raises(_capi.CovestHipError):
            add_without_reserve(full, reads)
        ok.add_reads(jr.noisy_reads(3, n=7))
        for x, y in ((full, ok), (ok, full)):
            rc = hip_lib.covest_kmer_join_histogram(x._handle, y._handle, 2, 2, out.ctypes.data)
            assert rc == _capi.COVEST_E_NOMEM and _capi.last_error().startswith("covest_kmer_join_histogram:"), rc
        full.clear()
        ref = counted(k, True, 3, 7)
        assert np.array_equal(ok.join_histogram(full, 3, 3), jr.join(ref, {}, 3, 3))
    finally:
        full.close()
        ok.close()


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import numpy as np
import join_reference as jr
import kmer_reference as kr
from covest_amd import _capi, kmer_hist as kh
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
k = 21
PAT, PAD = 0x25A5A5A5A5A5A5A5, 16
ref_a, ref_b = kr.count(jr.noisy_reads(1), k, True), kr.count(jr.noisy_reads(2), k, True)
a, b = kh.KmerCounts(k, canonical=True, min_slots=1024), kh.KmerCounts(k, canonical=True, min_slots=1024)
a.add_reads(jr.noisy_reads(1))
b.add_reads(jr.noisy_reads(2))


def run(rows, cols, fill):
    # the device form into rows * cols words between guard words; `fill`: what the words hold before the call
    buf = torch.full((PAD + rows * cols + PAD,), PAT, dtype=torch.int64, device=dev)
    buf[PAD:PAD + rows * cols] = fill
    a.join_histogram_device(b, rows, cols, buf.data_ptr() + 8 * PAD, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:PAD] == PAT).all() and (got[PAD + rows * cols:] == PAT).all(), ("stray write", rows, cols)
    return got[PAD:PAD + rows * cols].reshape(rows, cols)


for rows, cols in ((1, 1), (3, 5), (256, 16), (257, 17), jr.unclipped_shape(ref_a, ref_b)):
    want = jr.join(ref_a, ref_b, rows, cols)
    first = run(rows, cols, 0)
    assert np.array_equal(first, want), ("zeroed", rows, cols)
    assert np.array_equal(run(rows, cols, -7), want), ("garbage", rows, cols)          # the call zeroes its output
    assert np.array_equal(run(rows, cols, 1 << 40), first), ("twice", rows, cols)
# two calls in a row into ONE buffer, no synchronisation between them
buf = torch.full((PAD + 12 + PAD,), PAT, dtype=torch.int64, device=dev)
for _ in range(2):
    a.join_histogram_device(b, 3, 4, buf.data_ptr() + 8 * PAD, stream=stream)
torch.cuda.synchronize()
got = buf.cpu().numpy()
assert np.array_equal(got[PAD:PAD + 12].reshape(3, 4), jr.join(ref_a, ref_b, 3, 4)) and (got[:PAD] == PAT).all()
assert (got[PAD + 12:] == PAT).all()
print("device form ok")

# statuses that need device buffers: a misaligned output, a counter after the partitioned count (either side)
L = _capi.lib()
name = "covest_kmer_join_histogram_device"
for shift in (1, 2, 4, 7):
    rc = L.covest_kmer_join_histogram_device(a._handle, b._handle, 3, 4, buf.data_ptr() + 8 * PAD + shift, stream)
    assert rc == _capi.COVEST_E_INVALID and _capi.last_error().startswith(name + ":") and "aligned" in _capi.last_error(), rc
d_reads = torch.from_numpy(np.frombuffer("".join(kr.genome_reads(__import__("random").Random(5), 300, 100)).encode(),
                                         dtype=np.uint8).copy()).to(dev)
bulk = kh.KmerCounts(k, canonical=True)
path = bulk.count_reads_device(d_reads.data_ptr(), 300, 100, stream=stream)
assert path == "partitioned", (path, getattr(bulk, "why_not_partitioned", None))
out = np.zeros(12, dtype=np.int64)
for x, y in ((bulk, a), (a, bulk)):
    rc = L.covest_kmer_join_histogram_device(x._handle, y._handle, 3, 4, buf.data_ptr() + 8 * PAD, stream)
    assert rc == _capi.COVEST_E_INVALID and _capi.last_error().startswith(name + ":"), (rc, _capi.last_error())
    assert "covest_kmer_count_reads_device result" in _capi.last_error()
    rc = L.covest_kmer_join_histogram(x._handle, y._handle, 3, 4, out.ctypes.data)
    assert rc == _capi.COVEST_E_INVALID and "covest_kmer_count_reads_device result" in _capi.last_error(), rc
torch.cuda.synchronize()
assert np.array_equal(buf.cpu().numpy(), got), "a refused call wrote"
bulk.clear(stream)
bulk.add_device(d_reads.data_ptr(), 300, 100, stream=stream)
bulk.join_histogram_device(a, 3, 4, buf.data_ptr() + 8 * PAD, stream=stream)
torch.cuda.synchronize()
assert buf.cpu().numpy()[PAD:PAD + 12].sum() > 0
for c in (a, b, bulk):
    c.close()
print("statuses ok")
print("join device forms ok")
"""


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): guard words either side of the output untouched, an output full of garbage
    gives the same result (the call zeroes it), two calls in a row give equal results, and the statuses that need device
    buffers (a misaligned output, a counter after the partitioned count on either side)."""
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "join device forms ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


def test_genome_counts(hip_lib):
    """simulate.genome_counts leaves open the table genome_spectrum counts: the same spectrum, forward and canonical,
    a genome of more than one window, one shorter than k."""
    from covest_amd import simulate as sim
    g = sim.repeat_genome(150_000, 250, 0.7, 0.5, 0.5, 3)
    for k, canonical in ((21, False), (21, True), (12, True)):
        counts = sim.genome_counts(g, k, canonical=canonical)
        try:
            hist = counts.histogram()
            assert {o: v for o, v in enumerate(hist) if o > 0 and v > 0} == sim.genome_spectrum(g, k, canonical=canonical)
            assert counts.k == k and counts.canonical == canonical
        finally:
            counts.close()
    empty = sim.genome_counts("ACGT", 21)
    try:
        assert len(empty) == 0 and sim.genome_spectrum("ACGT", 21) == {}
    finally:
        empty.close()
    with pytest.raises(ValueError):
        sim.genome_counts("ACGN", 2)


def test_copy_spectrum_end_to_end(hip_lib):
    """A 20 000-base repeat genome and error-free reads of it: no k-mer of the reads is outside the genome (column 0 is
    exactly zero for every a >= 1), the column sums are the genome's own spectrum, the row sums the reads' histogram."""
    from covest_amd import copy_spectrum, simulate as sim
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    g = sim.repeat_genome(20_000, 250, 0.7, 0.5, 0.5, 11)
    reads = sim.simulate_reads(g.bases, 100, coverage=15, error_rate=0.0, seed=11, both_strands=False)
    counts = reads.add_to(KmerCounts(k, canonical=False))
    truth = sim.genome_counts(g, k, canonical=False)
    try:
        s = copy_spectrum(counts, truth)
        assert s.matrix.shape == (counts.stats()[0], truth.stats()[0]) and s.matrix[0, 0] == 0
        assert not s.matrix[1:, 0].any() and s.observed_kmers()["erroneous"] == 0
        assert s.genome_spectrum() == sim.genome_spectrum(g, k, canonical=False)
        assert s.abundance_histogram().tolist() == counts.histogram()
        assert s.matrix.sum() == len(truth) and s.matrix[1:].sum() == len(counts)
        assert s.error_cutoff() == 1 and max(s.genome_spectrum()) >= 3
        clipped_s = copy_spectrum(counts, truth, max_abundance=30, max_copies=2)
        assert clipped_s.matrix.shape == (31, 3) and clipped_s.matrix.sum() == s.matrix.sum()
        assert np.array_equal(clipped_s.matrix[:30, :2], s.matrix[:30, :2])
        noisy = sim.simulate_reads(g.bases, 100, coverage=15, error_rate=0.02, seed=12, both_strands=False)
        noisy_counts = noisy.add_to(KmerCounts(k, canonical=False))
        try:
            with_errors = copy_spectrum(noisy_counts, truth)
            assert with_errors.matrix[1:, 0].sum() > 0 and with_errors.error_share()[1] > 0.9
            assert with_errors.genome_spectrum() == s.genome_spectrum()
        finally:
            noisy_counts.close()
    finally:
        counts.close()
        truth.close()
