"""The per-read k-mer lookup on the device (kmer_lookup.hip through KmerCounts.lookup and the C ABI) against its plain
Python restatement (tests/lookup_reference.py): abundance, summary and score equal bit for bit, whatever the key width,
the shape of the reads, the fill of the table or the alignment of the caller's buffers.

Host forms run in this process.  What needs device buffers runs in ONE fresh child process with torch imported first (one
HIP runtime a process), as tests/test_gpu_simulate.py does.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_reference as kr
import lookup_reference as lr

pytestmark = pytest.mark.gpu

WEIGHTS = np.array([3.25, -1e-3, 0.1, 7.0e5, 2.0 ** -30, -0.7, 1.0 / 3.0])  # a fixed irregular table of 7 doubles
CUTOFF = 2


def check_equal(got, want, where):
    """A ReadAbundances against lr.lookup's (abundance, offsets, summary, score): every bit."""
    abundance, offsets, summary, score = want
    assert np.array_equal(got.offsets, offsets), where
    assert got.abundance.dtype == np.uint32 and np.array_equal(got.abundance, abundance), where
    assert np.array_equal(got.summary, summary), where
    for j, name in enumerate(("min_abundance", "weak", "first_weak", "last_weak")):
        assert np.array_equal(getattr(got, name), lr.signed(summary[:, j])), (where, name)
    if score is None:
        assert got.score is None, where
    else:
        assert got.score.dtype == np.float64 and np.array_equal(got.score.view(np.uint64), score.view(np.uint64)), where
    for i in sorted({0, (len(offsets) - 1) // 2, len(offsets) - 2}):  # the first read, one in the middle, the last
        n_windows = max(int(offsets[i + 1] - offsets[i]) - got.k + 1, 0)
        assert np.array_equal(got.windows(i), abundance[offsets[i]:offsets[i] + n_windows]), (where, i)


def add_without_reserve(counts, reads):
    """covest_kmer_add as it stands: the table keeps the size it was created with."""
    from covest_amd import _capi
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    _capi.check(_capi.lib().covest_kmer_add(counts._handle, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(reads)),
                "covest_kmer_add")


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 12, 13, 31])
def test_exact(hip_lib, k, canonical):
    """Every key width's paths (k = 12: no first slot; 13: the smallest with one; 31: the widest word), keys that collide
    in the first slot by construction (probe_reads: pairs that differ by one base mostly share minimizer and position),
    a table that grew with keys in it, absent keys, an empty read and one of k - 1 bases."""
    from covest_amd.kmer_hist import KmerCounts
    batches = kr.sweep_batches(k) + [list(kr.probe_reads(k))]
    counted = [r for b in batches for r in b]
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        for b in batches:
            counts.add_reads(b)
        reads = counted + kr.device_ragged_reads(k)
        want = lr.lookup(reads, kr.count(counted, k, canonical), k, canonical, CUTOFF, WEIGHTS)
        assert (want[2][:, 0] == lr.NONE).any() and (k == 1 or (want[0] == 0).any())  # no window; absent keys
        check_equal(counts.lookup(reads, cutoff=CUTOFF, weights=WEIGHTS), want, (k, canonical))
        got = counts.lookup(reads, cutoff=CUTOFF, per_window=False)
        assert got.abundance is None and got.score is None and np.array_equal(got.summary, want[2])
    finally:
        counts.close()


def _slot_of(key, log2_slots):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - log2_slots)  # slot_of, csrc/kmer_table.h


def test_probe_wraps(hip_lib):
    """k = 12 (no first slot), forward strand, 1 024 slots: six keys whose plain slot is 1 022 or 1 023 fill the table's
    end and wrap to its start; two absent keys with the same slots are probed round the end to an empty slot."""
    from covest_amd.kmer_hist import KmerCounts
    k, lg = 12, 10
    keys = [key for key in range(1, 200_000) if _slot_of(key, lg) >= 1022][:8]
    assert len(keys) == 8 and {_slot_of(key, lg) for key in keys} == {1022, 1023}
    kmers = ["".join("ACGT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k)) for key in keys]
    present, absent = kmers[:6], kmers[6:]
    counts = KmerCounts(k, canonical=False, min_slots=1024)
    try:
        assert counts.slots == 1024
        add_without_reserve(counts, [kmer for n, kmer in enumerate(present, 1) for _ in range(n)])
        assert counts.slots == 1024 and len(counts) == 6
        got = counts.lookup(present + absent, cutoff=3)
        assert [int(got.windows(i)[0]) for i in range(8)] == [1, 2, 3, 4, 5, 6, 0, 0]
        assert got.weak.tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
        want = lr.lookup(present + absent, kr.count([kmer for n, kmer in enumerate(present, 1) for _ in range(n)], k), k,
                         False, 3)
        check_equal(got, want, "wrap")
    finally:
        counts.close()


def test_full_table_and_after_reserve(hip_lib):
    """A 1 024-slot table at the contract's limit (500 distinct 21-mers, no reserve), looked up exactly; then the same
    answers from the 4 096-slot table covest_kmer_reserve re-inserted them into."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    g = kr.genome()
    counted = [g[:520], g[100:300], g[250:520].lower(), kr.revcomp(g[40:90])]
    reads = counted + [g[1000:1100], g[500:560], "", g[:20]]
    table = kr.count(counted, k, True)
    assert len(table) == 500
    want = lr.lookup(reads, table, k, True, CUTOFF, WEIGHTS)
    counts = KmerCounts(k, canonical=True, min_slots=1024)
    try:
        add_without_reserve(counts, counted)
        assert counts.slots == 1024 and len(counts) == 500
        check_equal(counts.lookup(reads, cutoff=CUTOFF, weights=WEIGHTS), want, "1024 slots")
        _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 4096), "covest_kmer_reserve")
        assert counts.slots == 4096 and len(counts) == 500
        check_equal(counts.lookup(reads, cutoff=CUTOFF, weights=WEIGHTS), want, "4096 slots")
    finally:
        counts.close()


SHAPES_K = 21


def shape_lengths(k):
    return [n for n in kr.sweep_lengths(k) if n in (k, k + 63, k + 64, k + 65, 2 * k + 200)]


@functools.lru_cache(maxsize=None)
def genome_counts(k):
    return kr.count([kr.genome()], k, True)


def test_wave_shapes(hip_lib):
    """Reads of k, k + 63, k + 64, k + 65 and 2k + 200 bases (a lane's first, last and second round), 1, 3, 4 and 5 of
    them (a workgroup is four reads), with offsets that start at 5."""
    import random
    from covest_amd.kmer_hist import KmerCounts
    k = SHAPES_K
    rng = random.Random(77)
    counts = KmerCounts(k, canonical=True)
    try:
        counts.add_reads([kr.genome()])
        for length in shape_lengths(k):
            for n in (1, 3, 4, 5):
                reads = kr.genome_reads(rng, n, length)
                want = lr.lookup(reads, genome_counts(k), k, True, CUTOFF, WEIGHTS)
                check_equal(counts.lookup(reads, cutoff=CUTOFF, weights=WEIGHTS), want, (length, n))
                blob = np.frombuffer(("NNNNN" + "".join(reads) + "NN").encode(), dtype=np.uint8)
                got = counts.lookup((blob, want[1] + 5), cutoff=CUTOFF, weights=WEIGHTS)
                check_equal(got, want, (length, n, "offsets from 5"))
        assert len(shape_lengths(k)) == 5
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
import lookup_reference as lr
from covest_amd import _capi, kmer_hist as kh
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
k, CUTOFF = 21, 2
WEIGHTS = np.array([3.25, -1e-3, 0.1, 7.0e5, 2.0 ** -30, -0.7, 1.0 / 3.0])
table = kr.count([kr.genome()], k, True)
d_weights = torch.from_numpy(WEIGHTS).to(dev)
d_genome = torch.from_numpy(np.frombuffer(kr.genome().encode(), dtype=np.uint8).copy()).to(dev)
counts = kh.KmerCounts(k, canonical=True, min_slots=1 << 14)
counts.add_device(d_genome.data_ptr(), 1, len(kr.genome()), stream=stream, reserve=False)
PAT32, PATF = 0xA5A5A5A5, -1.2345e300
PAD = 16


def run(reads, fixed_len, shift, want_a=True, want_s=True, want_f=True):
    # the device form on `reads` whose bases start `shift` bytes into an aligned buffer: (abundance, summary, score),
    # None for what was not asked for; canaries either side of every output checked
    blob = np.frombuffer(("N" * shift + "".join(reads)).encode(), dtype=np.uint8).copy()
    d_bases = torch.from_numpy(blob).to(dev)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    d_offsets = torch.from_numpy(offsets).to(dev)
    n, n_pos = len(reads), int(offsets[-1])
    a = torch.from_numpy(np.full(PAD + n_pos + PAD, PAT32, dtype=np.uint32).view(np.int32)).to(dev)
    s = torch.from_numpy(np.full(PAD + 4 * n + PAD, PAT32, dtype=np.uint32).view(np.int32)).to(dev)
    f = torch.full((PAD + n + PAD,), PATF, dtype=torch.float64, device=dev)
    counts.lookup_device(d_bases.data_ptr() + shift, n, fixed_len if fixed_len is not None else 0,
                         d_offsets_ptr=None if fixed_len is not None else d_offsets.data_ptr(), cutoff=CUTOFF,
                         d_weights_ptr=d_weights.data_ptr() if want_f else None, n_weights=len(WEIGHTS) if want_f else 0,
                         d_abundance_ptr=a.data_ptr() + 4 * PAD if want_a else None,
                         d_summary_ptr=s.data_ptr() + 4 * PAD if want_s else None,
                         d_score_ptr=f.data_ptr() + 8 * PAD if want_f else None, stream=stream)
    torch.cuda.synchronize()
    a, s, f = a.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32), f.cpu().numpy()
    where = (len(reads), fixed_len, shift, want_a, want_s, want_f)
    assert (a[:PAD] == PAT32).all() and (a[PAD + n_pos:] == PAT32).all(), ("stray abundance", where)
    assert (s[:PAD] == PAT32).all() and (s[PAD + 4 * n:] == PAT32).all(), ("stray summary", where)
    assert (f[:PAD] == PATF).all() and (f[PAD + n:] == PATF).all(), ("stray score", where)
    if not want_a:
        assert (a == PAT32).all(), ("abundance written though null", where)
    if not want_s:
        assert (s == PAT32).all(), ("summary written though null", where)
    if not want_f:
        assert (f == PATF).all(), ("score written though null", where)
    return (a[PAD:PAD + n_pos] if want_a else None, s[PAD:PAD + 4 * n].reshape(n, 4) if want_s else None,
            f[PAD:PAD + n] if want_f else None)


def same(got, want, where):
    abundance, _, summary, score = want
    if got[0] is not None:
        assert np.array_equal(got[0], abundance), ("abundance", where)
    if got[1] is not None:
        assert np.array_equal(got[1], summary), ("summary", where)
    if got[2] is not None:
        assert np.array_equal(got[2].view(np.uint64), score.view(np.uint64)), ("score", where)


rng = random.Random(99)
# reads of their own lengths (an empty one, one shorter than k), d_bases at byte offsets 0, 1, 3; each output null in
# turn, and alone: what is asked for does not depend on what else is
ragged = kr.genome_reads(rng, 2, k + 70) + ["", kr.genome()[:k - 1], "ACGT" * 30] + kr.genome_reads(rng, 4, 2 * k + 200)
want = lr.lookup(ragged, table, k, True, CUTOFF, WEIGHTS)
for shift in (0, 1, 3):
    same(run(ragged, None, shift), want, ("ragged", shift))
for asked in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False),
              (False, False, True)):
    same(run(ragged, None, 1, *asked), want, ("ragged", asked))
print("device form ok")

# reads of one length without offsets against the same reads with them: every shape of the wave
for length in (k, k + 63, k + 64, k + 65, 2 * k + 200, k - 1):
    for n in (1, 3, 4, 5):
        reads = kr.genome_reads(rng, n, length)
        want = lr.lookup(reads, table, k, True, CUTOFF, WEIGHTS)
        fixed, with_offsets = run(reads, length, 3), run(reads, None, 3)
        same(fixed, want, ("fixed", length, n))
        same(with_offsets, want, ("offsets", length, n))
print("fixed length ok")

# statuses that need device buffers
L = _capi.lib()
d_reads = torch.from_numpy(np.frombuffer("".join(kr.genome_reads(rng, 300, 100)).encode(), dtype=np.uint8).copy()).to(dev)
d_summary = torch.zeros(4 * 300, dtype=torch.int32, device=dev)
d_score = torch.zeros(300, dtype=torch.float64, device=dev)
rc = L.covest_kmer_lookup_reads_device(counts._handle, d_reads.data_ptr(), None, 300, 100, 2, None, 0, None,
                                       d_summary.data_ptr(), d_score.data_ptr(), stream)
assert rc == _capi.COVEST_E_INVALID and "weight" in _capi.last_error(), (rc, _capi.last_error())
rc = L.covest_kmer_lookup_reads_device(counts._handle, d_reads.data_ptr(), None, 300, 100, 2, d_weights.data_ptr(), 0, None,
                                       d_summary.data_ptr(), d_score.data_ptr(), stream)
assert rc == _capi.COVEST_E_INVALID, rc
rc = L.covest_kmer_lookup_reads_device(counts._handle, d_reads.data_ptr(), None, 300, -1, 2, None, 0, None,
                                       d_summary.data_ptr(), None, stream)
assert rc == _capi.COVEST_E_INVALID, rc
rc = L.covest_kmer_lookup_reads_device(counts._handle, None, None, 0, 100, 2, None, 0, None, d_summary.data_ptr(), None,
                                       stream)
assert rc == 0, rc
torch.cuda.synchronize()
assert not d_summary.cpu().numpy().any(), "n_reads == 0 launched something"
wide = kh.KmerCounts(32)
rc = L.covest_kmer_lookup_reads_device(wide._handle, d_reads.data_ptr(), None, 300, 100, 2, None, 0, None,
                                       d_summary.data_ptr(), None, stream)
assert rc == _capi.COVEST_E_UNSUPPORTED, rc
wide.close()
bulk = kh.KmerCounts(k, canonical=True)
path = bulk.count_reads_device(d_reads.data_ptr(), 300, 100, stream=stream)
assert path == "partitioned", (path, getattr(bulk, "why_not_partitioned", None))
rc = L.covest_kmer_lookup_reads_device(bulk._handle, d_reads.data_ptr(), None, 300, 100, 2, None, 0, None,
                                       d_summary.data_ptr(), None, stream)
assert rc == _capi.COVEST_E_INVALID and "covest_kmer_count_reads_device result" in _capi.last_error(), (rc, _capi.last_error())
bulk.clear(stream)
bulk.add_device(d_reads.data_ptr(), 300, 100, stream=stream)
bulk.lookup_device(d_reads.data_ptr(), 300, 100, cutoff=2, d_summary_ptr=d_summary.data_ptr(), stream=stream)
torch.cuda.synchronize()
assert (d_summary.cpu().numpy().reshape(300, 4)[:, 0] >= 1).all(), "a counted read's k-mers are all in the table"
bulk.close()
counts.close()
print("statuses ok")
print("lookup device forms ok")
"""


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): d_bases at byte offsets 0, 1 and 3, canaries either side of all three
    outputs, each output null in turn, reads of one length against the same reads with offsets, and the statuses that
    need device buffers (a counter after the partitioned count among them)."""
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "lookup device forms ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


def test_statuses(hip_lib):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    u8, i64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)
    blob = np.frombuffer(b"ACGT" * 20, dtype=np.uint8)
    offsets = np.array([0, 80], dtype=np.int64)
    summary = np.zeros((1, 4), dtype=np.uint32)
    score = np.zeros(1, dtype=np.float64)

    def call(counts, n, weights, n_weights, score_out):
        return hip_lib.covest_kmer_lookup_reads(
            counts._handle if counts is not None else None, blob.ctypes.data, offsets.ctypes.data, n, 2,
            weights.ctypes.data if weights is not None else None, n_weights, None, summary.ctypes.data,
            score_out.ctypes.data if score_out is not None else None)
    wide, counts = KmerCounts(32), KmerCounts(21)
    try:
        assert call(wide, 1, None, 0, None) == _capi.COVEST_E_UNSUPPORTED
        with pytest.raises(_capi.CovestHipError, match=r"\(-5\)"):
            wide.lookup(["ACGT" * 20])
        assert call(counts, 1, None, 0, score) == _capi.COVEST_E_INVALID      # a score without weights
        assert call(counts, 1, WEIGHTS, 0, score) == _capi.COVEST_E_INVALID   # ... with an empty table
        assert call(counts, -1, None, 0, None) == _capi.COVEST_E_INVALID
        assert call(None, 1, None, 0, None) == _capi.COVEST_E_INVALID
        assert call(counts, 0, None, 0, None) == 0 and not summary.any()      # no reads: OK, nothing written
        assert call(counts, 1, WEIGHTS, len(WEIGHTS), score) == 0             # an empty table: every k-mer absent
        assert summary.tolist() == [[0, 60, 0, 59]] and score[0] == lr.butterfly_sum([WEIGHTS[0]] * 60)
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
            counts.lookup([kr.genome()[:100]])
    finally:
        counts.close()


# ---- the simulated case of DESIGN.md section 6ae on the device ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_case():
    """(genome, SimulatedReads, KmerCounts that hold them) of lookup_reference.CASE, made on the device; shared."""
    from covest_amd import kmer_hist as kh, simulate as sim
    c = lr.CASE
    genome = sim.random_genome(c["genome_len"], c["seed"])
    reads = sim.simulate_reads(genome, c["read_len"], n_reads=c["n_reads"], error_rate=c["error_rate"], seed=c["seed"])
    return genome, reads, reads.add_to(kh.KmerCounts(c["k"], canonical=True))


def test_simulated_case(hip_lib):
    c, want = lr.CASE, lr.CASE_EXPECTED
    genome, reads, counts = device_case()
    hit = reads.bases != reads.error_free(genome)
    assert np.array_equal(hit, lr.simulated_case()[2])
    got = counts.lookup(reads, cutoff=c["cutoff"])
    assert np.array_equal(got.summary, lr.simulated_case_summary())
    flagged = got.weak > 0
    assert np.array_equal(flagged, lr.simulated_case_summary()[:, 1] > 0)
    n_wrong, n_flagged, missed, false, sens, spec = lr.detection_figures(flagged, hit)
    print("reads with a substitution %d, flagged %d, missed %d, falsely flagged %d, sensitivity %.4f, specificity %.4f"
          % (n_wrong, n_flagged, missed, false, sens, spec))
    assert (missed, false) == (want["missed"], want["false"]) == (1, 3)
    assert sens >= 0.99 and spec >= 0.99


def test_end_to_end(hip_lib):
    """The same reads' histogram fitted by the basic model (the flow of tests/flow_helper.py), read_error_scores at
    level 0.5: the fitted cutoff lies between the errors and the genomic mode, the flags and the scores equal the
    restatement's at that cutoff with the weights the call built, and print_output carries the record."""
    from covest_amd import constants, posterior_classes, print_output, read_error_scores
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    c = lr.CASE
    k, read_len = c["k"], c["read_len"]
    _, reads, counts = device_case()
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    # sample factor 1: the table's abundances are those of the whole read set, so the model is fitted to them as they are
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, k, read_len, sample_factor=1)
    assert sample_factor == 1
    model = select_model("basic")(k, read_len, hist, tail, max_error=constants.MAX_ERRORS)
    guess = [guess_c, guess_e]
    estimate, success = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage(guess)
    scores = read_error_scores(model, estimate, counts, reads, level=0.5)
    print("estimate", list(estimate), "fitted cutoff", scores.cutoff)
    assert 2 <= scores.cutoff < 30 * 48 / 64  # above the errors (abundance 1), below the genomic mode
    assert scores.cutoff == posterior_classes(model, estimate).error_cutoff(0.5)
    _, _, _, strings, table = lr.simulated_case()
    _, _, summary, score = lr.lookup(strings, table, k, True, scores.cutoff, scores.weights)
    assert np.array_equal(scores.flagged, summary[:, 1] > 0)
    for j, name in enumerate(("min_abundance", "weak", "first_weak", "last_weak")):
        assert np.array_equal(getattr(scores, name), lr.signed(summary[:, j])), name
    assert np.array_equal(scores.expected_erroneous_kmers.view(np.uint64), score.view(np.uint64))
    assert np.array_equal(scores.locate_single_errors(),
                          lr.locate_single_errors(k, scores.lengths, *(lr.signed(summary[:, j]) for j in (1, 2, 3))))
    plain = print_output(hist_orig, model, success, sample_factor, estimate, guess, silent=True)
    record = print_output(hist_orig, model, success, sample_factor, estimate, guess, silent=True, read_errors=scores)
    added = {"read_errors_" + name for name in ("cutoff", "level", "reads", "flagged_share", "predicted_share",
                                                "mean_expected_erroneous_kmers")}
    assert set(record) - set(plain) == added and {key: record[key] for key in plain} == plain
    assert record["read_errors_cutoff"] == scores.cutoff and record["read_errors_reads"] == c["n_reads"]
    assert record["read_errors_level"] == 0.5
    assert record["read_errors_flagged_share"] == float((summary[:, 1] > 0).mean())
    assert record["read_errors_predicted_share"] == pytest.approx(1 - (1 - estimate[1]) ** read_len, rel=1e-12)
    assert record["read_errors_mean_expected_erroneous_kmers"] == pytest.approx(float(score.mean()), rel=1e-12)
    print("flagged share %.4f, predicted share %.4f (not the same quantity: DESIGN.md section 6ae)"
          % (scores.flagged_share, scores.predicted_share))
    with pytest.raises(ValueError):
        read_error_scores(model, estimate, counts, reads, level=0.0)  # no key's erroneous share is below 0
