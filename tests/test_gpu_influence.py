"""The delete-one-read influence on the device (kmer_influence.hip through KmerCounts.read_influence, covest_amd.influence
and the C ABI) against its plain Python restatement (tests/influence_reference.py): the rows equal bit for bit whatever
the shape of the reads, the multiplicity of their keys, the table or the alignment of the caller's buffers; the moments
within the bound of an n-term sum and the same bits on every run; and the identity behind the rows through the model,
against leave-one-read-out histograms.

Host forms run in this process.  What needs device buffers runs in ONE fresh child process with torch imported first (one
HIP runtime a process), as tests/test_gpu_lookup.py does.
"""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import influence_reference as ir
import kmer_reference as kr
import lookup_reference as lr
from covest_amd import influence as infl

pytestmark = pytest.mark.gpu


def same_bits(got, want, where):
    assert got.dtype == np.float64 and got.shape == want.shape, where
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (where, got, want)


def make_table(n_rows, n_cols, seed=3):
    """A fixed irregular table: columns of very different scale, both signs."""
    rng = np.random.default_rng(seed + 100 * n_rows + n_cols)
    return rng.normal(size=(n_rows, n_cols)) * (10.0 ** rng.integers(-6, 7, size=n_cols))


def shape_reads(k):
    """(counted, reads): what the table is counted from, and the reads whose rows are asked for.

    Windows 0 (a read of k - 1 bases, and an empty one), 1, 63, 64, 65, 128, 129; a homopolymer of 71 windows (m = W,
    over two chunks) of which the table holds 3 (a < m); a segment repeated 93 + k bases on (the two windows of a key in
    different lanes and different 64-window chunks); a segment and its reverse complement (one key only if canonical);
    reads counted exactly once (a - m = 0); reads that were never counted (a = 0); the genome counted six times
    (a >= n_rows for the small tables)."""
    g = kr.genome()
    by_windows = [g[200 + 7 * w:200 + 7 * w + w + k - 1] for w in (0, 1, 63, 64, 65, 128, 129)]
    homopolymer = "A" * (k + 70)
    seg = g[1500:1500 + k + 3]
    twice = seg + g[1600:1690] + seg
    both_strands = seg + g[1700:1790] + kr.revcomp(seg)
    import random
    fresh = kr._random_bases(random.Random(4242), k + 140)  # (for k > 12 none of its keys is in the genome)
    once = kr._random_bases(random.Random(4243), k + 80)
    # (k = 1 has four keys: a short count keeps their abundances within the tables' rows and below the multiplicities)
    counted = [g] * 5 + [g.lower(), "A" * (k + 2), once, twice] if k > 1 else [g[:30], "AAA"]
    reads = by_windows + ["", homopolymer, twice, both_strands, once, fresh, g[:k + 30].lower()]
    return counted, reads


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 13, 31])
def test_rows_bit_for_bit(hip_lib, k, canonical):
    from covest_amd.kmer_hist import KmerCounts
    counted, reads = shape_reads(k)
    table_counts = kr.count(counted, k, canonical)
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        counts.add_reads(counted)
        terms = [ir.first_terms(r, table_counts, k, canonical, make_table(6, 1)) for r in reads]
        # the cases the list claims, as the restatement sees them
        assert any(m > 1 for t in terms for _, m, _, _ in t) and any(a < m for t in terms for _, m, a, _ in t)
        if k > 1:
            assert any(a == m for t in terms for _, m, a, _ in t) and any(a == 0 for t in terms for _, _, a, _ in t)
        assert any(a >= 6 for t in terms for _, _, a, _ in t)
        assert any(len(t) == 1 and t[0][1] == 71 for t in terms)  # the homopolymer: m = W
        for n_rows, n_cols in ((6, 1), (6, 2), (40, 5), (6, 8), (1, 2), (1, 8)):
            table = make_table(n_rows, n_cols)
            want = ir.influence_rows(reads, table_counts, k, canonical, table)
            assert n_rows == 1 or np.abs(want[:, :n_cols]).max() > 0
            same_bits(counts.read_influence(reads, table), want, (k, canonical, n_rows, n_cols))
        table = make_table(6, 2)
        want = ir.influence_rows(reads, table_counts, k, canonical, table)
        pick = [9, 8, 3, 10, 5]  # the repeated segment, the homopolymer, 64 windows, both strands, 128 windows
        for n in (1, 3, 4, 5):   # four reads a workgroup
            same_bits(counts.read_influence([reads[i] for i in pick[:n]], table), want[pick[:n]], (k, canonical, n))
        blob = np.frombuffer(("NNNNN" + "".join(reads) + "NN").encode(), dtype=np.uint8)
        offsets = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in reads], out=offsets[1:])
        same_bits(counts.read_influence((blob, offsets + 5), table), want, (k, canonical, "offsets from 5"))
    finally:
        counts.close()


def test_the_two_windows_of_a_key_sit_in_different_lanes_and_chunks():
    """What shape_reads claims about its repeated segment, from the restatement alone."""
    for k in (13, 31):
        _, reads = shape_reads(k)
        keys = ir.read_keys(reads[9], k, False)
        first, again = 0, keys.index(keys[0], 1)
        assert again == 93 + k and again // 64 != first // 64 and again % 64 != first % 64
        both = ir.read_keys(reads[10], k, True)
        assert both[0] in both[1:] and ir.read_keys(reads[10], k, False)[0] not in ir.read_keys(reads[10], k, False)[1:]


def test_too_many_windows_and_statuses(hip_lib):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    table = make_table(4, 2)
    rows = np.zeros((2, 3), dtype=np.float64)
    blob = np.frombuffer(("ACGT" * 2000).encode(), dtype=np.uint8)

    def call(counts, offsets, n, n_rows=4, n_cols=2, table_ptr=table.ctypes.data, rows_ptr=rows.ctypes.data):
        offsets = np.asarray(offsets, dtype=np.int64)
        return hip_lib.covest_kmer_read_influence(counts._handle if counts is not None else None, blob.ctypes.data,
                                                  offsets.ctypes.data, n, table_ptr, n_rows, n_cols, rows_ptr)
    wide, counts = KmerCounts(32), KmerCounts(k)
    try:
        counts.add_reads(["ACGT" * 30])
        assert call(counts, [0, 4096 + k - 1], 1) == 0 and rows[0, 2] == 4096.0 and np.isfinite(rows[0]).all()
        assert call(counts, [0, 100, 100 + 4097 + k - 1], 2) == _capi.COVEST_E_UNSUPPORTED  # 4097 windows
        assert "read 1 has 4097 windows" in _capi.last_error()
        with pytest.raises(_capi.CovestHipError, match=r"\(-5\)"):
            counts.read_influence(["ACGT" * 1030], table)
        assert call(wide, [0, 100], 1) == _capi.COVEST_E_UNSUPPORTED                       # k > 31
        with pytest.raises(_capi.CovestHipError, match=r"\(-5\)"):
            wide.read_influence(["ACGT" * 20], table)
        assert call(None, [0, 100], 1) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], -1) == _capi.COVEST_E_INVALID
        assert call(counts, [100, 0], 1) == _capi.COVEST_E_INVALID                         # bad offsets
        assert call(counts, [0, 100, 50], 2) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], 1, n_rows=0) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], 1, n_cols=0) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], 1, n_cols=9) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], 1, table_ptr=None) == _capi.COVEST_E_INVALID
        assert call(counts, [0, 100], 1, rows_ptr=None) == _capi.COVEST_E_INVALID
        rows[:] = 7.0
        assert call(counts, [0], 0) == 0 and (rows == 7.0).all()                           # no reads: OK, nothing written
        assert counts.read_influence([], table).shape == (0, 3)
        sums, cross = np.zeros(3), np.zeros(6)
        moments = hip_lib.covest_rows_moments
        assert moments(rows.ctypes.data, 2, 0, sums.ctypes.data, sums.ctypes.data, cross.ctypes.data) == _capi.COVEST_E_INVALID
        assert moments(rows.ctypes.data, 2, 10, sums.ctypes.data, sums.ctypes.data, cross.ctypes.data) == _capi.COVEST_E_INVALID
        assert moments(rows.ctypes.data, -1, 3, sums.ctypes.data, sums.ctypes.data, cross.ctypes.data) == _capi.COVEST_E_INVALID
        assert moments(None, 2, 3, sums.ctypes.data, sums.ctypes.data, cross.ctypes.data) == _capi.COVEST_E_INVALID
        assert moments(rows.ctypes.data, 2, 3, None, sums.ctypes.data, cross.ctypes.data) == _capi.COVEST_E_INVALID
    finally:
        wide.close()
        counts.close()


def test_overflowed_table_is_refused_by_the_host_form(hip_lib):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    counts = KmerCounts(21, min_slots=1024)
    try:
        blob = np.frombuffer(kr.genome().encode(), dtype=np.uint8)
        offsets = np.array([0, len(blob)], dtype=np.int64)
        rc = hip_lib.covest_kmer_add(counts._handle, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                     offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1)
        assert rc == _capi.COVEST_E_NOMEM  # 2 980 distinct 21-mers into 1 024 slots
        with pytest.raises(_capi.CovestHipError, match=r"\(-4\)"):
            counts.read_influence([kr.genome()[:100]], make_table(4, 2))
    finally:
        counts.close()


# ---- moments -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_rows():
    """(3000, 9) doubles, columns of different scale and offset; read-only.  Every case is a leading block of it."""
    rng = np.random.default_rng(11)
    rows = rng.normal(size=(3000, 9)) * np.array([1.0, 1e3, 1e-3, 50.0, 1.0, 1e6, 2.0, 0.5, 64.0]) + np.array(
        [0.0, 5e3, 0.0, -20.0, 1.0, 0.0, 0.0, 3.0, 40.0])
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("q", [1, 3, 6, 9])
def test_moments(hip_lib, q):
    """|sum_k - ref| <= n 2^-52 sum |u_k - m_k| and |cross_kl - ref| <= n 2^-52 sum |(u_k - m_k)(u_l - m_l)| against
    math.fsum -- the bound of an n-term floating-point sum in any order --, about zero and about a non-zero centre; the
    same bits from two runs."""
    for n in (0, 1, 255, 256, 257, 1023, 1024, 1025, 3000):
        rows = np.ascontiguousarray(moment_rows()[:n, :q])
        for centre in (None, np.ascontiguousarray(moment_rows()[:40, :q].mean(axis=0) + 0.125)):
            total, cross = infl.rows_moments(rows, centre)
            again = infl.rows_moments(rows, centre)
            same_bits(again[0], total, (n, q, "sum twice"))
            same_bits(again[1], cross, (n, q, "cross twice"))
            want_sum, want_cross, bound_sum, bound_cross = ir.moments(rows, np.zeros(q) if centre is None else centre)
            assert total.shape == (q,) and cross.shape == (q * (q + 1) // 2,)
            assert (np.abs(total - want_sum) <= bound_sum).all(), (n, q, total, want_sum, bound_sum)
            assert (np.abs(cross - want_cross) <= bound_cross).all(), (n, q, cross, want_cross, bound_cross)
            if n == 0:
                assert not total.any() and not cross.any() and not np.signbit(total).any()
            if n >= 255:  # (not vacuous: on the diagonal the bound is n 2^-52 of the value itself)
                diagonal = [ir.pair_index(q, a, a) for a in range(q)]
                assert (bound_cross[diagonal] < 1e-12 * np.abs(want_cross[diagonal])).all()


# ---- through the model ------------------------------------------------------------------------------------------------
def _as_hist(counts):
    return {i: int(v) for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}


@functools.lru_cache(maxsize=None)
def fitted(kind):
    """(reads (n, L) uint8, strings, KmerCounts, hist_orig, model, estimate) of lookup_reference.CASE's sizes -- 6 000
    bases, 2 812 reads of 64, e = 0.01, k = 17 canonical -- at sample factor 1: "basic" on the random genome of the
    case, "repeats" on a repeat_genome with the repeats model.  Shared, read-only."""
    from covest_amd import constants, kmer_hist as kh, simulate as sim
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    c = lr.CASE
    if kind == "basic":
        genome = sim.random_genome(c["genome_len"], c["seed"])
    else:
        genome = sim.repeat_genome(c["genome_len"], 150, 0.6, 0.5, 0.5, c["seed"]).bases
    reads = sim.simulate_reads(genome, c["read_len"], n_reads=c["n_reads"], error_rate=c["error_rate"], seed=c["seed"])
    counts = reads.add_to(kh.KmerCounts(c["k"], canonical=True))
    hist_orig = _as_hist(counts)
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, c["k"], c["read_len"], sample_factor=1)
    assert sample_factor == 1
    model = select_model(kind)(c["k"], c["read_len"], hist, tail, max_error=constants.MAX_ERRORS)
    guess = list(model.defaults)
    guess[:2] = guess_c, guess_e
    estimate, _ = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage(guess)
    strings = tuple(row.tobytes().decode() for row in reads.bases)
    return reads, strings, counts, hist_orig, model, [float(v) for v in estimate], genome


@functools.lru_cache(maxsize=None)
def influence_of(kind):
    reads, _, counts, _, model, estimate, _ = fitted(kind)
    return infl.read_influence(model, estimate, counts, reads)


@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_identity_through_the_model(hip_lib, kind):
    """grad L_(-r) - grad L, both from one HistogramBatch of the twin on the leave-one-read-out histogram (the host
    counter without read r) and the full one, equals the device's Delta_r within the contraction's bound 2 (n_keys + 2)
    2^-53 (sum_j h_j |g_k(j)| + tail |g_k,tail|) summed over both histograms plus the row's own W 2^-52 sum |terms|."""
    from covest_amd import jackknife
    from covest_amd.batch import HistogramBatch
    from covest_amd.kmer_hist import KmerCounts
    c = lr.CASE
    k = c["k"]
    reads, strings, counts, hist_orig, model, estimate, genome = fitted(kind)
    got = influence_of(kind)
    P = len(model.params)
    assert got.rows.shape == (c["n_reads"], P + 1) and (got.rows[:, P] == c["read_len"] - k + 1).all()
    assert got.occurrences_full == sum(i * v for i, v in hist_orig.items())
    table_counts = kr.count(strings, k, True)
    with_error = np.flatnonzero((reads.bases != reads.error_free(genome)).any(axis=1))
    chosen = [int(with_error[0])] + [r for r in (0, 1, 500, 1000, 1500, 2000, 2500, 2811) if r != int(with_error[0])][:7]
    assert len(chosen) == 8
    same_bits(got.rows[chosen], ir.influence_rows([strings[r] for r in chosen], table_counts, k, True, got.table), kind)

    trim = max(model.hist) + 1 if model.tail != 0 else None
    twin, table = infl.score_rows(model, estimate)
    try:
        same_bits(table, got.table, "table")
        keys = list(twin.hist.keys())
        assert keys == list(range(1, max(model.hist) + 1)) and table.shape == (len(keys) + 1 + (1 if trim else 0), P)
        g = np.abs(table[1:len(keys) + 1])                               # |g_k(j)| per key
        g_tail = np.abs(table[-1]) if trim else np.zeros(P)
        full_kept, full_tail = jackknife._cut(hist_orig, trim)
        scale = np.sqrt((got.rows[:, :P] ** 2).mean(axis=0))
        one = KmerCounts(k, canonical=True)
        try:
            for r in chosen:
                one.clear()
                one.add_reads(strings[:r] + strings[r + 1:])
                kept, tail = jackknife._cut(_as_hist(one), trim)
                h = np.array([[kept.get(j, 0) for j in keys], [full_kept.get(j, 0) for j in keys]], dtype=np.float64)
                tails = np.array([tail, full_tail], dtype=np.float64)
                batch = HistogramBatch(twin, h, tails)
                try:
                    _, grad = batch.loglikelihood_gradient_cross([estimate])
                finally:
                    batch.close()
                diff = grad[0, 0] - grad[1, 0]
                contraction = 2 * (len(keys) + 2) * 2.0 ** -53 * ((h @ g).sum(axis=0) + tails.sum() * g_tail)
                bound = contraction + ir.row_bound(strings[r], table_counts, k, True, table)
                delta = got.rows[r, :P]
                print("influence identity %s read %d: Delta %s, difference %s, bound %s" % (kind, r, delta, diff - delta, bound))
                assert (np.abs(diff - delta) <= bound).all(), (kind, r, diff, delta, bound)
                # not vacuous: every column's bound is below 1e-5 of the norm of this read's Delta_r; column by column it is
                # below 1e-5 of |Delta_r[k]| for the coverage and the error rate, which every read moves, and of the
                # column's root mean square over all reads for the repeat parameters, where a single read's component
                # can cancel to nothing (a read of unique sequence barely moves q1)
                assert (bound < 1e-5 * np.linalg.norm(delta)).all(), (kind, r, delta, bound)
                assert (bound[:2] < 1e-5 * np.abs(delta[:2])).all() and (bound < 1e-5 * scale).all(), (kind, r, delta, bound)
        finally:
            one.close()
    finally:
        twin.close()


@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_sum_of_rows_and_summary(hip_lib, kind):
    """sum_r Delta_r from the moments kernel against numpy's column sums (the bound of test_moments); summary()
    recomputed from the rows in numpy to 1e-10 relative; fix= honoured; the same bytes from the same inputs."""
    from scipy.stats import norm
    from covest_amd import print_output
    reads, _, counts, hist_orig, model, estimate, _ = fitted(kind)
    got = influence_of(kind)
    rows, n, P = got.rows, got.n_reads, len(model.params)
    total, cross = got.moments()
    bound = n * 2.0 ** -52 * np.abs(rows).sum(axis=0)
    assert (np.abs(total - rows.sum(axis=0)) <= bound).all()
    assert (np.abs(total - np.array([math.fsum(rows[:, j].tolist()) for j in range(P + 1)])) <= bound).all()
    summary = got.summary()
    again = infl.read_influence(model, estimate, counts, reads)
    same_bits(again.rows, rows, "rows twice")
    assert again.summary() == summary and repr(again.summary()) == repr(summary)
    assert summary['reads'] == n and summary['reason'] == got.info['reason']
    # both fitted cases have a positive definite information (all P parameters free): the recomputation below runs for both
    assert got.info['covariance'] is not None and summary['reason'] is None and got.info['free'] == list(range(P))

    free = got.info['free']
    inverse = np.zeros((P, P))
    inverse[np.ix_(free, free)] = np.asarray(got.info['covariance'])
    N, c = float(got.occurrences_full), estimate[0]
    S = N / model.correct_c(c)
    shifts = np.zeros((n, P + 1))
    shifts[:, :P] = rows[:, :P] @ inverse.T
    shifts[:, 0] += c * rows[:, P] / N
    shifts[:, P] = -S * shifts[:, 0] / c
    mean = shifts.mean(axis=0)
    V = (n - 1) / n * (shifts - mean).T @ (shifts - mean)
    z = norm.ppf(0.975)
    centres = list(estimate) + [S]
    for d, name in enumerate(list(model.params) + ['genome_size']):
        if (0 if d == P else d) not in free:
            assert summary['standard_errors'][name] is None
            continue
        se = math.sqrt(V[d, d])
        assert summary['standard_errors'][name] == pytest.approx(se, rel=1e-10), name
        assert summary['intervals'][name] == pytest.approx([centres[d] - z * se, centres[d] + z * se], rel=1e-10), name
    assert np.allclose(got.shifts(), shifts, rtol=1e-10, atol=1e-10 * np.abs(shifts).max())
    print("influence %s: standard errors %s" % (kind, summary['standard_errors']))

    fix = [None] * P
    fix[1] = estimate[1]
    fixed = infl.read_influence(model, estimate, counts, reads, fix=fix, level=0.9).summary()
    assert fixed['standard_errors'][model.params[1]] is None and fixed['standard_errors'][model.params[0]] is not None
    assert 1 not in fixed['free'] and fixed['level'] == 0.9
    plain = print_output(hist_orig, model, True, 1, estimate, silent=True)
    record = print_output(hist_orig, model, True, 1, estimate, silent=True, read_influence=got)
    assert {key: record[key] for key in plain} == plain
    assert record['read_influence_reads'] == n and record['read_influence_se_genome_size'] == summary['standard_errors']['genome_size']


# ---- device forms -------------------------------------------------------------------------------------------------------
_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import random
import numpy as np
import kmer_reference as kr
import influence_reference as ir
import stream_order as so
from covest_amd import _capi, influence as infl, kmer_hist as kh
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
k = 21
rng = np.random.default_rng(8)
TABLE = rng.normal(size=(5, 3)) * np.array([1.0, 1e4, 1e-5])
counted = [kr.genome(), kr.genome()[:700], "A" * (k + 2)]
table_counts = kr.count(counted, k, True)
counts = kh.KmerCounts(k, canonical=True, min_slots=1 << 14)
counts.add_reads(counted)
d_table = torch.from_numpy(TABLE).to(dev)
PATF, PAD = -1.2345e300, 16


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run(reads, fixed_len, shift, n_cols=3, on=None):
    # the device form on `reads` whose bases start `shift` bytes into an aligned buffer; guard doubles either side of rows
    blob = np.frombuffer(("N" * shift + "".join(reads)).encode(), dtype=np.uint8).copy()
    d_bases = torch.from_numpy(blob).to(dev)
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    d_offsets = torch.from_numpy(offsets).to(dev)
    n, width = len(reads), n_cols + 1
    out = torch.full((PAD + n * width + PAD,), PATF, dtype=torch.float64, device=dev)
    tab = d_table if n_cols == 3 else torch.from_numpy(np.ascontiguousarray(TABLE[:, :n_cols])).to(dev)
    counts.read_influence_device(d_bases.data_ptr() + shift, n, fixed_len if fixed_len is not None else 0, tab.data_ptr(),
                                 TABLE.shape[0], n_cols, out.data_ptr() + 8 * PAD,
                                 d_offsets_ptr=None if fixed_len is not None else d_offsets.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:PAD] == PATF).all() and (out[PAD + n * width:] == PATF).all(), ("stray rows", len(reads), fixed_len, shift)
    return out[PAD:PAD + n * width].reshape(n, width)


def want_rows(reads, n_cols=3):
    return ir.influence_rows(reads, table_counts, k, True, TABLE[:, :n_cols])


pyrng = random.Random(99)
ragged = (kr.genome_reads(pyrng, 2, k + 70) + ["", kr.genome()[:k - 1], "ACGT" * 30, "A" * (k + 70)] +
          kr.genome_reads(pyrng, 3, 2 * k + 200))
want = want_rows(ragged)
for shift in (0, 1, 2, 3):
    got = run(ragged, None, shift)
    assert np.array_equal(bits(got), bits(want)), ("ragged", shift, got, want)
print("device form ok")

for length in (k, k + 63, k + 64, k + 65, k + 128, k - 1):
    for n in (1, 3, 4, 5):
        reads = kr.genome_reads(pyrng, n, length)
        want = want_rows(reads, 2)
        for fixed_len in (length, None):
            got = run(reads, fixed_len, 3, n_cols=2)
            assert np.array_equal(bits(got), bits(want)), ("one length", length, n, fixed_len)
print("fixed length ok")

# more than 4096 windows: with offsets NaN in the value columns and W written, the neighbours untouched by it; reads of
# one length are refused on the host
long_read = (kr.genome() * 2)[:4097 + k - 1]
mixed = [kr.genome()[:100], long_read, kr.genome()[50:150]]
got, want = run(mixed, None, 1), want_rows(mixed)
assert np.isnan(got[1, :3]).all() and got[1, 3] == 4097.0 and np.isnan(want[1, :3]).all()
assert np.array_equal(bits(got[[0, 2]]), bits(want[[0, 2]]))
L = _capi.lib()
d_long = torch.from_numpy(np.frombuffer(long_read.encode(), dtype=np.uint8).copy()).to(dev)
d_rows = torch.full((4,), PATF, dtype=torch.float64, device=dev)
rc = L.covest_kmer_read_influence_device(counts._handle, d_long.data_ptr(), None, 1, len(long_read), d_table.data_ptr(), 5, 3,
                                         d_rows.data_ptr(), stream)
assert rc == _capi.COVEST_E_UNSUPPORTED and "4097 windows" in _capi.last_error(), (rc, _capi.last_error())
rc = L.covest_kmer_read_influence_device(counts._handle, d_long.data_ptr(), None, 1, len(long_read) - 1, d_table.data_ptr(), 5, 3,
                                         d_rows.data_ptr(), stream)
torch.cuda.synchronize()
assert rc == 0 and d_rows.cpu().numpy()[3] == 4096.0
print("long reads ok")

# statuses that need device buffers
d_reads = torch.from_numpy(np.frombuffer("".join(kr.genome_reads(pyrng, 300, 100)).encode(), dtype=np.uint8).copy()).to(dev)
d_out = torch.full((300 * 4,), PATF, dtype=torch.float64, device=dev)


def device_call(handle, bases=d_reads.data_ptr(), n=300, read_len=100, table=d_table.data_ptr(), n_rows=5, n_cols=3,
                rows=d_out.data_ptr()):
    return L.covest_kmer_read_influence_device(handle, bases, None, n, read_len, table, n_rows, n_cols, rows, stream)


assert device_call(None) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, n=-1) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, read_len=-1) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, n_rows=0) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, n_cols=0) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, n_cols=9) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, table=None) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, rows=None) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, rows=d_out.data_ptr() + 4) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, bases=None) == _capi.COVEST_E_INVALID
assert device_call(counts._handle, bases=None, n=0) == 0
torch.cuda.synchronize()
assert (d_out.cpu().numpy() == PATF).all(), "a refused or empty call wrote rows"
wide = kh.KmerCounts(32)
assert device_call(wide._handle) == _capi.COVEST_E_UNSUPPORTED
wide.close()
bulk = kh.KmerCounts(k, canonical=True)
path = bulk.count_reads_device(d_reads.data_ptr(), 300, 100, stream=stream)
assert path == "partitioned", (path, getattr(bulk, "why_not_partitioned", None))
assert device_call(bulk._handle) == _capi.COVEST_E_INVALID and "covest_kmer_count_reads_device result" in _capi.last_error()
bulk.close()
print("statuses ok")

# the moments on device arrays: the host form's bits, twice
rows = np.ascontiguousarray(rng.normal(size=(1500, 4)) * np.array([1.0, 1e3, 1e-3, 50.0]) + 7.0)
centre = np.array([7.0, 6.5, 7.25, 0.0])
d_in, d_centre = torch.from_numpy(rows).to(dev), torch.from_numpy(centre).to(dev)
d_sum = torch.full((PAD + 4 + PAD,), PATF, dtype=torch.float64, device=dev)
d_cross = torch.full((PAD + 10 + PAD,), PATF, dtype=torch.float64, device=dev)
host_sum, host_cross = infl.rows_moments(rows, centre)
for _ in range(2):
    infl.rows_moments_device(d_in.data_ptr(), 1500, 4, d_centre.data_ptr(), d_sum.data_ptr() + 8 * PAD, d_cross.data_ptr() + 8 * PAD,
                             stream=stream)
    torch.cuda.synchronize()
    s, c = d_sum.cpu().numpy(), d_cross.cpu().numpy()
    assert (s[:PAD] == PATF).all() and (s[PAD + 4:] == PATF).all() and (c[:PAD] == PATF).all() and (c[PAD + 10:] == PATF).all()
    assert np.array_equal(bits(s[PAD:PAD + 4]), bits(host_sum)) and np.array_equal(bits(c[PAD:PAD + 10]), bits(host_cross))
print("moments device ok")

# ---- a non-default stream, scheme A of stream_order.py: late inputs, poison bases, guard pattern under the outputs -----
reads = np.frombuffer("".join(kr.genome_reads(pyrng, 64, 100)).encode(), dtype=np.uint8).reshape(64, 100).copy()
strings = [row.tobytes().decode() for row in reads]
want = want_rows(strings)
poison = so.other_bases(reads)
assert not np.array_equal(bits(want), bits(want_rows([row.tobytes().decode() for row in poison])))
true_bases, true_table = so.to_device(reads), so.to_device(TABLE)
d_bases, d_tab = so.to_device(poison), so.to_device(TABLE[::-1].copy())
guard = torch.full((64 * 4,), PATF, dtype=torch.float64, device=dev)
d_rows = torch.zeros(64 * 4, dtype=torch.float64, device=dev)
m_guard = torch.full((3 + 6,), PATF, dtype=torch.float64, device=dev)
d_moments = torch.zeros(3 + 6, dtype=torch.float64, device=dev)
d_zero = torch.zeros(4, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
side = so.side_stream()
late = so.late(side, [(d_bases, true_bases), (d_tab, true_table), (d_rows, guard), (d_moments, m_guard)])
counts.read_influence_device(d_bases.data_ptr(), 64, 100, d_tab.data_ptr(), 5, 3, d_rows.data_ptr(), stream=side.cuda_stream)
infl.rows_moments_device(d_rows.data_ptr(), 64, 3, d_zero.data_ptr(), d_moments.data_ptr(), d_moments.data_ptr() + 8 * 3,
                         stream=side.cuda_stream)
issued = late.host_ms()
side.synchronize()
late.check_blind(issued, "read_influence_device + rows_moments_device")
got = d_rows.cpu().numpy().reshape(64, 4)
assert np.array_equal(bits(got), bits(want)), "the influence rows did not follow the stream"
# (the moments read d_rows as rows of 3 doubles: 64 rows of the first 192 doubles)
as_three = got.reshape(-1)[:192].reshape(64, 3)
host_sum, host_cross = infl.rows_moments(as_three)
got_m = d_moments.cpu().numpy()
assert np.array_equal(bits(got_m[:3]), bits(host_sum)) and np.array_equal(bits(got_m[3:]), bits(host_cross)), "moments off the stream"
torch.cuda.synchronize()
counts.close()
print("stream ok")
print("influence device forms ok")
"""


@functools.lru_cache(maxsize=None)
def device_child():
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): d_bases at byte offsets 0 .. 3, guard doubles either side of the rows, reads
    of one length against the same reads with offsets, a read of 4 097 windows (NaN with offsets, refused at one
    length), the statuses that need device buffers, the moments on device arrays."""
    proc = device_child()
    for marker in ("device form ok", "fixed length ok", "long reads ok", "statuses ok", "moments device ok"):
        assert marker in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


def test_device_entry_points_on_a_side_stream(hip_lib):
    """Scheme A of tests/stream_order.py on both device entry points: the true reads, the true table and the guard
    pattern arrive late on a side stream; only that stream is waited for; Delay.check_blind holds."""
    proc = device_child()
    assert proc.returncode == 0 and "stream ok" in proc.stdout and "influence device forms ok" in proc.stdout, (
        proc.stdout[-2000:] + proc.stderr[-4000:])
    print("\n".join(line for line in proc.stdout.splitlines() if line.startswith("stream-order:")))
