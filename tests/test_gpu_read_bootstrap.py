"""The bootstrap over reads on the device: the multiplicities of covest_bootstrap_weights* bit for
bit against their numpy restatement (tests/bootstrap_weights_reference.py); the weighted adds of every key width exactly
against the unweighted host counter (tests/kmer_reference.py) on the reads written out weight times
(bootstrap_weights_reference.expand); the identities that tie the weighted add to add_device and to the jackknife's
leave-out histograms; and bootstrap_histograms / read_bootstrap / print_output end to end.  No statistical assertion on
the size of a standard error: how the bootstrap's error compares with the jackknife's and with the empirical spread is a
measurement (tools/read_bootstrap_recovery.py, profiles/read_bootstrap_recovery.txt)."""
import ctypes
import functools
import math
import random

import numpy as np
import pytest

import bootstrap_weights_reference as bw
import kmer_reference as kr

pytestmark = pytest.mark.gpu

E_INVALID = -1
PATTERN = 0xA5A5A5A5
K_ALL = (5, 13, 21, 31, 32, 63, 64, 127, 128, 255)  # no first slot, the smallest with one, the widest word, both sides of
#                                                     every change of width
BIG = 70_000                                        # past the 4 096 LDS bins of the histogram kernel


def as_dict(hist_list):
    return {i: v for i, v in enumerate(hist_list) if i > 0 and v > 0}


def texts(bases):
    return [row.tobytes().decode() for row in bases]


def packed(reads):
    """(bases uint8, offsets int64) of a list of strings."""
    lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8), offsets


class Device:
    """Host arrays as device buffers for the life of a test (covest_amd.sample._DeviceArena: the runtime the library is
    bound to)."""

    def __init__(self):
        from covest_amd.sample import _DeviceArena
        self.arena = _DeviceArena("test_gpu_read_bootstrap")
        self.n = 0

    def up(self, array):
        a = np.ascontiguousarray(array)
        self.n += 1
        return self.arena.upload("b%d" % self.n, a.ctypes.data, a.nbytes)

    def down(self, ptr_name, array):
        self.arena.download(ptr_name, array)

    def close(self):
        self.arena.close()


@pytest.fixture
def dev(hip_lib):
    d = Device()
    yield d
    d.close()


# ---- the draw ------------------------------------------------------------------------------------------------------------
SEEDS = (12345, (7 << 32) | 99)                      # one of them above 2^32: both key words in use


@pytest.mark.parametrize("first_read", [0, (1 << 32) - 3])       # (the index crosses a word)
@pytest.mark.parametrize("replicate", [0, 1, (1 << 32) - 1])
def test_draw_is_the_restatement_bit_for_bit(hip_lib, first_read, replicate):
    from covest_amd.read_bootstrap import bootstrap_weights
    for seed in SEEDS:
        got = bootstrap_weights(1000, replicate, seed=seed, first_read=first_read)
        want = bw.weights(1000, replicate, seed=seed, first_read=first_read)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (seed, int((got != want).sum()))
        # rows 300 .. 700 drawn alone are rows 300 .. 700 of the whole
        part = bootstrap_weights(401, replicate, seed=seed, first_read=first_read + 300)
        assert np.array_equal(part, want[300:701]), seed
    assert not np.array_equal(bw.weights(1000, replicate, SEEDS[0], first_read), bw.weights(1000, replicate, SEEDS[1], first_read))
    assert bootstrap_weights(0, replicate).size == 0


def test_draw_on_the_device_writes_nothing_outside_its_output(dev):
    from covest_amd.read_bootstrap import bootstrap_weights_device
    for n in (1000, 257, 1):
        buf = np.full(n + 16, PATTERN, dtype=np.uint32)
        ptr = dev.up(buf)
        bootstrap_weights_device(ptr + 8 * 4, n, 3, seed=SEEDS[1], first_read=(1 << 32) - 3)
        dev.down("b%d" % dev.n, buf)  # (the null stream: waits for the kernel)
        assert (buf[:8] == PATTERN).all() and (buf[8 + n:] == PATTERN).all(), n
        assert np.array_equal(buf[8:8 + n], bw.weights(n, 3, seed=SEEDS[1], first_read=(1 << 32) - 3)), n


# ---- the weighted count, exact ---------------------------------------------------------------------------------------------
def unique_reads(rng, n, length):
    """Random reads that are not slices of the genome: at k >= 13 their keys are nobody else's."""
    return ["".join(rng.choice("ACGT") for _ in range(length)) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def ragged_set(k):
    """(a): a few dozen reads with offsets and a weight each.  An empty read, reads shorter than k, of length k, of k +
    63, k + 64, k + 65 (the 64-window round), four of each; a zero-weight read first, last and in the middle, all three
    with keys of their own; BIG on a read shorter than k and on one of k bases (one key each: the truth stays small)."""
    rng = random.Random(31000 + k)
    lengths = [0, max(k - 2, 1), k - 1, k, k + 1, k + 63, k + 64, k + 65]
    reads = [r for length in lengths for r in kr.genome_reads(rng, 4, length)]
    rng.shuffle(reads)
    weights = [(1, 2, 13, 1, 0, 2)[i % 6] for i in range(len(reads))]
    reads += [kr.genome_reads(rng, 1, k - 1)[0], kr.genome_reads(rng, 1, k)[0]]
    weights += [BIG, BIG]
    zero = unique_reads(rng, 3, k + 70)
    mid = len(reads) // 2
    reads = [zero[0]] + reads[:mid] + [zero[1]] + reads[mid:] + [zero[2]]
    weights = [0] + weights[:mid] + [0] + weights[mid:] + [0]
    return tuple(reads), tuple(weights)


def with_the_three(weights):
    """ragged_set's weights with its three zero-weight reads of keys of their own counted once."""
    mid = (len(weights) - 3) // 2
    return [1 if i in (0, mid + 1, len(weights) - 1) else w for i, w in enumerate(weights)]


@functools.lru_cache(maxsize=None)
def fixed_set(k, length):
    """(b), (c): reads of one length and a weight each, zero-weight reads first and last.  300 reads where a read has one
    window or two (more than one workgroup of the kernel that numbers the windows through) or is shorter than k, 40
    otherwise; BIG only where a read has at most two windows."""
    rng = random.Random(33000 + 1000 * k + length)
    n = 300 if length <= k + 1 else 40
    reads = kr.genome_reads(rng, n, length)
    weights = [rng.choice((0, 1, 2, 13)) for _ in range(n)]
    weights[0] = weights[-1] = 0
    if length <= k + 1:
        weights[n // 3] = BIG
    return tuple(reads), tuple(weights)


def truth(reads, weights, k, canonical, before=()):
    hist, distinct = kr.histogram(list(before) + bw.expand(reads, weights), k, canonical)
    return hist, distinct


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", K_ALL)
def test_weighted_count_is_the_expanded_truth(dev, k, canonical):
    from covest_amd.kmer_hist import KmerCounts
    # (a) ragged reads, on a counter that already holds counts
    reads, weights = ragged_set(k)
    before = kr.genome_reads(random.Random(35000 + k), 10, k + 40)
    want_hist, want_distinct = truth(reads, weights, k, canonical, before)
    bases, offsets = packed(reads)
    d_bases, d_off, d_w = dev.up(bases), dev.up(offsets), dev.up(np.array(weights, dtype=np.uint32))
    counts = KmerCounts(k, canonical=canonical)
    counts.add_reads(before)
    counts._reserve_for(bases.size + len(reads))
    counts.add_weighted_device(d_bases, len(reads), 0, d_w, d_offsets_ptr=d_off, reserve=False)
    assert counts.histogram() == want_hist, "ragged"
    assert len(counts) == want_distinct, "ragged: distinct"
    assert want_hist[BIG:] and len(want_hist) > 4096
    if k >= 13:  # the zero-weight reads hold keys nobody else has, 71 windows each: none of them was created
        with_zero = kr.histogram(list(before) + bw.expand(reads, with_the_three(weights)), k, canonical)[1]
        assert with_zero == want_distinct + 3 * 71, (with_zero, want_distinct)
    # ... and the host form, on an empty counter, against the device form on the same
    host, device = KmerCounts(k, canonical=canonical), KmerCounts(k, canonical=canonical)
    host.add_weighted(list(reads), weights)
    device._reserve_for(bases.size + len(reads))
    device.add_weighted_device(d_bases, len(reads), 0, d_w, d_offsets_ptr=d_off, reserve=False)
    want_alone = truth(reads, weights, k, canonical)
    assert host.histogram() == device.histogram() == want_alone[0], "host form"
    assert len(host) == len(device) == want_alone[1]
    for c in (counts, host, device):
        c.close()
    # (b) one length, no offsets: k and k + 1 (one window and two a read), k + 80; (c) shorter than k: the wave kernel
    for length in (k, k + 1, k + 80, k - 1):
        reads, weights = fixed_set(k, length)
        want_hist, want_distinct = truth(reads, weights, k, canonical)
        blob = np.frombuffer("".join(reads).encode("ascii"), dtype=np.uint8)
        counts = KmerCounts(k, canonical=canonical)
        counts.add_weighted_device(dev.up(blob), len(reads), length, dev.up(np.array(weights, dtype=np.uint32)))
        assert counts.histogram() == want_hist, ("one length", length)
        assert len(counts) == want_distinct, ("one length: distinct", length)
        counts.close()


# ---- identities ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_reads():
    """400 simulated reads of 50 bases from a 2 000-base genome (tests/test_gpu_jackknife.py's)."""
    from covest_amd import simulate as sim
    g = sim.random_genome(2000, 5)
    return sim.simulate_reads(g, 50, n_reads=400, error_rate=0.02, seed=5, first_read=0)


@pytest.mark.parametrize("k", [21, 40])
def test_all_weights_one_is_the_unweighted_add(dev, k):
    from covest_amd.kmer_hist import KmerCounts
    reads = small_reads()
    n, L = reads.bases.shape
    ones = dev.up(np.ones(n, dtype=np.uint32))
    d_bases = dev.up(reads.bases.reshape(-1))
    d_off = dev.up(np.arange(n + 1, dtype=np.int64) * L)
    for offs, read_len in ((None, L), (d_off, 0)):
        plain, weighted = KmerCounts(k), KmerCounts(k)
        plain._reserve_for(n * L)
        weighted._reserve_for(n * L)
        plain.add_device(d_bases, n, read_len, d_offsets_ptr=offs, reserve=False)
        weighted.add_weighted_device(d_bases, n, read_len, ones, d_offsets_ptr=offs, reserve=False)
        assert weighted.histogram() == plain.histogram() and len(weighted) == len(plain) > 0
        plain.close()
        weighted.close()


def test_group_indicator_weights_give_the_leave_out_histograms(dev):
    from covest_amd import jackknife, sample
    from covest_amd.kmer_hist import KmerCounts
    reads = small_reads()
    n, L = reads.bases.shape
    G, k, seed = 4, 9, 11
    _, hists, _ = jackknife.leave_group_out_histograms(reads, k, G, seed=seed)
    group = sample.read_groups(n, G, seed=seed)
    d_bases = dev.up(reads.bases.reshape(-1))
    for g in range(G):
        counts = KmerCounts(k)
        counts.add_weighted_device(d_bases, n, L, dev.up((group != g).astype(np.uint32)))
        assert as_dict(counts.histogram()) == hists[g], g
        counts.close()


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_their_status(dev):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    lib = _capi.lib()
    vp = ctypes.c_void_p
    bases, offsets = packed(["ACGTACGTAC", "ACGTA"])
    weights = np.array([1, 2, 0], dtype=np.uint32)
    d_bases, d_off, d_w = dev.up(bases), dev.up(offsets), dev.up(weights)
    counts = KmerCounts(5)

    def host(n=2, w=weights.ctypes.data):
        return lib.covest_kmer_add_weighted(counts._handle, vp(bases.ctypes.data), vp(offsets.ctypes.data), n, vp(w))

    def device(n=2, w=d_w):
        return lib.covest_kmer_add_weighted_device(counts._handle, vp(d_bases), vp(d_off), n, 0, vp(w), vp(0))

    for form in (host, device):
        assert form(w=0) == E_INVALID and "null weights" in _capi.last_error()
        assert form(w=(weights.ctypes.data if form is host else d_w) + 1) == E_INVALID and "aligned" in _capi.last_error()
        assert form(n=-1) == E_INVALID
        assert form(n=0, w=0) == 0                      # no reads: no weights needed
    assert counts.histogram() == [0] and len(counts) == 0   # nothing was counted by a refused call
    assert host() == 0 and device() == 0
    assert as_dict(counts.histogram()) == as_dict(kr.histogram(["ACGTACGTAC"] * 2 + ["ACGTA"] * 4, 5)[0])
    assert lib.covest_bootstrap_weights(-1, -1, 0, 0, 0, vp(weights.ctypes.data)) == E_INVALID
    assert lib.covest_bootstrap_weights(-1, 2, -1, 0, 0, vp(weights.ctypes.data)) == E_INVALID
    assert lib.covest_bootstrap_weights(-1, 2, 0, 0, 0, vp(0)) == E_INVALID
    assert lib.covest_bootstrap_weights(-1, 2, 0, 0, 0, vp(weights.ctypes.data + 2)) == E_INVALID
    assert lib.covest_bootstrap_weights_device(-1, 2, 0, 0, 0, vp(d_w + 2), vp(0)) == E_INVALID
    # a counter that holds a partitioned result refuses the weighted add as it refuses the unweighted one
    reads = small_reads()
    n, L = reads.bases.shape
    part = KmerCounts(21)
    d_reads = dev.up(reads.bases.reshape(-1))
    if part.count_reads_device(d_reads, n, L) == "partitioned":
        ones = dev.up(np.ones(n, dtype=np.uint32))
        rc = lib.covest_kmer_add_weighted_device(part._handle, vp(d_reads), vp(0), n, L, vp(ones), vp(0))
        assert rc == lib.covest_kmer_add_device(part._handle, vp(d_reads), vp(0), n, L, vp(0)) == E_INVALID
    part.close()
    counts.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
E2E_SEED = 17


@functools.lru_cache(maxsize=None)
def fitted():
    """(reads, model, estimate, histogram) of the basic model at k = 21 on 20 000 simulated 100-base reads of a 50 kbp
    random genome, e = 0.01."""
    from covest_amd import constants, simulate as sim
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import compute_coverage_apx
    from covest_amd.kmer_hist import KmerCounts
    from covest_amd.models import BasicModel
    g = sim.random_genome(50_000, 23)
    reads = sim.simulate_reads(g, 100, n_reads=20_000, error_rate=0.01, seed=23, both_strands=False)
    counts = reads.add_to(KmerCounts(21))
    hist = as_dict(counts.histogram())
    counts.close()
    model = BasicModel(21, 100, hist, 0, max_error=constants.MAX_ERRORS)
    est, ok = CoverageEstimator(model).compute_coverage(list(compute_coverage_apx(hist, 21, 100)))
    assert ok
    return reads, model, [float(v) for v in est], hist


def test_bootstrap_histograms_are_the_weighted_truths(hip_lib):
    from covest_amd.read_bootstrap import bootstrap_histograms
    reads, _, _, hist = fitted()
    strings = texts(reads.bases)
    full, hists, occ, drawn = bootstrap_histograms(reads, 21, 4, seed=E2E_SEED)
    assert full == hist == as_dict(kr.histogram(strings, 21)[0])
    assert len(hists) == len(occ) == len(drawn) == 4
    for b in range(4):
        w = bw.weights(reads.n_reads, b, seed=E2E_SEED, first_read=reads.first_read)
        assert hists[b] == as_dict(kr.histogram(bw.expand(strings, w), 21)[0]), b
        assert drawn[b] == int(w.sum()) and occ[b] == drawn[b] * (100 - 21 + 1), b
    assert len(set(drawn)) > 1


def test_bootstrap_histograms_of_ragged_reads(hip_lib):
    """Reads of their own lengths (the offsets go up beside the bases), cut as tests/test_gpu_jackknife.py cuts them."""
    from covest_amd.read_bootstrap import bootstrap_histograms
    reads = small_reads()
    lens = np.random.default_rng(8).choice((0, 5, 8, 9, 10, 30, 50), size=400)  # empty reads and reads shorter than k
    offsets = np.zeros(401, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.concatenate([reads.bases[i, :lens[i]] for i in range(400)])
    blob = bases.tobytes().decode()
    strings = [blob[offsets[i]:offsets[i + 1]] for i in range(400)]
    full, hists, occ, drawn = bootstrap_histograms((bases, offsets), 9, 3, seed=E2E_SEED)
    assert full == as_dict(kr.histogram(strings, 9)[0])
    assert len(hists) == len(occ) == len(drawn) == 3
    for b in range(3):
        w = bw.weights(400, b, E2E_SEED)
        assert hists[b] == as_dict(kr.histogram(bw.expand(strings, w), 9)[0]), b
        assert drawn[b] == int(w.sum()) and occ[b] == sum(i * n for i, n in hists[b].items()), b


def test_read_bootstrap_end_to_end(hip_lib):
    from covest_amd import print_output
    from covest_amd.read_bootstrap import read_bootstrap
    reads, model, est, hist = fitted()
    B = 8
    out = read_bootstrap(model, est, reads, replicates=B, seed=E2E_SEED)
    assert out["replicates"] == B and out["seed"] == E2E_SEED and out["refit"] == "lockstep-gradient"
    assert out["estimates"].shape == (B, 2) and out["success"].shape == (B,) and out["at_bound"].shape == (B, 2)
    assert out["used"] + out["failed"] == B and out["used"] == int(out["success"].sum())
    assert len(out["occurrences"]) == len(out["reads_drawn"]) == B and len(out["full_estimate"]) == 2
    assert out["occurrences"] == [d * 80 for d in out["reads_drawn"]]
    assert out["reads_drawn"] == [int(bw.weights(reads.n_reads, b, seed=E2E_SEED).sum()) for b in range(B)]
    assert out["occurrences_full"] == sum(i * n for i, n in hist.items()) and out["keys_added"] >= 0
    for name in ("coverage", "error_rate", "genome_size"):
        se, (lo, hi) = out["standard_errors"][name], out["intervals"][name]
        assert se is not None and math.isfinite(se) and se > 0.0, name
        assert math.isfinite(out["mean"][name]) and math.isfinite(out["bias"][name]) and -math.inf < lo <= hi < math.inf, name
        assert 0.0 <= out["bound_share"][name] <= 1.0
        print("%-12s mean %.6g se %.4g bias %.3g interval [%.6g, %.6g]" % (name, out["mean"][name], se, out["bias"][name], lo, hi))
    # the same seed: the same bits; another seed: other replicates
    again = read_bootstrap(model, est, reads, replicates=B, seed=E2E_SEED)
    assert again["estimates"].tobytes() == out["estimates"].tobytes() and again["reads_drawn"] == out["reads_drawn"]
    assert again["standard_errors"] == out["standard_errors"] and again["intervals"] == out["intervals"]
    other = read_bootstrap(model, est, reads, replicates=B, seed=E2E_SEED + 1)
    assert other["reads_drawn"] != out["reads_drawn"] and other["estimates"].tobytes() != out["estimates"].tobytes()
    # the record: the new fields with the keyword, and without it what it was
    plain = print_output(hist, model, True, 1, estimated=est, silent=True)
    record = print_output(hist, model, True, 1, estimated=est, silent=True, read_bootstrap=out)
    new = {key for key in record if key.startswith("read_bootstrap_")}
    assert not any(key.startswith("read_bootstrap") for key in plain)
    assert {key: value for key, value in record.items() if key not in new} == plain
    want = {"read_bootstrap_replicates", "read_bootstrap_used", "read_bootstrap_failed", "read_bootstrap_level"}
    want |= {"read_bootstrap_%s_%s" % (kind, name) for kind in ("se", "bias", "interval")
             for name in ("coverage", "error_rate", "genome_size")}
    assert new == want
    assert record["read_bootstrap_replicates"] == B and record["read_bootstrap_used"] == out["used"]
    assert record["read_bootstrap_failed"] == out["failed"] and record["read_bootstrap_level"] == 0.95
    assert record["read_bootstrap_se_genome_size"] == out["standard_errors"]["genome_size"]
    assert record["read_bootstrap_interval_coverage"] == out["intervals"]["coverage"]
    # fix= is honoured: the error rate stays, and has no summary nor a field in the record
    fixed = read_bootstrap(model, est, reads, replicates=4, seed=E2E_SEED, fix=[None, est[1]])
    assert fixed["standard_errors"]["error_rate"] is None and fixed["standard_errors"]["coverage"] is not None
    assert "read_bootstrap_se_error_rate" not in print_output(hist, model, True, 1, estimated=est, silent=True, read_bootstrap=fixed)
