"""The read split and the jackknife over reads without a GPU: the group rule's fixed points on its numpy restatement
(tests/split_reference.py), covest_amd.jackknife.summarize_jackknife on hand-made arrays, the record of
report.print_output with and without a jackknife on a stand-in model, and the argument errors of split_reads,
leave_group_out_histograms and read_jackknife, which are raised before the library is asked."""
import math

import numpy as np
import pytest

import sim_reference as sr
import split_reference as ref

SEED = (0x5a3d << 32) | 0x0badcafe   # both key words in use
NAMES = ("coverage", "error_rate")


# ---- the rule
def test_one_group_is_group_zero_and_groups_stay_in_range():
    assert not ref.groups_of(0, 1000, 1, SEED).any()
    for G in (2, 3, 64, 65, 255, 256):
        g = ref.groups_of(7, 5000, G, SEED)
        assert g.min() >= 0 and g.max() <= G - 1, G
        assert np.unique(g).size == min(G, np.unique(g).size) and np.unique(g).size > G // 2, G


def test_the_group_is_the_words_top_share():
    """group = (w * G) >> 32 of word 0 of block (lo32(r), hi32(r), 0, 8): one read by the scalar restatement."""
    r = 123456789
    w = sr.philox_scalar((r & sr.MASK, r >> 32, 0, 8), (SEED & sr.MASK, SEED >> 32))[0]
    for G in (1, 2, 7, 256):
        assert ref.groups_of(r, 1, G, SEED).tolist() == [(w * G) >> 32], G
    # the sampler's stream (.., 0, 2) is another one: the same read, the same seed, another word
    assert w != sr.philox_scalar((r & sr.MASK, r >> 32, 0, 2), (SEED & sr.MASK, SEED >> 32))[0]


def test_a_chunk_equals_the_same_rows_of_the_whole_run():
    whole = ref.groups_of(1000, 4000, 32, SEED)
    for a, m in ((0, 1), (17, 1024), (3999, 1), (1025, 2000)):
        assert np.array_equal(ref.groups_of(1000 + a, m, 32, SEED), whole[a:a + m]), (a, m)


def test_a_read_index_above_32_bits_uses_the_high_word():
    base = (1 << 32) - 3
    g = ref.groups_of(base, 2000, 256, SEED)
    low = ref.groups_of(0, 2000 - 3, 256, SEED)         # the same low words with the high word 0
    assert not np.array_equal(g[3:], low)
    r = (1 << 32) + 5
    w = sr.philox_scalar((5, 1, 0, 8), (SEED & sr.MASK, SEED >> 32))[0]
    assert ref.groups_of(r, 1, 256, SEED).tolist() == [(w * 256) >> 32]


def test_the_restated_partition_is_stable():
    rng = np.random.default_rng(3)
    lens = rng.choice((0, 1, 5, 40), size=500)
    offsets = np.zeros(501, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(offsets[-1]))
    out, out_offsets, index, first = ref.split(bases, offsets, 9, 5, SEED)
    group = ref.groups_of(9, 500, 5, SEED)
    assert first[0] == 0 and first[-1] == 500 and out.size == bases.size
    for g in range(5):
        rows = index[first[g]:first[g + 1]] - 9
        assert (group[rows] == g).all() and (np.diff(rows) > 0).all(), g
    for rank in (0, 1, 250, 499):
        i = index[rank] - 9
        assert np.array_equal(out[out_offsets[rank]:out_offsets[rank + 1]], bases[offsets[i]:offsets[i + 1]])


# ---- summarize_jackknife
def _correct_c(c):
    return c * 0.8


def test_the_jackknife_of_a_mean_is_its_standard_error():
    """A statistic that is the mean of the groups' values: the leave-one-out means give sd / sqrt(G), and a linear
    statistic has no bias.  The same float64 formula over at most 64 terms, in another order: 1e-12 relative."""
    from covest_amd.jackknife import summarize_jackknife
    rng = np.random.default_rng(5)
    for G in (2, 8, 64):
        x = rng.normal(0.05, 0.01, size=G)
        leave_out = (x.sum() - x) / (G - 1)
        est = np.column_stack([np.full(G, 10.0), leave_out])
        out = summarize_jackknife(est, np.ones(G, bool), [10.0, x.mean()], np.full(G, 1000.0), 1000.0, NAMES, None, 0.95,
                                  _correct_c)
        assert out["standard_errors"]["error_rate"] == pytest.approx(x.std(ddof=1) / math.sqrt(G), rel=1e-12), G
        assert abs(out["bias"]["error_rate"]) <= 1e-12 * abs(x.mean()), G
        assert out["bias_corrected"]["error_rate"] == pytest.approx(x.mean(), rel=1e-12)
        assert out["mean"]["error_rate"] == pytest.approx(x.mean(), rel=1e-12)
        assert out["failed"] == 0 and out["used"] == G
        from scipy.stats import t
        lo, hi = out["intervals"]["error_rate"]
        q = t.ppf(0.975, G - 1)
        assert lo == pytest.approx(x.mean() - q * out["standard_errors"]["error_rate"], rel=1e-12)
        assert hi == pytest.approx(x.mean() + q * out["standard_errors"]["error_rate"], rel=1e-12)
        # a statistic that does not vary has no error
        assert out["standard_errors"]["coverage"] == 0.0 and out["standard_errors"]["genome_size"] == 0.0


def test_the_coverage_is_rescaled_and_the_genome_size_mapped():
    """Numbers worked by hand: three groups, c_g and occurrences such that the rescaled coverage is 10, 10.5, 9.5, and
    correct_c(c) = 0.8 c."""
    from covest_amd.jackknife import summarize_jackknife
    occ = [8000.0, 6000.0, 7600.0]
    est = [[8.0, 0.01], [6.3, 0.02], [7.22, 0.03]]            # * 10000 / occ = 10, 10.5, 9.5
    full = [10.0, 0.02]
    out = summarize_jackknife(est, [True] * 3, full, occ, 10000.0, NAMES, None, 0.9, _correct_c)
    # coverage: mean 10, deviations 0, .5, -.5 -> se = sqrt(2/3 * .5) ; bias 2 * (10 - 10) = 0
    assert out["mean"]["coverage"] == pytest.approx(10.0, rel=1e-12)
    assert out["standard_errors"]["coverage"] == pytest.approx(math.sqrt(2.0 / 3.0 * 0.5), rel=1e-12)
    assert abs(out["bias"]["coverage"]) < 1e-12
    # genome size: 8000 / 6.4 = 1250, 6000 / 5.04, 7600 / 5.776; the full one 10000 / 8 = 1250
    sizes = np.array([8000 / 6.4, 6000 / 5.04, 7600 / 5.776])
    m = sizes.mean()
    assert out["mean"]["genome_size"] == pytest.approx(m, rel=1e-12)
    assert out["standard_errors"]["genome_size"] == pytest.approx(math.sqrt(2.0 / 3.0 * ((sizes - m) ** 2).sum()), rel=1e-12)
    assert out["bias"]["genome_size"] == pytest.approx(2.0 * (m - 1250.0), rel=1e-9)
    assert out["bias_corrected"]["genome_size"] == pytest.approx(1250.0 - 2.0 * (m - 1250.0), rel=1e-12)
    # error rate: 0.01, 0.02, 0.03 against 0.02
    assert out["standard_errors"]["error_rate"] == pytest.approx(math.sqrt(2.0 / 3.0 * 2e-4), rel=1e-12)
    from scipy.stats import t
    lo, hi = out["intervals"]["error_rate"]
    assert hi - lo == pytest.approx(2 * t.ppf(0.95, 2) * out["standard_errors"]["error_rate"], rel=1e-12)


def test_fixed_parameters_failures_and_too_few_groups():
    from covest_amd.jackknife import summarize_jackknife
    est = [[9.0, 0.01], [9.1, 0.02], [8.9, 0.03], [50.0, 0.4]]
    occ = [9000.0, 9000.0, 9000.0, 9000.0]
    ok = [True, True, True, False]
    out = summarize_jackknife(est, ok, [10.0, 0.02], occ, 10000.0, NAMES, [None, 0.02], 0.95, _correct_c)
    assert out["failed"] == 1 and out["used"] == 3
    for key in ("mean", "standard_errors", "bias", "bias_corrected", "intervals"):
        assert out[key]["error_rate"] is None and out[key]["coverage"] is not None and out[key]["genome_size"] is not None
    # the failed replicate is left out: the same numbers without its row
    three = summarize_jackknife(est[:3], ok[:3], [10.0, 0.02], occ[:3], 10000.0, NAMES, [None, 0.02], 0.95, _correct_c)
    assert {k: three[k] for k in ("mean", "standard_errors", "bias", "intervals")} == \
           {k: out[k] for k in ("mean", "standard_errors", "bias", "intervals")} and three["failed"] == 0
    # the coverage fixed: the genome size goes with it
    out = summarize_jackknife(est, ok, [10.0, 0.02], occ, 10000.0, NAMES, [10.0, None], 0.95, _correct_c)
    assert out["standard_errors"]["coverage"] is None and out["standard_errors"]["genome_size"] is None
    assert out["standard_errors"]["error_rate"] is not None
    # fewer than two successful refits: everything None
    for ok in ([True, False, False, False], [False] * 4):
        out = summarize_jackknife(est, ok, [10.0, 0.02], occ, 10000.0, NAMES, None, 0.95, _correct_c)
        assert out["used"] == sum(ok) and out["failed"] == 4 - sum(ok)
        for key in ("mean", "standard_errors", "bias", "bias_corrected", "intervals"):
            assert set(out[key].values()) == {None} and set(out[key]) == {"coverage", "error_rate", "genome_size"}
    with pytest.raises(ValueError):
        summarize_jackknife(est, [True] * 4, [10.0, 0.02], occ, 10000.0, NAMES, None, 1.0, _correct_c)
    with pytest.raises(ValueError):
        summarize_jackknife(est, [True] * 3, [10.0, 0.02], occ, 10000.0, NAMES, None, 0.95, _correct_c)


# ---- the record
class _Stub:
    """What print_output touches of a model."""
    params = NAMES
    hist = {1: 100, 2: 50, 7: 3}
    k, r = 21, 100

    @staticmethod
    def short_name():
        return "basic"

    def compute_loglikelihood(self, *args):
        return -1000.0 - sum(args)

    def correct_c(self, c):
        return c * (self.r - self.k + 1) / self.r


def test_print_output_without_a_jackknife_is_todays_record():
    import yaml
    from covest_amd import __version__
    from covest_amd.jackknife import summarize_jackknife
    from covest_amd.report import print_output
    hist_orig = {1: 1000, 2: 400, 10: 20}
    args = dict(estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True)
    today = {'model': 'basic', 'hist_size': 7, 'sample_factor': 1, 'orig_sample_factor': 1, 'success': True,
             'version': __version__, 'starting_points': 1, 'use_grid_search': False,
             'guessed_coverage': 9.0, 'guessed_error_rate': 0.1, 'guessed_loglikelihood': -1009.1,
             'coverage': 10.0, 'error_rate': 0.05, 'orig_coverage': 10.0, 'loglikelihood': -1010.05, 'genome_size': 250}
    rec = print_output(hist_orig, _Stub(), True, 1, **args)
    assert rec == today and list(rec) == list(today)
    assert print_output(hist_orig, _Stub(), True, 1, jackknife=None, **args) == today
    est = [[9.0, 0.04], [9.1, 0.05], [8.9, 0.06]]
    jack = summarize_jackknife(est, [True] * 3, [10.0, 0.05], [1800.0] * 3, 2000.0, NAMES, [None, 0.05], 0.95, _Stub().correct_c)
    jack.update(groups=3, level=0.95)
    with_it = print_output(hist_orig, _Stub(), True, 1, jackknife=jack, **args)
    assert {k: v for k, v in with_it.items() if k in today} == today and list(with_it)[:len(today)] == list(today)
    assert set(with_it) - set(today) == {'jackknife_groups', 'jackknife_used', 'jackknife_failed', 'jackknife_level',
                                         'jackknife_se_coverage', 'jackknife_bias_coverage', 'jackknife_interval_coverage',
                                         'jackknife_se_genome_size', 'jackknife_bias_genome_size',
                                         'jackknife_interval_genome_size'}   # (the error rate is fixed: nothing of it)
    assert with_it['jackknife_se_coverage'] == jack['standard_errors']['coverage']
    assert yaml.safe_load(yaml.dump(with_it)) == with_it


# ---- argument errors, before the library is asked
def test_argument_errors_come_before_the_library(monkeypatch):
    from covest_amd import _capi, jackknife, sample

    def no_library():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_capi, "lib", no_library)
    reads = np.full((10, 30), ord("A"), dtype=np.uint8)
    for groups in (0, 257, 2.5, True, None):
        with pytest.raises(ValueError):
            sample.split_reads(reads, groups)
        with pytest.raises(ValueError):
            sample.read_groups(10, groups)
    with pytest.raises(ValueError):
        sample.split_reads(reads, 4, seed=-1)
    with pytest.raises(ValueError):
        sample.split_reads(reads, 4, seed=1 << 64)
    with pytest.raises(ValueError):
        sample.split_reads(reads, 4, first_read=-1)
    with pytest.raises(ValueError):
        sample.split_reads(reads.astype(np.int32), 4)
    with pytest.raises(ValueError):
        sample.split_reads((reads.reshape(-1), np.array([0, 20, 10])), 4)     # offsets descend
    with pytest.raises(ValueError):
        sample.read_groups(-1, 4)
    with pytest.raises(ValueError):
        sample.split_reads_device(16, 10, 16, 0, 4, read_len=5)               # no group_first
    with pytest.raises(ValueError):
        sample.split_reads_device(16, 10, 16, 16, 4, offsets_ptr=16)          # offsets without out_offsets
    with pytest.raises(ValueError):
        sample.split_reads_device(16, -1, 16, 16, 4)
    for groups in (1, 0, 257, 2.0):
        with pytest.raises(ValueError):
            jackknife.leave_group_out_histograms(reads, 9, groups)
    with pytest.raises(ValueError):
        jackknife.leave_group_out_histograms(reads, 0, 4)

    class Model:
        params = NAMES
        k, tail = 9, 0
    est = [10.0, 0.02]
    with pytest.raises(ValueError, match="sample factor"):
        jackknife.read_jackknife(Model(), est, reads, sample_factor=2)
    sampled = Model()
    sampled.sample_factor = 3
    with pytest.raises(ValueError, match="sample factor"):
        jackknife.read_jackknife(sampled, est, reads)
    for bad in (dict(groups=1), dict(groups=257), dict(refit="sequential"), dict(level=1.0), dict(fix=[None]), dict(trim=0),
                dict(refit="lockstep", gradient="analytic"), dict(refit="lockstep-gradient", gradient="fd"), dict(seed=-1)):
        with pytest.raises(ValueError):
            jackknife.read_jackknife(Model(), est, reads, **bad)
    with pytest.raises(ValueError):
        jackknife.read_jackknife(Model(), est[:1], reads)


def test_the_shared_checks_word_their_messages_as_before(hip_lib):
    """The texts of the checks the split shares with the sampler (csrc/reads_args.h), byte for byte as the split worded
    them on its own, between its own two: the groups are looked at first, group_first last."""
    import ctypes
    bases = np.full(64, 65, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    offsets = np.arange(9, dtype=np.int64) * 8
    out_offsets = np.full(9, -1, dtype=np.int64)
    first_of = np.full(5, -1, dtype=np.int64)

    def host(n=8, L=8, first=0, groups=4, offs=None, out_offs=None, gf=first_of.ctypes.data):
        return hip_lib.covest_split_reads(-1, bases.ctypes.data, offs, n, L, first, groups, 1, out.ctypes.data, out_offs, None, gf)

    def device(n=8, L=8, first=0, groups=4, offs=None, out_offs=None, gf=first_of.ctypes.data):
        return hip_lib.covest_split_reads_device(-1, bases.ctypes.data, offs, n, L, first, groups, 1, out.ctypes.data, out_offs,
                                                 None, gf, None)

    def said(status):
        assert status == -1
        return hip_lib.covest_last_error().decode()

    for fn, name in ((host, "covest_split_reads"), (device, "covest_split_reads_device")):
        assert said(fn(n=-1, groups=257)) == name + ": groups must be within 1 .. 256"
        assert said(fn(n=-1, L=-1, gf=None)) == name + ": n_reads and first_read must not be negative"
        assert said(fn(first=-1)) == name + ": n_reads and first_read must not be negative"
        assert said(fn(L=-1, first=(1 << 63) - 4)) == name + ": without offsets read_len must not be negative"
        assert said(fn(first=(1 << 63) - 8)) == name + ": more reads than 64-bit offsets reach"
        assert said(fn(n=1 << 62, L=100)) == name + ": more reads than 64-bit offsets reach"
        assert said(fn(offs=offsets.ctypes.data, gf=None)) == name + ": reads of their own lengths need an array for the output offsets"
        assert said(fn(gf=None)) == name + ": group_first is null"
    bad = offsets.copy()
    bad[8] = 50
    assert said(host(offs=bad.ctypes.data, out_offs=out_offsets.ctypes.data)) == "covest_split_reads: offsets descend at read 7"
    bad = offsets - 1
    assert said(host(offs=bad.ctypes.data, out_offs=out_offsets.ctypes.data)) == "covest_split_reads: negative offset"
    assert (first_of == -1).all() and not out.any()


def test_the_header_states_the_rule_and_the_stream_table_has_its_row():
    import os
    from conftest import REPO
    header = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    assert "(lo32(r), hi32(r), 0, 8)" in header and "group(r) = (w * G) >> 32" in header
    philox = open(os.path.join(REPO, "covest_amd", "csrc", "sim_philox.h")).read()
    assert "kStreamGroup = 8" in philox
    from covest_amd import _capi, sample
    assert {"covest_split_reads", "covest_split_reads_device"} <= set(_capi.EXPORTS)
    # the constants the GPU sweep is built round are the kernels'
    import re
    text = open(os.path.join(REPO, "covest_amd", "csrc", "split.h")).read()
    const = {name: int(value) for name, value in re.findall(r"constexpr int (k\w+) = (\d+);", text)}
    assert const["kSplitMaxGroups"] == sample.MAX_GROUPS
    assert const["kSplitThreads"] * const["kSplitPerLane"] == sample.SPLIT_SHARE >= sample.MAX_GROUPS
    assert const["kSplitScanThreads"] * const["kSplitScanPerLane"] == sample.SPLIT_SCAN_PASS
