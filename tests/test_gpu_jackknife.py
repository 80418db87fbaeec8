"""The delete-a-group jackknife over reads on the device (covest_amd/jackknife.py over split_reads.hip, the k-mer counter
and the histogram batch): the leave-out histograms are exact integers and are held against the host counter
(tests/kmer_reference.py) on the reads the split puts outside each group; read_jackknife's summary is recomputed in numpy
from the refits it returns.  No statistical assertion: how close the jackknife error comes to the empirical spread is a
measurement (tools/jackknife_recovery.py, profiles/jackknife_recovery.txt)."""
import functools
import math

import numpy as np
import pytest

import kmer_reference as kr
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_KERNELS = 1e-10  # between two kernels of the library (tests/test_gpu_batch.py)
SEED = 11


def as_dict(hist_list):
    return {i: v for i, v in enumerate(hist_list) if i > 0 and v > 0}


def texts(bases, offsets=None):
    if offsets is None:
        return [row.tobytes().decode() for row in bases]
    blob = bases.tobytes().decode()
    return [blob[offsets[i]:offsets[i + 1]] for i in range(offsets.size - 1)]


@functools.lru_cache(maxsize=None)
def small_reads():
    """400 simulated reads of 50 bases from a 2 000-base genome."""
    from covest_amd import simulate as sim
    g = sim.random_genome(2000, 5)
    return sim.simulate_reads(g, 50, n_reads=400, error_rate=0.02, seed=5, first_read=0)


def check_leave_out(reads, read_texts, k, groups, canonical=False):
    from covest_amd import jackknife, sample
    full, hists, occ = jackknife.leave_group_out_histograms(reads, k, groups, seed=SEED, canonical=canonical)
    group = sample.read_groups(len(read_texts), groups, seed=SEED)
    assert full == as_dict(kr.histogram(read_texts, k, canonical)[0])
    assert len(hists) == groups == len(occ)
    for g in range(groups):
        outside = [t for t, of in zip(read_texts, group) if of != g]
        assert hists[g] == as_dict(kr.histogram(outside, k, canonical)[0]), g
        assert occ[g] == sum(i * n for i, n in hists[g].items()), g
    return full, hists, occ, group


@pytest.mark.parametrize("k,canonical", [(9, False), (9, True), (33, False)])
def test_leave_out_histograms_are_the_host_counters(hip_lib, k, canonical):
    reads = small_reads()
    full, hists, occ, group = check_leave_out(reads, texts(reads.bases), k, 4, canonical)
    # every read of L bases has L - k + 1 k-mers: the occurrences are those of the reads outside the group
    assert occ == [int((group != g).sum()) * (50 - k + 1) for g in range(4)]


def test_leave_out_histograms_of_ragged_reads(hip_lib):
    reads = small_reads()
    rng = np.random.default_rng(8)
    lens = rng.choice((0, 5, 8, 9, 10, 30, 50), size=400)       # empty reads and reads shorter than k among them
    offsets = np.zeros(401, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.concatenate([reads.bases[i, :lens[i]] for i in range(400)])
    check_leave_out((bases, offsets), texts(bases, offsets), 9, 4)


def test_two_groups_are_each_others_complement(hip_lib):
    from covest_amd import jackknife, kmer_hist as kh, sample
    reads = small_reads()
    full, hists, occ = jackknife.leave_group_out_histograms(reads, 9, 2, seed=SEED)
    split = sample.split_reads(reads, 2, seed=SEED)
    for g in (0, 1):  # leaving group g out is counting group 1 - g alone
        counts = kh.KmerCounts(9)
        counts.add_reads(texts(split.group(1 - g)))
        assert as_dict(counts.histogram()) == hists[g], g
        counts.close()
    with pytest.raises(ValueError):
        jackknife.leave_group_out_histograms(reads, 9, 1)


def test_a_read_index_that_crosses_a_word_inside_the_set(hip_lib):
    """A SimulatedReads carries its own first_read into the split and into the bootstrap's weights: reads 2^32 - 200 ..
    2^32 + 199."""
    import bootstrap_weights_reference as bw
    from covest_amd import jackknife, sample, simulate as sim
    from covest_amd.read_bootstrap import bootstrap_histograms
    first_read = (1 << 32) - 200
    reads = sim.simulate_reads(sim.random_genome(2000, 5), 50, n_reads=400, error_rate=0.02, seed=5, first_read=first_read)
    strings = texts(reads.bases)
    want_full = as_dict(kr.histogram(strings, 9)[0])
    full, hists, occ = jackknife.leave_group_out_histograms(reads, 9, 4, seed=SEED)
    group = sample.read_groups(400, 4, SEED, first_read=first_read)
    assert not np.array_equal(group, sample.read_groups(400, 4, SEED))      # (the groups do depend on the numbering)
    assert full == want_full and len(hists) == len(occ) == 4
    for g in range(4):
        assert hists[g] == as_dict(kr.histogram([t for t, of in zip(strings, group) if of != g], 9)[0]), g
        assert occ[g] == int((group != g).sum()) * (50 - 9 + 1), g
    full, hists, occ, drawn = bootstrap_histograms(reads, 9, 3, seed=SEED)
    assert full == want_full and len(hists) == len(occ) == len(drawn) == 3
    for b in range(3):
        w = bw.weights(400, b, SEED, first_read=first_read)
        assert hists[b] == as_dict(kr.histogram(bw.expand(strings, w), 9)[0]), b
        assert drawn[b] == int(w.sum()) and occ[b] == drawn[b] * (50 - 9 + 1), b


@functools.lru_cache(maxsize=None)
def fitted():
    """(reads, model, estimate) of the basic model on simulated reads: 50 000-base genome, coverage 10, e = 0.02, k = 15."""
    from covest_amd import constants, simulate as sim
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import compute_coverage_apx
    from covest_amd.kmer_hist import KmerCounts
    from covest_amd.models import BasicModel
    g = sim.random_genome(50_000, 21)
    reads = sim.simulate_reads(g, 100, coverage=10, error_rate=0.02, seed=21, both_strands=False)
    counts = reads.add_to(KmerCounts(15))
    hist = as_dict(counts.histogram())
    counts.close()
    model = BasicModel(15, 100, hist, 0, max_error=constants.MAX_ERRORS)
    est, ok = CoverageEstimator(model).compute_coverage(list(compute_coverage_apx(hist, 15, 100)))
    assert ok
    return reads, model, [float(v) for v in est], hist


def recompute(out, model):
    """read_jackknife's summary from its own `estimates`, in numpy."""
    from scipy.stats import t
    ok = np.asarray(out["success"], dtype=bool)
    est = np.asarray(out["estimates"])[ok]
    occ = np.asarray(out["occurrences"], dtype=np.float64)[ok]
    used = int(ok.sum())
    full = out["full_estimate"]
    columns = {name: est[:, d] for d, name in enumerate(out["params"])}
    columns["coverage"] = est[:, 0] * out["occurrences_full"] / occ
    columns["genome_size"] = occ / np.array([model.correct_c(c) for c in est[:, 0]])
    at_full = dict(zip(out["params"], full), genome_size=out["occurrences_full"] / model.correct_c(full[0]))
    q = t.ppf(0.5 * (1 + out["level"]), used - 1)
    want = {}
    for name, v in columns.items():
        mean = v.mean()
        se = math.sqrt((used - 1) / used * ((v - mean) ** 2).sum())
        bias = (used - 1) * (mean - at_full[name])
        want[name] = (mean, se, bias, at_full[name] - bias, [at_full[name] - q * se, at_full[name] + q * se])
    return want, used


@pytest.mark.parametrize("refit", ["lockstep", "lockstep-gradient"])
def test_read_jackknife_basic_model(hip_lib, refit):
    from covest_amd import jackknife
    reads, model, est, hist = fitted()
    G = 8
    out = jackknife.read_jackknife(model, est, reads, groups=G, seed=SEED, refit=refit)
    assert out["groups"] == G and out["refit"] == refit and out["seed"] == SEED and out["estimates"].shape == (G, 2)
    assert sum(out["group_sizes"]) == reads.n_reads and len(out["group_sizes"]) == G
    assert out["occurrences_full"] == sum(i * n for i, n in hist.items())
    assert out["occurrences"] == [(reads.n_reads - m) * (100 - 15 + 1) for m in out["group_sizes"]]
    assert out["failed"] + out["used"] == G and out["used"] >= 2
    assert out["full_minus_given"] == [a - b for a, b in zip(out["full_estimate"], est)]
    want, used = recompute(out, model)
    assert used == out["used"]
    for name, (mean, se, bias, corrected, interval) in want.items():
        for key, value in (("mean", mean), ("standard_errors", se), ("bias_corrected", corrected)):
            assert rel_err(out[key][name], value) <= 1e-12, (name, key, out[key][name], value)
        # (the bias is (G' - 1) times a difference of two nearly equal numbers: its error is the mean's, G' - 1 times)
        assert abs(out["bias"][name] - bias) <= 1e-12 * max(abs(mean), abs(bias)) * used, (name, out["bias"][name], bias)
        assert all(rel_err(a, b) <= 1e-12 for a, b in zip(out["intervals"][name], interval)), name
        print("%-12s full %.6g jackknife se %.4g bias %.3g" % (name, dict(zip(out["params"], out["full_estimate"]),
              genome_size=out["occurrences_full"] / model.correct_c(out["full_estimate"][0]))[name], se, bias))
    # the same seed: the same bytes; another seed: other groups
    again = jackknife.read_jackknife(model, est, reads, groups=G, seed=SEED, refit=refit)
    assert again["estimates"].tobytes() == out["estimates"].tobytes() and again["group_sizes"] == out["group_sizes"]
    assert again["standard_errors"] == out["standard_errors"]
    if refit == "lockstep-gradient":
        other = jackknife.read_jackknife(model, est, reads, groups=G, seed=SEED + 1, refit=refit)
        assert other["group_sizes"] != out["group_sizes"] and other["occurrences"] != out["occurrences"]
        # fix= is honoured: the error rate stays, and has no summary
        fixed = jackknife.read_jackknife(model, est, reads, groups=G, seed=SEED, refit=refit, fix=[None, est[1]])
        assert fixed["estimates"][:, 1].tolist() + [fixed["full_estimate"][1]] == pytest.approx([est[1]] * (G + 1), rel=1e-14)
        assert len(set(fixed["estimates"][:, 0].tolist())) == G  # the free parameter moved, each leave-out set its own way
        assert fixed["standard_errors"]["error_rate"] is None and fixed["standard_errors"]["coverage"] is not None


def test_the_full_row_scores_as_the_model(hip_lib):
    """Row G of the batch is the model's own histogram on the model's own keys where the union adds none: its
    log-likelihood at the estimate is the model's, between two kernels."""
    from covest_amd import jackknife
    from covest_amd.hist_steps import trim_hist
    from covest_amd.models import BasicModel
    from covest_amd import constants
    reads, model, est, hist = fitted()
    G = 8
    full, hists, _ = jackknife.leave_group_out_histograms(reads, 15, G, seed=SEED)
    assert full == hist
    trimmed = BasicModel(15, 100, *trim_hist(hist, 12), max_error=constants.MAX_ERRORS)
    assert trimmed.tail > 0
    for m, trim in ((model, None), (trimmed, 12), (trimmed, None)):
        twin, batch, added = jackknife.jackknife_batch(m, hists, full, trim)
        try:
            assert len(batch) == G + 1
            if added == 0:
                got = float(batch.loglikelihood_pairs([G], [est])[0])
                want = float(m.compute_loglikelihood(*est))
                assert rel_err(got, want) <= TOL_KERNELS, (trim, got, want)
            counts, tails = batch.counts()
            assert counts[G].sum() + tails[G] == sum(hist.values())
            if m is trimmed:
                assert (tails > 0).all() and added == 0
        finally:
            batch.close()
            twin.close()
    trimmed.close()
