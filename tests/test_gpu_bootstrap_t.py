"""The studentized (bootstrap-t) interval of the parametric bootstrap (parametric_bootstrap(studentized=True), DESIGN.md
section 6x): every replicate's observed information at its own refit from ONE HistogramBatch.loglikelihood_hessian_pairs
call, against observed_information of a twin model per replicate; the interval arithmetic recomputed from what the call
returns; the result's keys with and without; and the free-set rule on the repeat model with q1 on its bound."""
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist

pytestmark = pytest.mark.gpu

SEED = 20240702  # test_gpu_bootstrap.py's
B = 32
KEYS_TODAY = {'replicates', 'seed', 'n_draws', 'level', 'params', 'estimate', 'estimates', 'success', 'loglikelihood', 'at_bound',
              'refit', 'mean', 'bias', 'standard_errors', 'percentile_intervals', 'failed', 'genome_size'}
KEYS_STUDENTIZED = {'replicate_standard_errors', 'studentized_used', 't_intervals'}


def _basic_model():
    from covest_amd import BasicModel, constants
    from covest_amd.hist_steps import process_histogram
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sf, _, _ = process_histogram(hist_orig, 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    opt = load_golden("own_optimum.json")["models"]["basic"]
    return model, [opt[name] for name in model.params], hist_orig, sf


@pytest.mark.parametrize("refit", ["lockstep-gradient", "sequential"])
def test_basic_model(hip_lib, refit):
    from covest_amd import HistogramBatch, constants, observed_information, parametric_bootstrap
    from covest_amd.bootstrap import _replicate_model
    model, est, hist_orig, sf = _basic_model()
    options = dict(replicates=B, seed=SEED, hist_orig=hist_orig, sample_factor=sf, err_scale=constants.DEFAULT_ERR_SCALE, refit=refit)
    out = parametric_bootstrap(model, est, studentized=True, **options)
    names = list(model.params)
    assert set(out) == KEYS_TODAY | KEYS_STUDENTIZED and out["refit"] == refit
    rse = out["replicate_standard_errors"]
    assert rse.shape == (B, 2) and out["estimates"].shape == (B, 2)
    # three replicates against a twin model each, on the rows the batch holds
    batch = HistogramBatch.draw(model, est, B, seed=SEED, n_draws=out["n_draws"])
    counts, tails = batch.counts()
    batch.close()
    keys = list(model.hist.keys())
    for r in (0, B // 2, B - 1):
        twin = _replicate_model(model, keys, counts[r], tails[r])
        try:
            info = observed_information(twin, out["estimates"][r])
        finally:
            twin.close()
        for d, name in enumerate(names):
            want = info["standard_errors"][name]
            print("%s replicate %d %s: se %r, twin %r" % (refit, r, name, rse[r, d], want))
            if want is None:
                assert math.isnan(rse[r, d])
            else:
                assert abs(rse[r, d] - want) <= 1e-8 * want, (r, name, rse[r, d], want)
    # the intervals, recomputed from what the call returned and the original's own standard errors
    original = observed_information(model, est)
    lo_q, hi_q = 50.0 * (1.0 - out["level"]), 50.0 * (1.0 + out["level"])
    for d, name in enumerate(names):
        take = out["success"] & np.isfinite(rse[:, d])
        assert out["studentized_used"][name] == int(take.sum()) <= B - out["failed"]
        se = original["standard_errors"][name]
        assert se is not None and take.sum() >= 2
        t = (out["estimates"][take, d] - est[d]) / rse[take, d]
        q_lo, q_hi = np.percentile(t, [lo_q, hi_q])
        iv = out["t_intervals"][name]
        assert iv == [est[d] - q_hi * se, est[d] - q_lo * se], (name, iv)
        assert math.isfinite(iv[0]) and math.isfinite(iv[1]) and iv[0] < iv[1]
        print("%s %s: t-interval %r, percentile %r, used %d" % (refit, name, iv, out["percentile_intervals"][name], take.sum()))
    size = out["genome_size"]
    occurrences = sum(i * h for i, h in hist_orig.items())
    c_lo, c_hi = out["t_intervals"]["coverage"]
    assert size["t_interval"] == [occurrences / model.correct_c(c_hi * sf), occurrences / model.correct_c(c_lo * sf)]
    assert size["t_interval"][0] < size["t_interval"][1] and set(size) == {"mean", "standard_error", "interval", "t_interval"}
    # without: today's dict, key for key, and the same refits
    plain = parametric_bootstrap(model, est, **options)
    assert set(plain) == KEYS_TODAY and set(plain["genome_size"]) == {"mean", "standard_error", "interval"}
    assert plain["estimates"].tobytes() == out["estimates"].tobytes() and plain["success"].tolist() == out["success"].tolist()
    for key in ("mean", "bias", "standard_errors", "percentile_intervals", "failed"):
        assert plain[key] == out[key]
    model.close()


def test_report_records_the_t_intervals_only_when_present(hip_lib):
    from covest_amd import constants, parametric_bootstrap, print_output
    model, est, hist_orig, sf = _basic_model()
    options = dict(replicates=8, seed=SEED, hist_orig=hist_orig, sample_factor=sf, err_scale=constants.DEFAULT_ERR_SCALE,
                   refit="lockstep-gradient")
    with_t = print_output(hist_orig, model, True, sf, estimated=est, silent=True,
                          bootstrap=parametric_bootstrap(model, est, studentized=True, **options))
    without = print_output(hist_orig, model, True, sf, estimated=est, silent=True, bootstrap=parametric_bootstrap(model, est, **options))
    new = {"bootstrap_t_interval_coverage", "bootstrap_t_interval_error_rate", "bootstrap_t_interval_genome_size"}
    assert set(with_t) - set(without) == new and not set(without) - set(with_t)
    assert all(with_t[k] == without[k] for k in without if k != "loglikelihood")
    lo, hi = with_t["bootstrap_t_interval_coverage"]
    assert lo < hi
    model.close()


def test_the_free_set_rule_on_the_repeat_model(hip_lib):
    """H10k_rep_trim.hist at its golden optimum with q1 on its bound 1 (and held there): threshold_o is 2, (1 - q1)
    annihilates q2's and q's rows in every replicate as in the original -- None in t_intervals, NaN columns in the replicate
    standard errors -- and every replicate's (coverage, error rate) block is inverted.  (The point is not the optimum of
    the ORIGINAL histogram under q1 = 1, so the original's own block need not be positive definite: where it has no
    standard error the interval is None, by the rule, and that is what is asserted.)"""
    from covest_amd import RepeatsModel, observed_information, parametric_bootstrap
    g = load_golden("c3_trim.json")
    cand = g["candidates"]
    at = np.unravel_index(cand["flat_index"][int(np.argmax(cand["ll"]))], [len(a) for a in g["axes"]])
    c, e, q1, q = (g["axes"][d][i] for d, i in enumerate(at))
    point = [c, e, 1.0, g["q2"], q]
    model = RepeatsModel(g["k"], g["r"], load_hist(g["hist"]), g["tail"], max_error=g["max_error"])
    fix = [None, None, 1.0, None, None]
    out = parametric_bootstrap(model, point, replicates=6, seed=SEED, refit="lockstep-gradient", studentized=True, fix=fix)
    original = observed_information(model, point, fix)
    assert not set(original["free"]) & {2, 3, 4}
    rse = out["replicate_standard_errors"]
    assert rse.shape == (6, 5) and np.all(out["estimates"][:, 2] == 1.0)
    assert np.all(np.isnan(rse[:, 2:]))
    assert out["t_intervals"]["q1"] is None and out["t_intervals"]["q2"] is None and out["t_intervals"]["q"] is None
    assert out["studentized_used"]["q1"] == out["studentized_used"]["q2"] == out["studentized_used"]["q"] == 0
    ok = out["success"]
    assert np.all(np.isfinite(rse[ok][:, :2])) and np.all(rse[ok][:, :2] > 0)
    for name in ("coverage", "error_rate"):
        assert out["studentized_used"][name] == int(ok.sum()) <= 6 - out["failed"]
        iv = out["t_intervals"][name]
        assert (iv is None) == (original["standard_errors"][name] is None or ok.sum() < 2)
        if iv is not None:
            assert math.isfinite(iv[0]) and math.isfinite(iv[1]) and iv[0] < iv[1]
    model.close()
