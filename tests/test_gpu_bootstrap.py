"""The parametric bootstrap end to end on the device (covest_amd.bootstrap): the basic model on
sim_c10_e0.05.hist, estimated by the existing flow, then 16 model-drawn histograms refitted -- reproducible, every
refit inside the bounds, and the bootstrap's standard errors against the Wald ones within a factor 2 of the ratio
profiles/bootstrap_recovery.txt records for B = 64; and the repeat model on H10k_rep_trim.hist, determinism only."""
import math
import os

import numpy as np
import pytest

from conftest import REPO, load_golden, load_hist

pytestmark = pytest.mark.gpu

SEED = 20240702  # (tools/bootstrap_recovery.py uses seed 1)


def recorded_se_ratio(block):
    """{parameter: bootstrap se / Wald se} from the '# se ratio, BLOCK NAME VALUE' lines of profiles/bootstrap_recovery.txt."""
    out = {}
    with open(os.path.join(REPO, "profiles", "bootstrap_recovery.txt")) as f:
        for line in f:
            if line.startswith("# se ratio, %s " % block):
                _, name, value = line.split(",", 1)[1].split()
                out[name] = float(value)
    return out


def test_basic_model_bootstrap_against_the_record(hip_lib):
    """The factor 2 covers the roughly 18 % sampling error of a standard deviation from 16 values, with room for the
    difference between two seeds; the bound moves with the record, not with this test's own figures."""
    from covest_amd import BasicModel, CoverageEstimator, constants, observed_information, parametric_bootstrap
    from covest_amd.hist_steps import process_histogram
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sf, guess_c, guess_e = process_histogram(hist_orig, 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    est, ok = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage([guess_c, guess_e])
    assert ok
    runs = [parametric_bootstrap(model, est, replicates=16, seed=SEED, hist_orig=hist_orig, sample_factor=sf,
                                 err_scale=constants.DEFAULT_ERR_SCALE) for _ in range(2)]
    a, b = runs
    assert a["estimates"].shape == (16, 2) and a["estimates"].tobytes() == b["estimates"].tobytes()
    assert a["loglikelihood"].tobytes() == b["loglikelihood"].tobytes()
    assert a["n_draws"] == sum(hist.values()) + tail and a["failed"] == 0 and a["success"].all()
    assert not a["at_bound"].any()
    for d, (lo, hi) in enumerate(model.bounds):
        assert (a["estimates"][:, d] > lo).all() and (hi is None or (a["estimates"][:, d] < hi).all())
    info = observed_information(model, est)
    recorded = recorded_se_ratio("basic")
    assert set(recorded) == {"coverage", "error_rate"}
    for name in ("coverage", "error_rate"):
        assert math.isfinite(a["bias"][name]) and math.isfinite(a["standard_errors"][name])
        lo, hi = a["percentile_intervals"][name]
        assert lo <= a["mean"][name] <= hi
        ratio = a["standard_errors"][name] / info["standard_errors"][name]
        print("%-10s bias %.3g, bootstrap se %.4g, Wald se %.4g, ratio %.3f (recorded for B = 64: %.3f)"
              % (name, a["bias"][name], a["standard_errors"][name], info["standard_errors"][name], ratio, recorded[name]))
        assert recorded[name] / 2 <= ratio <= recorded[name] * 2, (name, ratio, recorded[name])
    assert math.isfinite(a["genome_size"]["mean"]) and a["genome_size"]["interval"][0] <= a["genome_size"]["interval"][1]
    model.close()


def test_repeats_model_bootstrap_is_reproducible(hip_lib):
    """H10k_rep_trim.hist at its golden optimum (the best candidate of tests/golden/c3_trim.json, q2 = 0.5): determinism,
    finiteness and the shape of the result only -- the q components are printed, not asserted."""
    from covest_amd import RepeatsModel, parametric_bootstrap
    g = load_golden("c3_trim.json")
    cand = g["candidates"]
    at = np.unravel_index(cand["flat_index"][int(np.argmax(cand["ll"]))], [len(a) for a in g["axes"]])
    c, e, q1, q = (g["axes"][d][i] for d, i in enumerate(at))
    point = [c, e, q1, g["q2"], q]
    model = RepeatsModel(g["k"], g["r"], load_hist(g["hist"]), g["tail"], max_error=g["max_error"])
    a, b = (parametric_bootstrap(model, point, replicates=4, seed=SEED) for _ in range(2))
    assert a["estimates"].shape == (4, 5) and a["at_bound"].shape == (4, 5) and a["success"].shape == (4,)
    assert a["estimates"].tobytes() == b["estimates"].tobytes() and a["success"].tolist() == b["success"].tolist()
    assert np.isfinite(a["estimates"]).all() and np.isfinite(a["loglikelihood"]).all()
    assert a["n_draws"] == sum(model.hist.values()) + g["tail"]
    assert set(a["bias"]) == set(model.params) and "genome_size" not in a
    for name in model.params:
        print("%-10s point %.6g mean %s bias %s se %s" % (name, point[model.params.index(name)], a["mean"][name],
                                                          a["bias"][name], a["standard_errors"][name]))
    model.close()
