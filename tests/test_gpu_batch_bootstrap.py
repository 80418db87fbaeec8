"""The parametric bootstrap with lock-step refits (parametric_bootstrap(refit="lockstep")): the
replicates drawn into a HistogramBatch, all refits advancing together on one loglikelihood_pairs launch per round --
against the sequential route (a twin model per replicate), on the set-up of test_gpu_bootstrap.py."""
import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err

pytestmark = pytest.mark.gpu

SEED = 20240702  # test_gpu_bootstrap.py's


def test_basic_model_lockstep_against_sequential(hip_lib):
    """The two routes evaluate with different kernels (the batch's table and pairs dot; the twin's recurrence kernel),
    so L-BFGS-B may stop a step apart: what is asserted is the log-likelihood of either estimate by the SAME sequential
    twin model, to 1e-6 relative -- the bound test_gpu_parity.py puts on a refinement's final value.  The parameters are
    printed side by side."""
    from covest_amd import BasicModel, CoverageEstimator, constants, model_cells, parametric_bootstrap
    from covest_amd.bootstrap import _replicate_model, draw_histograms
    from covest_amd.hist_steps import process_histogram
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sf, guess_c, guess_e = process_histogram(hist_orig, 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    est, ok = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage([guess_c, guess_e])
    assert ok
    options = dict(replicates=16, seed=SEED, hist_orig=hist_orig, sample_factor=sf, err_scale=constants.DEFAULT_ERR_SCALE)
    a, b = (parametric_bootstrap(model, est, refit="lockstep", **options) for _ in range(2))
    seq = parametric_bootstrap(model, est, **options)
    assert a["refit"] == b["refit"] == "lockstep" and seq["refit"] == "sequential"
    assert set(a) == set(seq)
    assert a["estimates"].shape == (16, 2) and a["estimates"].tobytes() == b["estimates"].tobytes()
    assert a["loglikelihood"].tobytes() == b["loglikelihood"].tobytes() and a["success"].tolist() == b["success"].tolist()
    assert a["n_draws"] == seq["n_draws"] == sum(hist.values()) + tail
    assert a["failed"] == 0 and a["success"].all() and not a["at_bound"].any()
    for d, (lo, hi) in enumerate(model.bounds):
        assert (a["estimates"][:, d] > lo).all() and (hi is None or (a["estimates"][:, d] < hi).all())
    keys, weights, has_tail = model_cells(model, est)
    counts = draw_histograms(weights, a["n_draws"], 16, seed=SEED, device=model.device)
    for r in range(16):
        twin = _replicate_model(model, keys, counts[r, :len(keys)], int(counts[r, len(keys)]) if has_tail else 0)
        try:
            ll_lock = twin.compute_loglikelihood(*a["estimates"][r])
            ll_seq = twin.compute_loglikelihood(*seq["estimates"][r])
        finally:
            twin.close()
        print("replicate %2d  lock-step %s (LL %.10g)  sequential %s (LL %.10g)"
              % (r, a["estimates"][r].tolist(), ll_lock, seq["estimates"][r].tolist(), ll_seq))
        assert rel_err(ll_lock, ll_seq) <= 1e-6, (r, ll_lock, ll_seq)
        assert np.isfinite(a["loglikelihood"][r])
    model.close()


def test_lockstep_honours_fix(hip_lib):
    from covest_amd import BasicModel, constants, parametric_bootstrap
    from covest_amd.hist_steps import process_histogram
    hist, tail, _, guess_c, guess_e = process_histogram(load_hist("sim_c10_e0.05"), 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    scale = constants.DEFAULT_ERR_SCALE  # (`fix` is in the optimiser's space, where the error rate is scaled)
    out = parametric_bootstrap(model, [guess_c, guess_e], replicates=3, seed=SEED, fix=[None, guess_e * scale],
                               refit="lockstep", err_scale=scale)
    assert out["estimates"][:, 1].tolist() == pytest.approx([guess_e] * 3, rel=1e-14) and out["mean"]["error_rate"] is None
    assert len(set(out["estimates"][:, 0].tolist())) == 3  # the free parameter moved, each replicate its own way
    assert np.isfinite(out["estimates"]).all() and out["mean"]["coverage"] is not None
    model.close()


def test_repeats_model_lockstep_is_reproducible(hip_lib):
    """H10k_rep_trim.hist at its golden optimum, 4 replicates: determinism and finiteness only."""
    from covest_amd import RepeatsModel, parametric_bootstrap
    g = load_golden("c3_trim.json")
    cand = g["candidates"]
    at = np.unravel_index(cand["flat_index"][int(np.argmax(cand["ll"]))], [len(a) for a in g["axes"]])
    c, e, q1, q = (g["axes"][d][i] for d, i in enumerate(at))
    point = [c, e, q1, g["q2"], q]
    model = RepeatsModel(g["k"], g["r"], load_hist(g["hist"]), g["tail"], max_error=g["max_error"])
    a, b = (parametric_bootstrap(model, point, replicates=4, seed=SEED, refit="lockstep") for _ in range(2))
    assert a["estimates"].shape == (4, 5) and a["at_bound"].shape == (4, 5) and a["success"].shape == (4,)
    assert a["estimates"].tobytes() == b["estimates"].tobytes() and a["success"].tolist() == b["success"].tolist()
    assert a["loglikelihood"].tobytes() == b["loglikelihood"].tobytes()
    assert np.isfinite(a["estimates"]).all() and np.isfinite(a["loglikelihood"]).all()
    assert a["n_draws"] == sum(model.hist.values()) + g["tail"] and a["refit"] == "lockstep"
    model.close()
