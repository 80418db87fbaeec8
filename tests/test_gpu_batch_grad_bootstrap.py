"""The parametric bootstrap with lock-step refits by the batch's analytic gradient
(parametric_bootstrap(refit="lockstep-gradient")): the replicates drawn into a HistogramBatch, one
CoverageEstimator(gradient="analytic") per replicate, a round ONE loglikelihood_gradient_pairs call -- against the
sequential route with gradient="analytic" (a twin model per replicate through the derivative kernel), on the set-up of
tests/test_gpu_batch_bootstrap.py."""
import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err

pytestmark = pytest.mark.gpu

SEED = 20240702  # test_gpu_bootstrap.py's


def _basic_model():
    from covest_amd import BasicModel, constants
    from covest_amd.hist_steps import process_histogram
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sf, _, _ = process_histogram(hist_orig, 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    opt = load_golden("own_optimum.json")["models"]["basic"]
    return model, [opt[name] for name in model.params], hist_orig, sf


def test_basic_model_against_sequential_analytic(hip_lib):
    """sim_c10_e0.05 at its recorded optimum, 8 replicates.  The two routes evaluate with different sums (the batch's
    uncompensated dot products; the twin's compensated segment sums), so L-BFGS-B may stop a step apart: what is asserted
    is the log-likelihood of either route's estimate by the SAME sequential twin model, to 1e-6 relative -- the bound of
    tests/test_gpu_batch_bootstrap.py, for its stated reason -- and that both routes report the same number of
    successful refits.  Two runs give identical bytes."""
    from covest_amd import constants, model_cells, parametric_bootstrap
    from covest_amd.bootstrap import _replicate_model, draw_histograms
    model, est, hist_orig, sf = _basic_model()
    options = dict(replicates=8, seed=SEED, hist_orig=hist_orig, sample_factor=sf, err_scale=constants.DEFAULT_ERR_SCALE)
    a, b = (parametric_bootstrap(model, est, refit="lockstep-gradient", **options) for _ in range(2))
    seq = parametric_bootstrap(model, est, gradient="analytic", **options)
    assert a["refit"] == b["refit"] == "lockstep-gradient" and seq["refit"] == "sequential"
    assert set(a) == set(seq)
    assert a["estimates"].shape == (8, 2) and a["estimates"].tobytes() == b["estimates"].tobytes()
    assert a["loglikelihood"].tobytes() == b["loglikelihood"].tobytes() and a["success"].tolist() == b["success"].tolist()
    assert a["n_draws"] == seq["n_draws"] == sum(model.hist.values()) + model.tail
    keys, weights, has_tail = model_cells(model, est)
    counts = draw_histograms(weights, a["n_draws"], 8, seed=SEED, device=model.device)
    for r in range(8):
        twin = _replicate_model(model, keys, counts[r, :len(keys)], int(counts[r, len(keys)]) if has_tail else 0)
        try:
            ll_lock = twin.compute_loglikelihood(*a["estimates"][r])
            ll_seq = twin.compute_loglikelihood(*seq["estimates"][r])
        finally:
            twin.close()
        print("replicate %d  lock-step-gradient %s (LL %.10g, success %s)  sequential %s (LL %.10g, success %s)"
              % (r, a["estimates"][r].tolist(), ll_lock, a["success"][r], seq["estimates"][r].tolist(), ll_seq, seq["success"][r]))
        assert rel_err(ll_lock, ll_seq) <= 1e-6, (r, ll_lock, ll_seq)
        assert np.isfinite(a["loglikelihood"][r])
    differ = [r for r in range(8) if a["success"][r] != seq["success"][r]]
    for r in differ:
        print("replicate %d: lock-step-gradient success %s at %s, sequential success %s at %s"
              % (r, a["success"][r], a["estimates"][r].tolist(), seq["success"][r], seq["estimates"][r].tolist()))
    assert int(a["success"].sum()) == int(seq["success"].sum()), differ
    model.close()


def test_the_route_honours_fix(hip_lib):
    from covest_amd import constants, parametric_bootstrap
    model, est, _, _ = _basic_model()
    scale = constants.DEFAULT_ERR_SCALE  # (`fix` is in the optimiser's space, where the error rate is scaled)
    out = parametric_bootstrap(model, est, replicates=3, seed=SEED, fix=[None, est[1] * scale], refit="lockstep-gradient",
                               err_scale=scale)
    assert out["refit"] == "lockstep-gradient"
    assert out["estimates"][:, 1].tolist() == pytest.approx([est[1]] * 3, rel=1e-14) and out["mean"]["error_rate"] is None
    assert len(set(out["estimates"][:, 1].tolist())) == 1  # the fixed parameter is equal in every replicate
    assert len(set(out["estimates"][:, 0].tolist())) == 3  # the free parameter moved, each replicate its own way
    assert np.isfinite(out["estimates"]).all() and out["mean"]["coverage"] is not None
    model.close()


def test_repeats_model_is_reproducible(hip_lib):
    """H10k_rep_trim.hist at its golden optimum, 4 replicates: finite, reproducible, the `refit` key set."""
    from covest_amd import RepeatsModel, parametric_bootstrap
    g = load_golden("c3_trim.json")
    cand = g["candidates"]
    at = np.unravel_index(cand["flat_index"][int(np.argmax(cand["ll"]))], [len(a) for a in g["axes"]])
    c, e, q1, q = (g["axes"][d][i] for d, i in enumerate(at))
    point = [c, e, q1, g["q2"], q]
    model = RepeatsModel(g["k"], g["r"], load_hist(g["hist"]), g["tail"], max_error=g["max_error"])
    a, b = (parametric_bootstrap(model, point, replicates=4, seed=SEED, refit="lockstep-gradient") for _ in range(2))
    assert a["estimates"].shape == (4, 5) and a["at_bound"].shape == (4, 5) and a["success"].shape == (4,)
    assert a["estimates"].tobytes() == b["estimates"].tobytes() and a["success"].tolist() == b["success"].tolist()
    assert a["loglikelihood"].tobytes() == b["loglikelihood"].tobytes()
    assert np.isfinite(a["estimates"]).all() and np.isfinite(a["loglikelihood"]).all()
    assert a["n_draws"] == sum(model.hist.values()) + g["tail"] and a["refit"] == "lockstep-gradient"
    model.close()
