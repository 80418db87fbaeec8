"""The analytic gradient on the GPU (covest_eval_points_grad, ll_deriv.hip) against the 50-digit restatement of
tests/golden/gradient.json, against K-direct's value, for independence of what else is in the call, for the clamp and
NaN conventions -- and the refinement driven by it, end to end."""
import math
import random

import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err
from parity_helpers import TOL, _grad_bound, _model, _tail_delta

pytestmark = pytest.mark.gpu


def test_every_fixture_point(hip_lib):
    """ll to 1e-9 and per component |g_k - G_k| <= 1e-9 C_k + |tail| D_k delta / (1 - sp)^2: the suite's plain tolerance
    applied to the gradient's own condition sum, plus the first-order propagation of the sp_j slack the parity suite
    grants (delta = 8 eps n_keys).  No point of the fixture is left out."""
    g = load_golden("gradient.json")
    n, worst_ll, worst_g = 0, 0.0, 0.0
    for case in g["cases"]:
        m = _model(case)
        ll, grad = m.loglikelihood_gradient_points(case["points"])
        delta = _tail_delta(case["n_keys"])
        for i, point in enumerate(case["points"]):
            n += 1
            e = rel_err(float(ll[i]), case["ll"][i])
            print("%s %r: ll rel %.3g" % (case["source"], point, e))
            worst_ll = max(worst_ll, e)
            assert e <= TOL, (case["source"], point, float(ll[i]), case["ll"][i])
            sp, tail = case["sp"][i], case["tail"]
            for d, want in enumerate(case["grad"][i]):
                C, D = case["C"][i][d], case["D"][i][d]
                bound = _grad_bound(tail, sp, C, D, delta)
                diff = abs(float(grad[i, d]) - want)
                print("    d%d: got %.17g want %.17g |diff| %.3g bound %.3g (C %.3g)" % (d, grad[i, d], want, diff, bound, C))
                if C > 0:
                    worst_g = max(worst_g, diff / C)
                assert diff <= bound, (case["source"], point, d, float(grad[i, d]), want, diff, bound)
        m.close()
    assert n == g["kept"]
    print("%d points: worst ll rel %.3g, worst |dg| / C_k %.3g" % (n, worst_ll, worst_g))


def test_value_is_k_directs(hip_lib):
    """The value returned beside the gradient against loglikelihood_points(kernel="direct") at 1e-11."""
    g = load_golden("gradient.json")
    for case in g["cases"]:
        m = _model(case)
        ll, _ = m.loglikelihood_gradient_points(case["points"])
        want = m.loglikelihood_points(case["points"], kernel="direct")
        for a, b, p in zip(ll, want, case["points"]):
            assert rel_err(float(a), float(b)) <= 1e-11, (case["source"], p, float(a), float(b))
        m.close()


@pytest.mark.parametrize("kind,hist,tail", [("repeats", "H10k_rep_trim", 11192), ("basic", "H10k_basic_trim", 163),
                                            ("repeats", "sim_c10_e0.05", 0), ("repeats", "H10k_rep", 0)])
def test_a_point_does_not_depend_on_its_company(hip_lib, kind, hist, tail):
    """A batch of 1, 20 and 300 points holding the same point gives that point the same bits each time."""
    rng = np.random.default_rng(5)
    case = {"model": kind, "hist": hist, "k": 21, "r": 100, "tail": tail, "max_error": 8}
    m = _model(case)
    if kind == "repeats":
        c0 = 24.0 if hist.startswith("H10k") else 10.0
        point = [c0, 0.02, 0.6, 0.5, 0.2]
        others = np.column_stack([rng.uniform(0.5 * c0, 1.5 * c0, 300), rng.uniform(0.005, 0.1, 300), rng.uniform(0.3, 1, 300),
                                  rng.uniform(0, 1, 300), rng.uniform(0.15, 1, 300)])
    else:
        point = [4000.0, 0.02]
        others = np.column_stack([rng.uniform(3000, 5000, 300), rng.uniform(0.005, 0.05, 300)])
    alone_ll, alone_g = m.loglikelihood_gradient_points([point])
    assert math.isfinite(alone_ll[0]) and np.all(np.isfinite(alone_g))
    for n, at in ((20, 7), (300, 0), (300, 299), (300, 150)):
        batch = others[:n].copy()
        batch[at] = point
        ll, grad = m.loglikelihood_gradient_points(batch)
        assert ll[at].tobytes() == alone_ll[0].tobytes() and grad[at].tobytes() == alone_g[0].tobytes(), (n, at)
    again_ll, again_g = m.loglikelihood_gradient_points([point])
    assert again_ll.tobytes() == alone_ll.tobytes() and again_g.tobytes() == alone_g.tobytes()
    m.close()


def test_clamp_and_nan_conventions(hip_lib):
    from covest_amd import BasicModel, RepeatsModel
    hist = load_hist("sim_c10_e0.05")
    m = RepeatsModel(21, 100, hist, 0, max_error=8)
    inside = [10.0, 0.05, 0.6, 0.5, 0.3]
    on_ll, on_g = m.loglikelihood_gradient_points([[10.0, 0.5, 1.0, 0.5, 1.0]])  # ON the bounds: nothing moved
    out_ll, out_g = m.loglikelihood_gradient_points([[10.0, 0.7, 1.2, 0.5, 1.5], [10.0, -0.1, 0.1, -0.2, 0.3], inside])  # (q2 = 0: threshold_o = 2)
    assert out_ll[0] == on_ll[0]
    assert out_g[0, 1] == 0.0 and out_g[0, 2] == 0.0 and out_g[0, 4] == 0.0
    assert out_g[0, 0] == on_g[0, 0] and out_g[0, 3] == on_g[0, 3] and on_g[0, 1] != 0.0 and on_g[0, 2] != 0.0
    assert out_g[1, 1] == 0.0 and out_g[1, 2] == 0.0 and out_g[1, 3] == 0.0 and out_g[1, 0] != 0.0
    assert np.all(np.isfinite(out_g[1]))
    assert np.all(np.isfinite(out_g[2])) and np.all(out_g[2] != 0.0)
    ll1, g1 = m.compute_loglikelihood_gradient(*inside)
    assert ll1 == out_ll[2] and g1 == list(out_g[2])
    m.close()
    # LL = -inf (a counted key the model gives probability 0): every component NaN
    b = BasicModel(21, 100, {1: 10, 5000: 3}, 0, max_error=8)
    ll, grad = b.loglikelihood_gradient_points([[1.0, 0.01], [10.0, 0.05]])
    assert ll[0] == -math.inf and np.all(np.isnan(grad[0]))
    assert ll[0] == b.loglikelihood_points([[1.0, 0.01]], kernel="direct")[0]
    b.close()
    empty_ll, empty_g = m.__class__(21, 100, hist, 0, max_error=8).loglikelihood_gradient_points(np.empty((0, 5)))
    assert empty_ll.shape == (0,) and empty_g.shape == (0, 5)


def _first_guess(kind):
    """The steps of tests/flow_helper.py up to the estimator, restated."""
    from covest_amd import constants
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, constants.DEFAULT_K, constants.DEFAULT_READ_LENGTH)
    m = select_model(kind)(constants.DEFAULT_K, constants.DEFAULT_READ_LENGTH, hist, tail, max_error=constants.MAX_ERRORS,
                           max_cov=None, min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
    guess = list(m.defaults)
    if not (guess_c == 0 and guess_e == 1):
        guess[:2] = guess_c, guess_e
    return m, guess


@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_refinement_end_to_end(hip_lib, kind):
    """gradient="analytic" from the first guess process_histogram gives: success, and an end value no worse than the
    finite-difference flow's by more than scipy's own stopping tolerance 2.22e-9 max(|f|, 1) (factr * eps of the
    L-BFGS-B defaults).  The projected analytic gradient at the end point is printed."""
    from covest_amd import constants
    from covest_amd.estimator import CoverageEstimator
    m, guess = _first_guess(kind)
    x0 = list(guess)
    x0[1] *= constants.DEFAULT_ERR_SCALE
    fd = CoverageEstimator(m, err_scale=constants.DEFAULT_ERR_SCALE)._optimize(x0)
    est = CoverageEstimator(m, err_scale=constants.DEFAULT_ERR_SCALE, gradient="analytic")
    an = est._optimize(x0)
    row = est.negll_gradient_points([an.x])[0]
    lo = np.array([-np.inf if b[0] is None else b[0] for b in est.bounds])
    hi = np.array([np.inf if b[1] is None else b[1] for b in est.bounds])
    proj = np.where(((an.x <= lo) & (row[1:] > 0)) | ((an.x >= hi) & (row[1:] < 0)), 0.0, row[1:])
    print("%s: fd  end %r f %.10f nit %d nfev %d" % (kind, list(fd.x), fd.fun, fd.nit, fd.nfev))
    print("%s: an  end %r f %.10f nit %d nfev %d" % (kind, list(an.x), an.fun, an.nit, an.nfev))
    print("%s: projected analytic gradient at the analytic end point %r" % (kind, list(proj)))
    assert an.success
    assert an.fun <= fd.fun + 2.22e-9 * max(abs(fd.fun), 1.0), (an.fun, fd.fun)
    res, ok = CoverageEstimator(m, err_scale=constants.DEFAULT_ERR_SCALE, gradient="analytic").compute_coverage(guess)
    assert ok and list(res) == [v / constants.DEFAULT_ERR_SCALE if i == 1 else v for i, v in enumerate(an.x)]
    m.close()


def test_lock_step_equals_sequential_bit_for_bit(hip_lib):
    from covest_amd import RepeatsModel
    from covest_amd.estimator import CoverageEstimator, _LockStep
    from covest_amd.grid import initial_grid
    m = RepeatsModel(21, 100, load_hist("sim_c10_e0.05"), 0, max_error=8)
    est = CoverageEstimator(m, gradient="analytic")
    random.seed(3)
    starts = initial_grid([9.0, 0.05, 0.8, 0.5, 0.5], count=6, bounds=est.bounds)
    seq = [est._optimize(s) for s in starts]
    lock = _LockStep(est.negll_gradient_points, len(starts))
    par = lock.map(est._optimize, starts)
    for a, b in zip(seq, par):
        assert np.array_equal(a.x, b.x) and a.fun == b.fun and a.nit == b.nit and a.nfev == b.nfev
    assert lock.rounds == max(r.nfev for r in par)
    best_seq = CoverageEstimator(m, gradient="analytic")._best_of(starts)
    best_lock = CoverageEstimator(m, gradient="analytic", lock_step=True)._best_of(starts)
    assert np.array_equal(best_seq.x, best_lock.x) and best_seq.fun == best_lock.fun
    m.close()
