"""The closed-form Hessian on the GPU (covest_eval_points_hess, ll_deriv.hip) against the 50-digit restatement of
tests/golden/hessian.json, against K-direct's value and K-grad's gradient, for symmetry, for independence of what else is
in the call, for the clamp and NaN conventions -- and the observed information built on it, end to end."""
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err
from parity_helpers import TOL, _grad_bound, _hess_bound, _model, _tail_delta

pytestmark = pytest.mark.gpu


def _grad_bound_of(case, i, d, delta):
    return _grad_bound(case["tail"], case["sp"][i], case["Cg"][i][d], case["D"][i][d], delta)


def test_every_fixture_point(hip_lib):
    """ll to 1e-9; per gradient component gradient.json's own bound 1e-9 C_k + |tail| D_k delta / (1 - sp)^2; per Hessian
    entry |H_kl - want| <= 1e-9 C_kl + s_kl with s_kl = |tail| (D_kl delta / (1 - sp)^2 + 2 D_k D_l delta / (1 - sp)^3):
    the suite's plain tolerance applied to the entry's own condition sum, plus the first-order propagation of the sp_j
    slack the parity suite grants (delta = 8 eps n_keys).  No point of the fixture is left out."""
    g = load_golden("hessian.json")
    n, worst_ll, worst_g, worst_h = 0, 0.0, 0.0, 0.0
    for case in g["cases"]:
        m = _model(case)
        P = m.param_count
        ll, grad, hess = m.loglikelihood_hessian_points(case["points"])
        delta = _tail_delta(case["n_keys"])
        tail = case["tail"]
        for i, point in enumerate(case["points"]):
            n += 1
            e = rel_err(float(ll[i]), case["ll"][i])
            print("%s %r: ll rel %.3g" % (case["source"], point, e))
            worst_ll = max(worst_ll, e)
            assert e <= TOL, (case["source"], point, float(ll[i]), case["ll"][i])
            sp = case["sp"][i]
            for d, want in enumerate(case["grad"][i]):
                bound = _grad_bound_of(case, i, d, delta)
                diff = abs(float(grad[i, d]) - want)
                if case["Cg"][i][d] > 0:
                    worst_g = max(worst_g, diff / case["Cg"][i][d])
                assert diff <= bound, (case["source"], point, d, float(grad[i, d]), want, diff, bound)
            for k in range(P):
                for l in range(P):
                    want, C = case["hess"][i][k][l], case["C"][i][k][l]
                    bound = _hess_bound(tail, sp, C, case["D2"][i][k][l], case["D"][i][k], case["D"][i][l], delta)
                    diff = abs(float(hess[i, k, l]) - want)
                    if l >= k:
                        print("    H%d%d: got %.17g want %.17g |diff| %.3g bound %.3g (C %.3g)" % (k, l, hess[i, k, l], want, diff, bound, C))
                    if C > 0:
                        worst_h = max(worst_h, diff / C)
                    assert diff <= bound, (case["source"], point, k, l, float(hess[i, k, l]), want, diff, bound)
        m.close()
    assert n == g["kept"]
    print("%d points: worst ll rel %.3g, worst |dg| / C_k %.3g, worst |dH| / C_kl %.3g" % (n, worst_ll, worst_g, worst_h))


def test_value_is_k_directs_and_gradient_is_k_grads(hip_lib):
    """The value against loglikelihood_points(kernel="direct") at 1e-11 (as the gradient's test), the gradient against
    loglikelihood_gradient_points within twice the gradient's bound (each may use all of it)."""
    g = load_golden("hessian.json")
    for case in g["cases"]:
        m = _model(case)
        ll, grad, _ = m.loglikelihood_hessian_points(case["points"])
        want = m.loglikelihood_points(case["points"], kernel="direct")
        _, want_g = m.loglikelihood_gradient_points(case["points"])
        delta = _tail_delta(case["n_keys"])
        for i, p in enumerate(case["points"]):
            assert rel_err(float(ll[i]), float(want[i])) <= 1e-11, (case["source"], p, float(ll[i]), float(want[i]))
            for d in range(m.param_count):
                assert abs(float(grad[i, d]) - float(want_g[i, d])) <= 2 * _grad_bound_of(case, i, d, delta), (case["source"], p, d)
        m.close()


@pytest.mark.parametrize("kind,hist,tail", [("repeats", "H10k_rep_trim", 11192), ("basic", "H10k_basic_trim", 163),
                                            ("repeats", "sim_c10_e0.05", 0), ("repeats", "H10k_rep", 0)])
def test_symmetric_and_independent_of_company(hip_lib, kind, hist, tail):
    """H[k][l] and H[l][k] are the same bits; a batch of 1, 20 and 300 points holding the same point gives that point the
    same bits each time (300 is past the in-place limit: the other copy route), and so does a repeated call."""
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
    alone = m.loglikelihood_hessian_points([point])
    assert math.isfinite(alone[0][0]) and np.all(np.isfinite(alone[1])) and np.all(np.isfinite(alone[2]))
    assert alone[2][0].tobytes() == np.ascontiguousarray(alone[2][0].T).tobytes()
    assert np.all(alone[2][0][:2, :2] != 0.0)
    for n, at in ((20, 7), (300, 0), (300, 299), (300, 150)):
        batch = others[:n].copy()
        batch[at] = point
        ll, grad, hess = m.loglikelihood_hessian_points(batch)
        assert ll[at].tobytes() == alone[0][0].tobytes() and grad[at].tobytes() == alone[1][0].tobytes(), (n, at)
        assert hess[at].tobytes() == alone[2][0].tobytes(), (n, at)
        for i in range(n):
            assert hess[i].tobytes() == np.ascontiguousarray(hess[i].T).tobytes(), (n, i)
    again = m.loglikelihood_hessian_points([point])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, alone))
    m.close()


def test_clamp_and_nan_conventions(hip_lib):
    from covest_amd import BasicModel, RepeatsModel
    hist = load_hist("sim_c10_e0.05")
    m = RepeatsModel(21, 100, hist, 0, max_error=8)
    inside = [10.0, 0.05, 0.6, 0.5, 0.3]
    on = m.loglikelihood_hessian_points([[10.0, 0.5, 0.9, 0.5, 1.0]])  # ON the bounds of e and q: nothing moved
    out = m.loglikelihood_hessian_points([[10.0, 0.7, 0.9, 0.5, 1.5], inside])
    assert out[0][0] == on[0][0]
    H_out, H_on = out[2][0], on[2][0]
    for d in (1, 4):  # moved: zero row and column, zero gradient component
        assert not H_out[d].any() and not H_out[:, d].any() and out[1][0, d] == 0.0
        assert H_on[d].any()
    rest = [0, 2, 3]
    assert np.array_equal(H_out[np.ix_(rest, rest)], H_on[np.ix_(rest, rest)])  # the rest: the on-bound point's, bit for bit
    assert np.array_equal(out[1][0, rest], on[1][0, rest])
    assert np.all(np.isfinite(out[2][1])) and np.all(out[2][1] != 0.0)
    ll1, g1, h1 = m.compute_loglikelihood_hessian(*inside)
    assert ll1 == out[0][1] and g1 == list(out[1][1]) and h1 == out[2][1].tolist()
    ll_g, g_g = m.loglikelihood_gradient_points([inside])
    assert rel_err(ll1, float(ll_g[0])) <= 1e-11
    # LL = -inf (a counted key the model gives probability 0): every entry NaN
    b = BasicModel(21, 100, {1: 10, 5000: 3}, 0, max_error=8)
    ll, grad, hess = b.loglikelihood_hessian_points([[1.0, 0.01], [10.0, 0.05]])
    assert ll[0] == -math.inf and np.all(np.isnan(grad[0])) and np.all(np.isnan(hess[0]))
    assert ll[0] == b.loglikelihood_points([[1.0, 0.01]], kernel="direct")[0]
    b.close()
    empty = m.loglikelihood_hessian_points(np.empty((0, 5)))
    assert empty[0].shape == (0,) and empty[1].shape == (0, 5) and empty[2].shape == (0, 5, 5)
    m.close()


def _flow_model(kind):
    """The steps of tests/flow_helper.py up to the estimator, restated."""
    from covest_amd import constants
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sample_factor, _, _ = process_histogram(hist_orig, constants.DEFAULT_K, constants.DEFAULT_READ_LENGTH)
    m = select_model(kind)(constants.DEFAULT_K, constants.DEFAULT_READ_LENGTH, hist, tail, max_error=constants.MAX_ERRORS,
                           max_cov=None, min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
    return m, hist_orig, sample_factor


@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_observed_information_end_to_end(hip_lib, kind):
    """At the recorded optimum of sim_c10_e0.05 (tests/golden/own_optimum.json).  basic: two free parameters, positive
    definite, finite standard errors, the Wald interval of the coverage contains the estimate and genome_size +- z se_G
    the recorded genome size.  repeats: q1 = 1 sits on its bound and (1 - q1) annihilates q2's and q's rows -- the three
    are reported None and the (c, e) block is inverted.
    PRINTED, NOT ASSERTED (DESIGN.md 6f records them): the Wald 95 % half-width of the coverage beside the profile
    interval's +-0.018 of 6d, and the Hessian by central differences of loglikelihood_gradient_points, h = 1e-4 |theta|,
    beside the closed form, entry by entry."""
    from covest_amd.information import genome_size_se, observed_information, wald_intervals
    from covest_amd.report import print_output
    opt = load_golden("own_optimum.json")["models"][kind]
    m, hist_orig, sample_factor = _flow_model(kind)
    est = [opt[name] for name in m.params]
    info = observed_information(m, est)
    names = list(m.params)
    print("%s: estimate %r" % (kind, est))
    print("%s: -LL Hessian\n%s" % (kind, np.array2string(np.array(info['hessian']), precision=10)))
    print("%s: free %r, standard errors %r, reason %r" % (kind, info['free'], info['standard_errors'], info['reason']))
    assert info['reason'] is None and info['free'] == [0, 1]
    se = info['standard_errors']
    assert math.isfinite(se['coverage']) and se['coverage'] > 0 and math.isfinite(se['error_rate']) and se['error_rate'] > 0
    cov = np.array(info['covariance'])
    H = np.array(info['hessian'])
    assert np.max(np.abs(cov @ H[:2, :2] - np.eye(2))) <= 1e-9
    assert abs(info['correlation'][0][1]) < 1
    if kind == "repeats":
        assert est[2] == 1.0 and se['q1'] is None and se['q2'] is None and se['q'] is None
        assert not H[3].any() and not H[4].any()
    walds = wald_intervals(info)
    lo, hi = walds['coverage']
    assert lo < est[0] < hi
    size = genome_size_se(m, hist_orig, info, sample_factor=sample_factor)
    glo, ghi = size['genome_size_wald_interval']
    print("%s: genome size %.1f se %.1f Wald [%.1f, %.1f], recorded %d" % (kind, size['genome_size'], size['genome_size_se'],
                                                                          glo, ghi, opt['genome_size']))
    assert glo <= opt['genome_size'] <= ghi
    rec = print_output(hist_orig, m, True, sample_factor, estimated=est, silent=True, information=info)
    assert rec['standard_errors']['coverage'] == se['coverage'] * sample_factor and rec['wald_level'] == 0.95
    assert rec['genome_size_wald_interval'][0] <= rec['genome_size'] <= rec['genome_size_wald_interval'][1]
    print("%s: Wald 95 %% half-width of the coverage %.6g (profile interval of DESIGN 6d: +-0.018); of the error rate %.6g; "
          "correlation(c, e) %.6f" % (kind, (hi - lo) / 2, (walds['error_rate'][1] - walds['error_rate'][0]) / 2,
                                      info['correlation'][0][1]))
    # the route the closed form replaces: central differences of the analytic gradient (not asserted)
    P = m.param_count
    inside = [d for d in range(P) if (m.bounds[d][0] is None or est[d] > m.bounds[d][0])
              and (m.bounds[d][1] is None or est[d] < m.bounds[d][1])]
    pts = []
    for d in inside:
        h = 1e-4 * abs(est[d])
        up, down = list(est), list(est)
        up[d] += h
        down[d] -= h
        pts += [up, down]
    _, g = m.loglikelihood_gradient_points(pts)
    for at, d in enumerate(inside):
        h = 1e-4 * abs(est[d])
        column = -(g[2 * at] - g[2 * at + 1]) / (2 * h)
        for k in range(P):
            closed = H[k, d]
            print("%s: -d2LL/d%s d%s closed form %.12g, differenced gradient %.12g, difference %.3g (%.3g of the entry)" % (
                kind, names[k], names[d], closed, column[k], column[k] - closed,
                abs(column[k] - closed) / abs(closed) if closed != 0 else float('nan')))
    m.close()
