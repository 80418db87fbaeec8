"""The outer product of the scores on the GPU (covest_eval_points_opg, ll_deriv.hip's third mode) against the 50-digit
restatement of tests/golden/opg.json, against K-grad's value and gradient bit for bit, for symmetry, for independence of
what else is in the call, for the clamp and NaN conventions and the in-place boundary -- and the sandwich covariance
built on it, end to end."""
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err
from parity_helpers import K_TAIL, TOL, _grad_bound, _model, _opg_bound, _tail_delta

pytestmark = pytest.mark.gpu


def test_every_fixture_point(hip_lib):
    """ll to 1e-9; per gradient component gradient.json's own bound 1e-9 C_k + |tail| D_k delta / (1 - sp)^2; per entry
    |B_kl - want| <= 1e-9 C_kl + s_kl with the fixture's C_kl = sum |h r_k r_l| + |tail S_k S_l / (1 - sp)^2| and
    s_kl = |tail| 2 |S_k| |S_l| delta / (1 - sp)^3: the suite's plain tolerance applied to the entry's own condition sum,
    plus the first-order propagation of the sp slack the parity suite grants (delta = 8 eps n_keys), the Hessian's form.
    No point of the fixture is left out."""
    g = load_golden("opg.json")
    assert K_TAIL == g["k_tail"]
    n, worst_ll, worst_g, worst_b = 0, 0.0, 0.0, 0.0
    for case in g["cases"]:
        m = _model(case)
        P = m.param_count
        ll, grad, opg = m.loglikelihood_score_outer_points(case["points"])
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
                bound = _grad_bound(tail, sp, case["Cg"][i][d], case["D"][i][d], delta)
                diff = abs(float(grad[i, d]) - want)
                if case["Cg"][i][d] > 0:
                    worst_g = max(worst_g, diff / case["Cg"][i][d])
                assert diff <= bound, (case["source"], point, d, float(grad[i, d]), want, diff, bound)
            for k in range(P):
                for l in range(P):
                    want, C, s_kl = case["opg"][i][k][l], case["C"][i][k][l], case["s"][i][k][l]
                    bound = _opg_bound(C, s_kl)
                    diff = abs(float(opg[i, k, l]) - want)
                    if l >= k:
                        print("    B%d%d: got %.17g want %.17g |diff| %.3g bound %.3g (C %.3g)" % (k, l, opg[i, k, l], want, diff, bound, C))
                    if C > 0:
                        worst_b = max(worst_b, diff / C)
                    assert diff <= bound, (case["source"], point, k, l, float(opg[i, k, l]), want, diff, bound)
        m.close()
    assert n == g["kept"]
    print("%d points: worst ll rel %.3g, worst |dg| / C_k %.3g, worst |dB| / C_kl %.3g" % (n, worst_ll, worst_g, worst_b))


def test_value_and_gradient_are_k_grads_bits(hip_lib):
    """The mode is order 1's walk, unchanged: ll and grad are covest_eval_points_grad's, bit for bit, on every fixture point."""
    g = load_golden("opg.json")
    for case in g["cases"]:
        m = _model(case)
        ll, grad, _ = m.loglikelihood_score_outer_points(case["points"])
        want_ll, want_g = m.loglikelihood_gradient_points(case["points"])
        assert ll.tobytes() == want_ll.tobytes(), case["source"]
        assert grad.tobytes() == want_g.tobytes(), case["source"]
        m.close()


def _setup(kind, hist, tail):
    rng = np.random.default_rng(5)
    m = _model({"model": kind, "hist": hist, "k": 21, "r": 100, "tail": tail, "max_error": 8})
    if kind == "repeats":
        c0 = 24.0 if hist.startswith("H10k") else 10.0
        point = [c0, 0.02, 0.6, 0.5, 0.2]
        others = np.column_stack([rng.uniform(0.5 * c0, 1.5 * c0, 300), rng.uniform(0.005, 0.1, 300), rng.uniform(0.3, 1, 300),
                                  rng.uniform(0, 1, 300), rng.uniform(0.15, 1, 300)])
    else:
        point = [4000.0, 0.02]
        others = np.column_stack([rng.uniform(3000, 5000, 300), rng.uniform(0.005, 0.05, 300)])
    return m, point, others


SETUPS = [("repeats", "H10k_rep_trim", 11192), ("basic", "H10k_basic_trim", 163), ("repeats", "sim_c10_e0.05", 0),
          ("repeats", "H10k_rep", 0)]


@pytest.mark.parametrize("kind,hist,tail", SETUPS)
def test_symmetric_and_independent_of_company(hip_lib, kind, hist, tail):
    """B[k][l] and B[l][k] are the same bits; a batch of 1, 20 and 300 points holding the same point gives that point the
    same bits each time (300 is past the in-place limit: the other copy route), and so does a repeated call."""
    m, point, others = _setup(kind, hist, tail)
    alone = m.loglikelihood_score_outer_points([point])
    assert math.isfinite(alone[0][0]) and np.all(np.isfinite(alone[1])) and np.all(np.isfinite(alone[2]))
    assert alone[2][0].tobytes() == np.ascontiguousarray(alone[2][0].T).tobytes()
    assert np.all(alone[2][0][:2, :2] != 0.0) and alone[2][0][0, 0] > 0.0 and alone[2][0][1, 1] > 0.0
    for n, at in ((20, 7), (300, 0), (300, 299), (300, 150)):
        batch = others[:n].copy()
        batch[at] = point
        ll, grad, opg = m.loglikelihood_score_outer_points(batch)
        assert ll[at].tobytes() == alone[0][0].tobytes() and grad[at].tobytes() == alone[1][0].tobytes(), (n, at)
        assert opg[at].tobytes() == alone[2][0].tobytes(), (n, at)
        for i in range(n):
            assert opg[i].tobytes() == np.ascontiguousarray(opg[i].T).tobytes(), (n, i)
    again = m.loglikelihood_score_outer_points([point])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, alone))
    m.close()


@pytest.mark.parametrize("kind,hist,tail", SETUPS[:2])
def test_in_place_boundary(hip_lib, kind, hist, tail):
    """256 points are read and written in place in page-locked host memory, 257 go through the staged copies: the first
    256 points' numbers are the same bits either way."""
    m, point, others = _setup(kind, hist, tail)
    rng = np.random.default_rng(11)
    pts = others[rng.integers(0, 300, 257)]
    pts[255], pts[256] = point, point
    inside = m.loglikelihood_score_outer_points(pts[:256])
    beyond = m.loglikelihood_score_outer_points(pts)
    for a, b in zip(inside, beyond):
        assert a.shape[0] == 256 and b.shape[0] == 257
        assert a.tobytes() == np.ascontiguousarray(b[:256]).tobytes()
        assert b[255].tobytes() == b[256].tobytes()
    m.close()


def test_clamp_and_nan_conventions(hip_lib):
    from covest_amd import BasicModel, RepeatsModel
    hist = load_hist("sim_c10_e0.05")
    m = RepeatsModel(21, 100, hist, 0, max_error=8)
    inside = [10.0, 0.05, 0.6, 0.5, 0.3]
    on = m.loglikelihood_score_outer_points([[10.0, 0.5, 0.9, 0.5, 1.0]])  # ON the bounds of e and q: nothing moved
    out = m.loglikelihood_score_outer_points([[10.0, 0.7, 0.9, 0.5, 1.5], inside])
    assert out[0][0] == on[0][0]
    B_out, B_on = out[2][0], on[2][0]
    for d in (1, 4):  # moved: zero row and column, zero gradient component
        assert not B_out[d].any() and not B_out[:, d].any() and out[1][0, d] == 0.0
        assert B_on[d].any()
    rest = [0, 2, 3]
    assert np.array_equal(B_out[np.ix_(rest, rest)], B_on[np.ix_(rest, rest)])  # the rest: the on-bound point's, bit for bit
    assert np.array_equal(out[1][0, rest], on[1][0, rest])
    assert np.all(np.isfinite(out[2][1])) and np.all(out[2][1] != 0.0)
    ll1, g1, b1 = m.compute_loglikelihood_score_outer(*inside)
    assert ll1 == out[0][1] and g1 == list(out[1][1]) and b1 == out[2][1].tolist()
    # LL = -inf (a counted key the model gives probability 0): every entry NaN
    b = BasicModel(21, 100, {1: 10, 5000: 3}, 0, max_error=8)
    ll, grad, opg = b.loglikelihood_score_outer_points([[1.0, 0.01], [10.0, 0.05]])
    assert ll[0] == -math.inf and np.all(np.isnan(grad[0])) and np.all(np.isnan(opg[0]))
    assert ll[0] == b.loglikelihood_points([[1.0, 0.01]], kernel="direct")[0]
    b.close()
    empty = m.loglikelihood_score_outer_points(np.empty((0, 5)))
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
def test_sandwich_end_to_end(hip_lib, kind):
    """At the recorded optimum of sim_c10_e0.05 (tests/golden/own_optimum.json): the sandwich is formed over the (c, e)
    block the observed information inverts, the robust covariance is symmetric and positive on its diagonal, the dict is
    observed_information's extended, the record gains the three robust keys.
    PRINTED, NOT ASSERTED (DESIGN.md 6j records them; nobody had measured them): B, information_ratio, se_ratio and the
    robust Wald 95 % interval of the coverage beside the model's of 6f."""
    from covest_amd.information import genome_size_se, observed_information, sandwich_covariance, wald_intervals
    from covest_amd.report import print_output
    opt = load_golden("own_optimum.json")["models"][kind]
    m, hist_orig, sample_factor = _flow_model(kind)
    est = [opt[name] for name in m.params]
    info = observed_information(m, est)
    out = sandwich_covariance(m, est, info=info)
    print("%s: estimate %r, n = sum h + tail = %r" % (kind, est, sum(m.hist.values()) + m.tail))
    print("%s: A = -LL Hessian\n%s" % (kind, np.array2string(np.array(out['hessian']), precision=10)))
    print("%s: B (uncentred)\n%s" % (kind, np.array2string(np.array(out['opg']), precision=10)))
    print("%s: gradient %r" % (kind, out['gradient']))
    print("%s: free %r, reason %r" % (kind, out['free'], out['reason']))
    print("%s: information_ratio (eigenvalues of A^-1 B_c) %r" % (kind, out['information_ratio']))
    print("%s: standard errors %r" % (kind, out['standard_errors']))
    print("%s: robust standard errors %r" % (kind, out['robust_standard_errors']))
    print("%s: se_ratio %r" % (kind, out['se_ratio']))
    assert out['reason'] is None and out['free'] == [0, 1]
    for key, value in info.items():
        assert out[key] == value, key
    B = np.array(out['opg'])
    assert np.array_equal(B, B.T) and B[0, 0] > 0 and B[1, 1] > 0
    _, g_g = m.loglikelihood_gradient_points([est])
    _, g_o, _ = m.loglikelihood_score_outer_points([est])
    assert g_o.tobytes() == g_g.tobytes()
    V = np.array(out['robust_covariance'])
    assert V.shape == (2, 2) and np.all(np.isfinite(V)) and V[0, 0] > 0 and V[1, 1] > 0
    assert abs(V[0, 1] - V[1, 0]) <= 1e-12 * math.sqrt(V[0, 0] * V[1, 1])
    assert len(out['information_ratio']) == 2 and all(math.isfinite(v) for v in out['information_ratio'])
    rse = out['robust_standard_errors']
    assert rse['coverage'] > 0 and rse['error_rate'] > 0
    assert out['se_ratio']['coverage'] == rse['coverage'] / out['standard_errors']['coverage']
    if kind == "repeats":
        assert est[2] == 1.0 and rse['q1'] is None and rse['q2'] is None and rse['q'] is None
        assert not B[3].any() and not B[4].any()
    model_iv, robust_iv = wald_intervals(out)['coverage'], wald_intervals(out, robust=True)['coverage']
    assert robust_iv[0] < est[0] < robust_iv[1]
    print("%s: Wald 95 %% interval of the coverage: model [%.6f, %.6f] (half-width %.6g), robust [%.6f, %.6f] (half-width %.6g)" % (
        kind, model_iv[0], model_iv[1], (model_iv[1] - model_iv[0]) / 2, robust_iv[0], robust_iv[1], (robust_iv[1] - robust_iv[0]) / 2))
    size, rsize = (genome_size_se(m, hist_orig, out, sample_factor=sample_factor, robust=r) for r in (False, True))
    print("%s: genome size %.1f, se %.1f, robust se %.1f" % (kind, size['genome_size'], size['genome_size_se'], rsize['genome_size_se']))
    rec = print_output(hist_orig, m, True, sample_factor, estimated=est, silent=True, information=out)
    plain = print_output(hist_orig, m, True, sample_factor, estimated=est, silent=True, information=info)
    assert set(rec) - set(plain) == {'robust_standard_errors', 'robust_wald_intervals', 'genome_size_robust_se'}
    assert rec['robust_standard_errors']['coverage'] == rse['coverage'] * sample_factor
    assert rec['genome_size_robust_se'] == rsize['genome_size_se']
    m.close()
