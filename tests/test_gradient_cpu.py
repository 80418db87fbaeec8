"""The analytic gradient without a GPU: the entry point is declared and bound, the committed fixture
(tests/golden/gradient.json) is consistent with the formulas it states, and CoverageEstimator(gradient="analytic")
maps the model's gradient into optimiser space -- on a stand-in model whose likelihood is an ordinary Python function,
in the manner of tests/test_refinement_cpu.py."""
import math
import os
import random
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from covest_amd.estimator import CoverageEstimator, _LockStep
from covest_amd.grid import initial_grid


def test_entry_point_declared_and_bound(hip_lib):
    from covest_amd import _capi
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+covest_eval_points_grad\s*\(\s*covest_model\s*\*\s*m\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*"
                     r"\s*params\s*,\s*double\s*\*\s*out_ll\s*,\s*double\s*\*\s*out_grad\s*\)", text)
    assert "covest_eval_points_grad" in _capi.EXPORTS
    assert hasattr(hip_lib, "covest_eval_points_grad")
    assert hip_lib.covest_abi_version() == 1
    from covest_amd import BasicModel, RepeatsModel
    for cls in (BasicModel, RepeatsModel):
        assert callable(cls.loglikelihood_gradient_points) and callable(cls.compute_loglikelihood_gradient)


def test_fixture_shape_and_selection_rule():
    """Every point of the fixture is finite, carries one gradient / C / D entry per parameter, and obeys the rule the
    generator selected by: 1e-9 C_k >= |tail| D_k delta / (1 - sp)^2, delta = 8 eps n_keys."""
    g = load_golden("gradient.json")
    n = 0
    for case in g["cases"]:
        P = 5 if case["model"] == "repeats" else 2
        delta = g["k_tail"] * 2.0 ** -52 * case["n_keys"]
        for i, point in enumerate(case["points"]):
            n += 1
            assert len(point) == P and math.isfinite(case["ll"][i])
            assert len(case["grad"][i]) == len(case["C"][i]) == len(case["D"][i]) == P
            sp, tail = case["sp"][i], case["tail"]
            if tail and sp < 1:
                assert abs(1 - sp) >= 1e-6
                for d in range(P):
                    if case["grad"][i][d] != 0.0:
                        assert 1e-9 * case["C"][i][d] >= abs(tail) * case["D"][i][d] * delta / (1 - sp) ** 2
            for d in range(P):
                assert abs(case["grad"][i][d]) <= case["C"][i][d] * (1 + 1e-12)
    assert n == g["kept"] and 60 <= n <= 100


def test_fixture_consistent_with_a_recomputation():
    """The fixture's own consistency on a small case: value and gradient recomputed with the generator's restatement at
    30 digits, and the gradient against a central difference of the SMOOTH value (the generator's quantize=False: the
    recorded gradient uses the weights a_os as the kernels round them, which moves a weight by up to
    comb_s * 1.1e-16 / tot_o ~ 3e-8 -- hence 1e-7 of the condition sum there)."""
    mpmath = pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_gradient",
                                                  os.path.join(REPO, "tests", "golden", "make_golden_gradient.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    mp, mpf = mpmath.mp, mpmath.mpf
    g = load_golden("gradient.json")
    case = next(c for c in g["cases"] if c["source"] == "own: sim_c10_e0.05, repeats")
    keep = ("model", "hist", "k", "r", "tail", "max_error", "max_cov", "threshold", "min_single_copy_ratio")
    mspec = {k: case[k] for k in keep if k in case}
    old = mp.dps
    try:
        mp.dps = 30
        m, consts, counts, n_keys = gen.consts_of(mspec)
        for i in (0, 1, 3):
            point, T = case["points"][i], case["T"][i]
            theta = [mpf(float(v)) for v in m.fit_to_bounds(point)]
            ll, sp, grad, C, D = gen.finish(gen.grad_partial(consts, theta, 1, T), counts, case["tail"], 5)
            assert abs(float(ll) - case["ll"][i]) <= 1e-14 * abs(case["ll"][i])
            for d in range(5):
                assert abs(float(grad[d]) - case["grad"][i][d]) <= 1e-13 * case["C"][i][d]
                if float(theta[d]) != float(point[d]) or case["C"][i][d] == 0.0:
                    assert case["grad"][i][d] == 0.0
                    continue
                h = mpf(10) ** -12
                up, down = list(theta), list(theta)
                up[d], down[d] = theta[d] + h, theta[d] - h
                num = (gen.ll_only(mspec, up, T) - gen.ll_only(mspec, down, T)) / (2 * h)
                assert abs(float(num) - case["grad"][i][d]) <= 1e-7 * case["C"][i][d], (i, d)
    finally:
        mp.dps = old


# ---------------------------------------------------------------------------------------------- the estimator
class _StubModel:
    """Smooth, bounded, with the API the estimator touches -- and its gradient in closed form."""
    bounds = ((0.01, None), (0, 0.5), (0.3, 1), (0, 1), (0, 1))
    params = ('coverage', 'error_rate', 'q1', 'q2', 'q')

    def __init__(self):
        self.calls = 0
        self.grad_calls = 0
        self.points = 0

    def compute_loglikelihood(self, c, e, q1, q2, q):
        self.calls += 1
        self.points += 1
        return -(1e6 * ((math.log(c) - math.log(12.0)) ** 2 + 40 * (e - 0.03) ** 2 + (q1 - 0.9) ** 2
                        + 0.5 * (q2 - 0.4) ** 2 * (1 + c / 50) + (q - 0.2) ** 4) + 3.25e7)

    def loglikelihood_points(self, pts, kernel="auto"):
        self.calls += 1
        self.points += len(pts)
        calls, points = self.calls, self.points
        out = np.array([self.compute_loglikelihood(*p) for p in pts])
        self.calls, self.points = calls, points
        return out

    def loglikelihood_gradient_points(self, pts):
        self.grad_calls += 1
        pts = np.asarray(pts, dtype=np.float64)
        ll = self.loglikelihood_points(pts)
        self.calls -= 1
        c, e, q1, q2, q = pts.T
        grad = -1e6 * np.stack([2 * (np.log(c) - math.log(12.0)) / c + 0.5 * (q2 - 0.4) ** 2 / 50, 80 * (e - 0.03),
                                2 * (q1 - 0.9), (q2 - 0.4) * (1 + c / 50), 4 * (q - 0.2) ** 3], axis=1)
        return ll, grad


def _same(a, b):
    return np.array_equal(a.x, b.x) and a.fun == b.fun and a.nit == b.nit and a.success == b.success


def test_err_scale_chain_rule_and_fixed_parameters():
    model = _StubModel()
    x = [9.0, 0.4, 0.5, 0.5, 0.5]  # optimiser space: the error rate times err_scale
    plain = CoverageEstimator(model, err_scale=10, gradient="analytic").negll_gradient_points([x])
    ll, grad = model.loglikelihood_gradient_points([[9.0, 0.04, 0.5, 0.5, 0.5]])
    assert plain.shape == (1, 6) and plain[0, 0] == -ll[0]
    want = -grad[0]
    want[1] /= 10
    assert np.array_equal(plain[0, 1:], want)
    # against a central difference of the estimator's own objective, in optimiser space
    est = CoverageEstimator(model, err_scale=10, gradient="analytic")
    for d in range(5):
        h = 1e-6
        up, down = list(x), list(x)
        up[d] += h
        down[d] -= h
        num = (est.likelihood_f(up) - est.likelihood_f(down)) / (2 * h)
        assert abs(num - plain[0, 1 + d]) <= 1e-6 * max(1.0, abs(num)), d
    fix = [None, None, 0.7, None, 0.25]
    pinned = CoverageEstimator(model, err_scale=10, fix=fix, gradient="analytic").negll_gradient_points([x])
    ll, grad = model.loglikelihood_gradient_points([[9.0, 0.04, 0.7, 0.5, 0.25]])
    assert pinned[0, 0] == -ll[0] and pinned[0, 3] == 0.0 and pinned[0, 5] == 0.0
    assert pinned[0, 1] == -grad[0, 0] and pinned[0, 2] == -grad[0, 1] / 10 and pinned[0, 4] == -grad[0, 3]


def test_analytic_refinement_one_evaluation_a_gradient():
    for start in ([10.0, 0.05, 0.8, 0.5, 0.3], [30.0, 0.5, 1.0, 0.0, 1.0]):
        fd_model, an_model = _StubModel(), _StubModel()
        fd = CoverageEstimator(fd_model)._optimize(start)
        an = CoverageEstimator(an_model, gradient="analytic")._optimize(start)
        assert an.success and an_model.grad_calls == an.nfev and an_model.points == an.nfev  # one point a gradient
        assert fd_model.points == 6 * fd.nfev
        assert an.fun <= fd.fun + 2.22e-9 * max(abs(fd.fun), 1.0)
        assert np.allclose(an.x[:4], [12.0, 0.03, 0.9, 0.4], atol=0.01) and abs(an.x[4] - 0.2) < 0.1  # (quartic in q: flat)
    fix = [None, None, 0.7, None, 0.25]
    res, ok = CoverageEstimator(_StubModel(), err_scale=10, fix=fix, gradient="analytic").compute_coverage(
        [9.0, 0.04, 0.5, 0.5, 0.5])
    assert ok and abs(res[0] - 12.0) < 1e-3 and abs(res[1] - 0.03) < 1e-5 and abs(res[3] - 0.4) < 1e-3


def test_analytic_lock_step_equals_sequential():
    random.seed(11)
    est_seq = CoverageEstimator(_StubModel(), gradient="analytic")
    starts = initial_grid([11.0, 0.04, 0.8, 0.5, 0.3], count=7, bounds=est_seq.bounds)
    seq = [est_seq._optimize(s) for s in starts]
    model = _StubModel()
    est = CoverageEstimator(model, gradient="analytic")
    lock = _LockStep(est.negll_gradient_points, len(starts))
    par = lock.map(est._optimize, starts)
    assert all(_same(a, b) for a, b in zip(seq, par))
    assert lock.rounds == max(r.nfev for r in par) == model.grad_calls and lock.points == sum(r.nfev for r in par)
    want = min(seq, key=lambda r: r.fun)
    for flag in (False, True):
        best = CoverageEstimator(_StubModel(), lock_step=flag, gradient="analytic")._best_of(starts)
        assert np.array_equal(best.x, want.x)


def test_option_is_checked():
    with pytest.raises(ValueError):
        CoverageEstimator(_StubModel(), gradient="analytic", reference_specials=True)
    with pytest.raises(ValueError):
        CoverageEstimator(_StubModel(), gradient="analytic", batched=False)
    with pytest.raises(ValueError):
        CoverageEstimator(_StubModel(), gradient="exact")
    assert CoverageEstimator(_StubModel()).gradient == "fd"


def test_default_route_is_untouched():
    """gradient="fd" is the default and produces, bit for bit, the iterates scipy's own differencing of the scalar
    objective produces (the reference's call pattern) -- and never asks the model for a gradient."""
    for start in ([10.0, 0.05, 0.8, 0.5, 0.3], [0.01, 0.0, 0.3, 1.0, 0.0]):
        plain, default, named = _StubModel(), _StubModel(), _StubModel()
        a = CoverageEstimator(plain, batched=False)._optimize(start)
        b = CoverageEstimator(default)._optimize(start)
        c = CoverageEstimator(named, gradient="fd")._optimize(start)
        assert _same(a, b) and _same(a, c) and b.nfev == c.nfev
        assert default.grad_calls == named.grad_calls == 0 and default.points == plain.points
