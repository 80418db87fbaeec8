"""The observed information without a GPU: covest_amd/information.py on synthetic Hessians handed out by a stand-in
model, the record of report.print_output with and without it, the committed fixture tests/golden/hessian.json against
the rules its generator selected by, and the new entry point declared and bound."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from covest_amd.information import genome_size_se, observed_information, wald_intervals

NAMES5 = ('coverage', 'error_rate', 'q1', 'q2', 'q')


class _Stub:
    """What information.py and print_output touch of a model; loglikelihood_hessian_points hands out -H."""
    k, r = 21, 100
    hist = {1: 100, 2: 50, 7: 3}

    def __init__(self, negll_hessian, params=NAMES5, bounds=((0.01, None), (0, 0.5), (0.3, 1), (0, 1), (0, 1))):
        self.H = np.asarray(negll_hessian, dtype=np.float64)
        self.params = params
        self.bounds = bounds
        self.asked = []

    def loglikelihood_hessian_points(self, points):
        self.asked.append([list(p) for p in points])
        P = len(self.params)
        return np.array([-5.0e7]), np.zeros((1, P)), -self.H.reshape(1, P, P)

    def short_name(self):
        return 'stub'

    def correct_c(self, c):
        return c * (self.r - self.k + 1) / self.r

    def compute_loglikelihood(self, *args):
        return -123.5


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, n))
    return a @ a.T + n * np.eye(n)


def test_all_free_covariance_is_the_inverse():
    H = _spd(5, 1) * 1e4
    m = _Stub(H)
    est = [10.0, 0.05, 0.6, 0.5, 0.3]
    info = observed_information(m, est)
    assert m.asked == [[est]]
    assert info['reason'] is None and info['free'] == [0, 1, 2, 3, 4]
    assert np.array_equal(np.array(info['hessian']), H)  # of -LL, the model's parameters
    cov = np.array(info['covariance'])
    assert np.max(np.abs(cov @ H - np.eye(5))) <= 1e-12
    assert np.max(np.abs(cov - np.linalg.inv(H))) <= 1e-12 * np.max(np.abs(cov))
    corr = np.array(info['correlation'])
    assert np.allclose(np.diag(corr), 1.0, rtol=0, atol=1e-14) and np.all(np.abs(corr) <= 1 + 1e-14)
    assert np.array_equal(corr, corr.T)
    for d, name in enumerate(NAMES5):
        assert info['standard_errors'][name] == pytest.approx(math.sqrt(cov[d, d]), rel=1e-14)


def test_free_set_rule():
    H = _spd(5, 2)
    # q1 ON its bound, and (1 - q1) annihilates the q2 and q rows: the (c, e) block is what is inverted
    H[2:, :] = 0.0
    H[:, 2:] = 0.0
    H[2, 0] = H[0, 2] = 0.7  # (a q1 row that is not zero: it is the bound that excludes it)
    info = observed_information(_Stub(H), [10.0, 0.05, 1.0, 0.9, 0.6])
    assert info['free'] == [0, 1] and info['reason'] is None
    assert np.max(np.abs(np.array(info['covariance']) - np.linalg.inv(H[:2, :2]))) <= 1e-12
    se = info['standard_errors']
    assert se['q1'] is None and se['q2'] is None and se['q'] is None and se['coverage'] > 0 and se['error_rate'] > 0
    # a fixed parameter is not free, whatever its row
    H = _spd(5, 3)
    info = observed_information(_Stub(H), [10.0, 0.05, 0.6, 0.5, 0.3], fix=[None, 0.05, None, None, None])
    assert info['free'] == [0, 2, 3, 4]
    keep = [0, 2, 3, 4]
    assert np.max(np.abs(np.array(info['covariance']) - np.linalg.inv(H[np.ix_(keep, keep)]))) <= 1e-12
    assert info['standard_errors']['error_rate'] is None
    # the lower bound counts too, an open upper bound (None) never excludes
    info = observed_information(_Stub(_spd(5, 4)), [1e9, 0.0, 0.3, 0.0, 1.0])
    assert info['free'] == [0]
    # nothing free
    info = observed_information(_Stub(_spd(5, 4)), [0.01, 0.0, 0.3, 0.0, 1.0])
    assert info['free'] == [] and info['covariance'] is None and "no free parameter" in info['reason']
    assert all(v is None for v in info['standard_errors'].values())
    with pytest.raises(ValueError):
        observed_information(_Stub(_spd(5, 4)), [10.0, 0.05])
    with pytest.raises(ValueError):
        observed_information(_Stub(_spd(5, 4)), [10.0, 0.05, 0.6, 0.5, 0.3], fix=[None])


def test_not_positive_definite_is_said_not_mended():
    H = _spd(2, 5)
    H[1, 1] = -1.0  # a saddle
    m = _Stub(H, params=NAMES5[:2], bounds=((0.01, None), (0, 0.5)))
    info = observed_information(m, [10.0, 0.05])
    assert info['free'] == [0, 1] and info['covariance'] is None and info['correlation'] is None
    assert "not positive definite" in info['reason'] and "coverage" in info['reason']
    assert info['standard_errors'] == {'coverage': None, 'error_rate': None}
    assert wald_intervals(info) == {'coverage': None, 'error_rate': None}
    assert genome_size_se(m, {1: 10}, info)['genome_size_se'] is None
    # a singular block likewise, and a Hessian that is not finite
    info = observed_information(_Stub([[1.0, 1.0], [1.0, 1.0]], NAMES5[:2], m.bounds), [10.0, 0.05])
    assert info['covariance'] is None and info['reason']
    info = observed_information(_Stub([[math.nan] * 2] * 2, NAMES5[:2], m.bounds), [10.0, 0.05])
    assert info['free'] == [] and "not finite" in info['reason'] and info['standard_errors']['coverage'] is None


def test_wald_intervals_and_delta_method():
    from scipy.stats import norm
    H = np.diag([1.0 / 0.02 ** 2, 1.0 / 0.3 ** 2])  # se 0.02 and 0.3
    m = _Stub(H, params=NAMES5[:2], bounds=((0.01, None), (0, 0.5)))
    info = observed_information(m, [10.0, 0.05])
    assert info['standard_errors']['coverage'] == pytest.approx(0.02, rel=1e-12)
    z = float(norm.ppf(0.975))
    iv = wald_intervals(info)
    assert iv['coverage'] == pytest.approx((10.0 - z * 0.02, 10.0 + z * 0.02), rel=1e-12)
    assert iv['error_rate'] == (0.0, 0.5)  # 0.05 +- 0.59 clipped to the model's bounds
    z90 = float(norm.ppf(0.95))
    assert wald_intervals(info, level=0.9)['coverage'] == pytest.approx((10.0 - z90 * 0.02, 10.0 + z90 * 0.02), rel=1e-12)
    for bad in (0.0, 1.0, -0.5, 1.5, None, "0.95"):
        with pytest.raises(ValueError):
            wald_intervals(info, level=bad)
        with pytest.raises(ValueError):
            genome_size_se(m, {1: 10}, info, level=bad)
    hist_orig = {1: 1000, 2: 400, 10: 20}
    occurrences = 2000
    for factor in (1, 2):
        size = genome_size_se(m, hist_orig, info, sample_factor=factor)
        G = occurrences / (10.0 * factor * 0.8)
        assert size['genome_size'] == pytest.approx(G, rel=1e-15)
        assert size['genome_size_se'] == pytest.approx(G * 0.02 / 10.0, rel=1e-12)  # G ~ 1 / c
        lo, hi = size['genome_size_wald_interval']
        assert lo == pytest.approx(G - z * size['genome_size_se'], rel=1e-12) and hi == pytest.approx(G + z * size['genome_size_se'], rel=1e-12)
    # the delta method against the mapping itself, one standard error to either side (first order)
    up = occurrences / ((10.0 - 0.02) * 0.8)
    assert genome_size_se(m, hist_orig, info)['genome_size_se'] == pytest.approx(up - occurrences / 8.0, rel=5e-3)


def test_print_output_with_and_without_information():
    import yaml
    from covest_amd.report import print_output
    H = np.diag([1.0 / 0.02 ** 2, 1.0 / 0.001 ** 2])
    m = _Stub(H, params=NAMES5[:2], bounds=((0.01, None), (0, 0.5)))
    hist_orig = {1: 1000, 2: 400, 10: 20}
    args = dict(estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True)
    plain = print_output(hist_orig, m, True, 2, **args)
    assert print_output(hist_orig, m, True, 2, information=None, **args) == plain
    assert list(print_output(hist_orig, m, True, 2, information=None, **args)) == list(plain)
    assert yaml.dump(print_output(hist_orig, m, True, 2, information=None, **args)) == yaml.dump(plain)
    info = observed_information(m, [10.0, 0.05])
    rec = print_output(hist_orig, m, True, 2, information=info, **args)
    assert {k: v for k, v in rec.items() if k in plain} == plain
    assert set(rec) - set(plain) == {'standard_errors', 'wald_intervals', 'genome_size_se', 'genome_size_wald_interval',
                                     'wald_level'}
    assert rec['wald_level'] == 0.95
    assert rec['standard_errors']['coverage'] == pytest.approx(0.04, rel=1e-12)  # the record's coverage is c * sample_factor
    assert rec['standard_errors']['error_rate'] == pytest.approx(0.001, rel=1e-12)
    lo, hi = rec['wald_intervals']['coverage']
    assert lo < rec['coverage'] < hi and hi - lo == pytest.approx(2 * 1.959963984540054 * 0.04, rel=1e-9)
    G = 2000 / (20.0 * 0.8)
    assert rec['genome_size_se'] == pytest.approx(G * 0.02 / 10.0, rel=1e-12)
    assert rec['genome_size_wald_interval'][0] < rec['genome_size'] < rec['genome_size_wald_interval'][1]
    assert yaml.safe_load(yaml.dump(rec)) == rec  # plain data: the record still prints as YAML
    rec90 = print_output(hist_orig, m, True, 2, information=dict(info, level=0.9), **args)
    assert rec90['wald_level'] == 0.9 and rec90['wald_intervals']['coverage'][0] > lo
    # not identified: None all the way into the record
    saddle = observed_information(_Stub([[1.0, 2.0], [2.0, 1.0]], NAMES5[:2], m.bounds), [10.0, 0.05])
    rec = print_output(hist_orig, m, True, 2, information=saddle, **args)
    assert rec['standard_errors'] == {'coverage': None, 'error_rate': None} and rec['genome_size_se'] is None
    assert rec['genome_size_wald_interval'] is None and rec['wald_intervals'] == {'coverage': None, 'error_rate': None}


def test_fixture_shape_and_selection_rule():
    """hessian.json: the conditions the issue sets (at least 50 of gradient.json's points, every category present), each
    matrix symmetric bit for bit with zero rows and columns where the point's parameter is clamped, each entry within its
    condition sum, and the rule the generator selected by: s_kl <= 1e-9 C_kl."""
    g = load_golden("hessian.json")
    grad = load_golden("gradient.json")
    known = {(c["source"], tuple(p)): (c["ll"][i], c["grad"][i], c["C"][i]) for c in grad["cases"] for i, p in enumerate(c["points"])}
    seen, n = set(), 0
    for case in g["cases"]:
        P = 5 if case["model"] == "repeats" else 2
        delta = g["k_tail"] * 2.0 ** -52 * case["n_keys"]
        tail = case["tail"]
        for i, point in enumerate(case["points"]):
            n += 1
            ll, gr, Cg = known[(case["source"], tuple(point))]  # a candidate of gradient.json, the same numbers
            assert case["ll"][i] == ll and case["grad"][i] == gr and np.allclose(case["Cg"][i], Cg, rtol=1e-14, atol=0)
            H, C, D2, D = (np.array(case[k][i]) for k in ("hess", "C", "D2", "D"))
            assert H.shape == C.shape == D2.shape == (P, P) and np.all(np.isfinite(H))
            assert np.array_equal(H, H.T) and np.array_equal(C, C.T)
            assert np.all(np.abs(H) <= C * (1 + 1e-12))
            moved = case["moved"][i]
            for d in range(P):
                if moved[d]:
                    assert not H[d].any() and not H[:, d].any() and case["grad"][i][d] == 0.0
            sp = case["sp"][i]
            if tail and sp < 1:
                for k in range(P):
                    for l in range(P):
                        if not (moved[k] or moved[l]):
                            s_kl = abs(tail) * (D2[k, l] * delta / (1 - sp) ** 2 + 2 * D[k] * D[l] * delta / (1 - sp) ** 3)
                            assert s_kl <= 1e-9 * C[k, l] * (1 + 1e-9)
            seen.add("%s/%s" % (case["model"], "tail" if tail else "no tail"))
            if case["hist"] == "H10k_rep":
                seen.add("full H10k_rep")
            if point[1] <= 0.0:
                seen.add("e = 0")
            if any(moved):
                seen.add("clamped")
            if case["source"].startswith("own_optimum.json") or (case["source"] == "own: sim_c10_e0.05, repeats" and i == 0):
                seen.add("optimum " + case["model"])
    assert n == g["kept"] and g["kept"] + g["dropped"] == g["candidates"] == grad["kept"] == 70
    assert g["kept"] >= 50
    assert seen >= {"basic/no tail", "basic/tail", "repeats/no tail", "repeats/tail", "full H10k_rep", "e = 0", "clamped",
                    "optimum basic", "optimum repeats"}
    assert g["worst_diff_check"] <= 1e-20 and g["entries_diff_checked"] > 0
    opt = load_golden("own_optimum.json")["models"]["repeats"]
    rep = next(c for c in g["cases"] if c["source"] == "own: sim_c10_e0.05, repeats")
    assert rep["points"][0] == [opt[k] for k in NAMES5]
    H = np.array(rep["hess"][0])
    assert not H[3].any() and not H[4].any() and H[0, 0] < 0 and H[1, 1] < 0  # q1 = 1: q2 and q are not identified there


def test_entry_point_declared_and_bound(hip_lib):
    from covest_amd import _capi
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+covest_eval_points_hess\s*\(\s*covest_model\s*\*\s*m\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*"
                     r"\s*params\s*,\s*double\s*\*\s*out_ll\s*,\s*double\s*\*\s*out_grad\s*,\s*double\s*\*\s*out_hess\s*\)", text)
    assert "covest_eval_points_hess" in _capi.EXPORTS
    assert hasattr(hip_lib, "covest_eval_points_hess")
    assert hip_lib.covest_abi_version() == 1
    from covest_amd import BasicModel, RepeatsModel
    for cls in (BasicModel, RepeatsModel):
        assert callable(cls.loglikelihood_hessian_points) and callable(cls.compute_loglikelihood_hessian)
    import covest_amd
    assert covest_amd.observed_information is observed_information
