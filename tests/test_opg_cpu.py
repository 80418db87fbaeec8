"""The sandwich covariance without a GPU: covest_amd/information.py's sandwich_covariance on matrices handed out by a
stand-in model, the record of report.print_output with and without it, the committed fixture tests/golden/opg.json
against the rules its generator selected by, and the new entry point declared and bound."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

NAMES5 = ('coverage', 'error_rate', 'q1', 'q2', 'q')
BOUNDS5 = ((0.01, None), (0, 0.5), (0.3, 1), (0, 1), (0, 1))
EPS = 2.0 ** -52


class _Stub:
    """What information.py and print_output touch of a model: loglikelihood_hessian_points hands out -A,
    loglikelihood_score_outer_points the chosen gradient g and B.  n = sum h + tail = 153 + 47 = 200."""
    k, r = 21, 100
    hist = {1: 100, 2: 50, 7: 3}
    tail = 47

    def __init__(self, A, B, g, params=NAMES5, bounds=BOUNDS5):
        self.A, self.B, self.g = (np.asarray(v, dtype=np.float64) for v in (A, B, g))
        self.params = params
        self.bounds = bounds
        self.asked = []

    def loglikelihood_hessian_points(self, points):
        P = len(self.params)
        return np.array([-5.0e7]), self.g.reshape(1, P).copy(), -self.A.reshape(1, P, P)

    def loglikelihood_score_outer_points(self, points):
        self.asked.append([list(p) for p in points])
        P = len(self.params)
        return np.array([-5.0e7]), self.g.reshape(1, P).copy(), self.B.reshape(1, P, P).copy()

    def short_name(self):
        return 'stub'

    def correct_c(self, c):
        return c * (self.r - self.k + 1) / self.r

    def compute_loglikelihood(self, *args):
        return -123.5


N_OBS = 200.0
EST5 = [10.0, 0.05, 0.6, 0.5, 0.3]


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, n))
    return a @ a.T + n * np.eye(n)


def _uncentred(centred, g):
    return centred + np.outer(g, g) / N_OBS


def test_meat_equal_to_information_gives_the_models_covariance():
    from covest_amd.information import observed_information, sandwich_covariance
    A = _spd(5, 1) * 1e4
    g = np.array([3.0, -40.0, 0.5, 0.0, -2.0])
    m = _Stub(A, _uncentred(A, g), g)
    out = sandwich_covariance(m, EST5)
    assert m.asked == [[EST5]]
    assert out['reason'] is None and out['free'] == [0, 1, 2, 3, 4]
    assert np.array_equal(np.array(out['opg']), m.B)  # B as the model returned it, uncentred
    V, cov = np.array(out['robust_covariance']), np.array(out['covariance'])
    assert np.max(np.abs(V - np.linalg.inv(A))) <= 1e-10 * np.max(np.abs(cov))
    assert np.max(np.abs(V - cov)) <= 1e-10 * np.max(np.abs(cov))
    assert len(out['information_ratio']) == 5 and np.allclose(out['information_ratio'], 1.0, rtol=0, atol=1e-10)
    for name in NAMES5:
        assert out['se_ratio'][name] == pytest.approx(1.0, abs=1e-10)
        assert out['robust_standard_errors'][name] == pytest.approx(out['standard_errors'][name], rel=1e-10)
    # an information dict handed in is used, not recomputed, and not changed
    info = observed_information(m, EST5)
    before = dict(info)
    again = sandwich_covariance(m, EST5, info=info)
    assert info == before and 'opg' not in info
    assert again['robust_covariance'] == out['robust_covariance'] and again['hessian'] == info['hessian']


def test_scaled_meat_scales_the_covariance_and_general_meat_is_the_product():
    from covest_amd.information import sandwich_covariance
    A = _spd(5, 2) * 1e3
    g = np.array([1.0, 2.0, -3.0, 4.0, -5.0])
    out = sandwich_covariance(_Stub(A, _uncentred(4.0 * A, g), g), EST5)
    inv = np.linalg.inv(A)
    assert np.max(np.abs(np.array(out['robust_covariance']) - 4.0 * inv)) <= 1e-10 * np.max(np.abs(inv))
    assert np.allclose(out['information_ratio'], 4.0, rtol=1e-10, atol=0)
    for name in NAMES5:
        assert out['se_ratio'][name] == pytest.approx(2.0, rel=1e-10)
    # any meat: V = A^-1 B_c A^-1, the ratios the eigenvalues of A^-1 B_c, ascending
    Bc = _spd(5, 3) * 2e3
    out = sandwich_covariance(_Stub(A, _uncentred(Bc, g), g), EST5)
    want = inv @ Bc @ inv
    V = np.array(out['robust_covariance'])
    assert np.max(np.abs(V - want)) <= 1e-10 * np.max(np.abs(want))
    eig = np.sort(np.linalg.eigvals(inv @ Bc).real)
    assert np.allclose(out['information_ratio'], eig, rtol=1e-9, atol=0)
    assert out['information_ratio'] == sorted(out['information_ratio'])
    for d, name in enumerate(NAMES5):
        assert out['robust_standard_errors'][name] == pytest.approx(math.sqrt(want[d, d]), rel=1e-10)
        assert out['se_ratio'][name] == pytest.approx(math.sqrt(want[d, d] / inv[d, d]), rel=1e-10)
    # the centring counts: the same B with another gradient is another covariance
    other = sandwich_covariance(_Stub(A, _uncentred(Bc, g), 10.0 * g), EST5)
    want = inv @ (_uncentred(Bc, g) - np.outer(10.0 * g, 10.0 * g) / N_OBS) @ inv
    assert np.max(np.abs(np.array(other['robust_covariance']) - want)) <= 1e-10 * np.max(np.abs(want))


def test_cannot_be_formed_is_said_not_mended():
    from covest_amd.information import genome_size_se, sandwich_covariance, wald_intervals
    names, bounds = NAMES5[:2], BOUNDS5[:2]
    saddle = _spd(2, 5)
    saddle[1, 1] = -1.0
    g = np.zeros(2)
    m = _Stub(saddle, _spd(2, 6), g, names, bounds)
    out = sandwich_covariance(m, [10.0, 0.05])
    assert "not positive definite" in out['reason']
    assert out['robust_covariance'] is None and out['information_ratio'] is None
    assert out['robust_standard_errors'] == {'coverage': None, 'error_rate': None} == out['se_ratio']
    assert np.array_equal(np.array(out['opg']), m.B)
    assert wald_intervals(out, robust=True) == {'coverage': None, 'error_rate': None}
    assert genome_size_se(m, {1: 10}, out, robust=True)['genome_size_se'] is None
    # a B that is not finite: the model's covariance stands, the robust one is None, and the reason says which
    A = _spd(2, 7)
    for bad in (math.nan, math.inf):
        out = sandwich_covariance(_Stub(A, [[bad, 1.0], [1.0, 2.0]], g, names, bounds), [10.0, 0.05])
        assert out['covariance'] is not None and out['standard_errors']['coverage'] > 0
        assert out['robust_covariance'] is None and out['information_ratio'] is None
        assert out['robust_standard_errors'] == {'coverage': None, 'error_rate': None} == out['se_ratio']
        assert "outer product" in out['reason'] and "not finite" in out['reason']
    out = sandwich_covariance(_Stub(A, _spd(2, 8), [math.nan, 0.0], names, bounds), [10.0, 0.05])
    assert out['robust_covariance'] is None and "not finite" in out['reason']


def test_fixed_and_on_bound_parameters_are_left_out_of_both_matrices():
    from covest_amd.information import sandwich_covariance
    A, Bc = _spd(5, 9) * 1e3, _spd(5, 10) * 1e3
    g = np.array([1.0, -2.0, 3.0, -4.0, 5.0])
    m = _Stub(A, _uncentred(Bc, g), g)
    # the error rate held fixed, q ON its upper bound
    out = sandwich_covariance(m, [10.0, 0.05, 0.6, 0.5, 1.0], fix=[None, 0.05, None, None, None])
    keep = [0, 2, 3]
    assert out['free'] == keep and out['reason'] is None
    inv = np.linalg.inv(A[np.ix_(keep, keep)])
    want = inv @ Bc[np.ix_(keep, keep)] @ inv
    V = np.array(out['robust_covariance'])
    assert V.shape == (3, 3) and np.max(np.abs(V - want)) <= 1e-10 * np.max(np.abs(want))
    assert len(out['information_ratio']) == 3
    assert np.allclose(out['information_ratio'], np.sort(np.linalg.eigvals(inv @ Bc[np.ix_(keep, keep)]).real), rtol=1e-9, atol=0)
    for name in ('error_rate', 'q'):
        assert out['robust_standard_errors'][name] is None and out['se_ratio'][name] is None
    for at, d in enumerate(keep):
        assert out['robust_standard_errors'][NAMES5[d]] == pytest.approx(math.sqrt(want[at, at]), rel=1e-10)
    # entries of the excluded rows do not matter, even when they are not finite in A^-1's sense (huge)
    B2 = m.B.copy()
    B2[1, :] = B2[:, 1] = 1e30
    out2 = sandwich_covariance(_Stub(A, B2, g), [10.0, 0.05, 0.6, 0.5, 1.0], fix=[None, 0.05, None, None, None])
    assert out2['robust_covariance'] == out['robust_covariance']


def test_robust_wald_intervals_and_genome_size():
    from covest_amd.information import genome_size_se, sandwich_covariance, wald_intervals
    A = np.diag([1.0 / 0.02 ** 2, 1.0 / 0.001 ** 2])
    g = np.zeros(2)
    m = _Stub(A, 9.0 * A, g, NAMES5[:2], BOUNDS5[:2])
    out = sandwich_covariance(m, [10.0, 0.05])
    assert out['robust_standard_errors']['coverage'] == pytest.approx(0.06, rel=1e-12)
    z = 1.959963984540054
    assert wald_intervals(out)['coverage'] == pytest.approx((10.0 - z * 0.02, 10.0 + z * 0.02), rel=1e-12)
    assert wald_intervals(out, robust=True)['coverage'] == pytest.approx((10.0 - z * 0.06, 10.0 + z * 0.06), rel=1e-12)
    hist_orig = {1: 1000, 2: 400, 10: 20}
    G = 2000 / (10.0 * 0.8)
    assert genome_size_se(m, hist_orig, out)['genome_size_se'] == pytest.approx(G * 0.02 / 10.0, rel=1e-12)
    assert genome_size_se(m, hist_orig, out, robust=True)['genome_size_se'] == pytest.approx(G * 0.06 / 10.0, rel=1e-12)


def test_print_output_gains_exactly_three_keys_with_the_sandwich():
    import yaml
    from covest_amd.information import observed_information, sandwich_covariance
    from covest_amd.report import print_output
    A = np.diag([1.0 / 0.02 ** 2, 1.0 / 0.001 ** 2])
    m = _Stub(A, 9.0 * A, np.zeros(2), NAMES5[:2], BOUNDS5[:2])
    hist_orig = {1: 1000, 2: 400, 10: 20}
    args = dict(estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True)
    info = observed_information(m, [10.0, 0.05])
    without = print_output(hist_orig, m, True, 2, information=info, **args)
    assert not [key for key in without if 'robust' in key]
    rec = print_output(hist_orig, m, True, 2, information=sandwich_covariance(m, [10.0, 0.05], info=info), **args)
    assert {k: v for k, v in rec.items() if k in without} == without
    assert set(rec) - set(without) == {'robust_standard_errors', 'robust_wald_intervals', 'genome_size_robust_se'}
    assert list(rec)[:len(without)] == list(without)
    # the record's coverage is c * sample_factor, and so are its errors
    assert rec['robust_standard_errors'] == {'coverage': pytest.approx(0.12, rel=1e-12), 'error_rate': pytest.approx(0.003, rel=1e-12)}
    lo, hi = rec['robust_wald_intervals']['coverage']
    assert lo < rec['coverage'] < hi and hi - lo == pytest.approx(2 * 1.959963984540054 * 0.12, rel=1e-9)
    assert hi - lo == pytest.approx(3 * (rec['wald_intervals']['coverage'][1] - rec['wald_intervals']['coverage'][0]), rel=1e-9)
    assert rec['genome_size_robust_se'] == pytest.approx(3 * rec['genome_size_se'], rel=1e-12)
    assert yaml.safe_load(yaml.dump(rec)) == rec  # plain data: the record still prints as YAML
    # the sandwich could not be formed: the three keys are there and say None
    bad = sandwich_covariance(_Stub(A, [[math.nan] * 2] * 2, np.zeros(2), NAMES5[:2], BOUNDS5[:2]), [10.0, 0.05])
    rec = print_output(hist_orig, m, True, 2, information=bad, **args)
    assert rec['robust_standard_errors'] == {'coverage': None, 'error_rate': None} == rec['robust_wald_intervals']
    assert rec['genome_size_robust_se'] is None and rec['genome_size_se'] is not None


def _fixture_points():
    g = load_golden("opg.json")
    for case in g["cases"]:
        for i, point in enumerate(case["points"]):
            yield g, case, i, point


def test_fixture_shape_and_selection_rule():
    """opg.json: the conditions the issue sets (at most 10 of gradient.json's 70 points dropped, every category that
    test_hessian_cpu.py requires of hessian.json present), value and gradient gradient.json's doubles, each matrix
    symmetric bit for bit with zero rows and columns where the point's parameter is clamped, a diagonal >= 0, each entry
    within its condition sum, the stored slack the formula's, and the rule the generator selected by: s_kl <= 1e-9 C_kl."""
    grad = load_golden("gradient.json")
    known = {(c["source"], tuple(p)): (c["ll"][i], c["grad"][i], c["C"][i], c["D"][i]) for c in grad["cases"]
             for i, p in enumerate(c["points"])}
    seen, n = set(), 0
    for g, case, i, point in _fixture_points():
        P = 5 if case["model"] == "repeats" else 2
        delta = g["k_tail"] * EPS * case["n_keys"]
        tail = case["tail"]
        n += 1
        ll, gr, Cg, D = known[(case["source"], tuple(point))]  # a candidate of gradient.json, the same numbers
        assert case["ll"][i] == ll and case["grad"][i] == gr
        assert np.allclose(case["Cg"][i], Cg, rtol=1e-14, atol=0) and np.allclose(case["D"][i], D, rtol=1e-14, atol=0)
        B, C, s = (np.array(case[k][i]) for k in ("opg", "C", "s"))
        assert B.shape == C.shape == s.shape == (P, P) and np.all(np.isfinite(B))
        assert np.array_equal(B, B.T) and np.array_equal(C, C.T) and np.array_equal(s, s.T)
        assert np.all(np.diag(B) >= 0.0)
        assert np.all(np.abs(B) <= C * (1 + 1e-12))
        moved = case["moved"][i]
        for d in range(P):
            if moved[d]:
                assert not B[d].any() and not B[:, d].any() and case["grad"][i][d] == 0.0
            else:
                assert B[d, d] == pytest.approx(C[d, d], rel=1e-14)  # a sum of squares: its own condition sum
        sp = case["sp"][i]
        D = np.array(case["D"][i])
        if tail and sp < 1:
            want_s = abs(tail) * 2 * np.outer(D, D) * delta / (1 - sp) ** 3
            assert np.allclose(s, want_s, rtol=1e-9, atol=0)  # (1 - sp of the stored double: 1e-6 at the least)
            for k in range(P):
                for l in range(P):
                    if not (moved[k] or moved[l]):
                        assert s[k, l] <= 1e-9 * C[k, l]
        else:
            assert not s.any()
        seen.add("%s/%s" % (case["model"], "tail" if tail else "no tail"))
        if case["hist"] == "H10k_rep":
            seen.add("full H10k_rep")
        if point[1] <= 0.0:
            seen.add("e = 0")
        if any(moved):
            seen.add("clamped")
        if case["source"].startswith("own_optimum.json") or (case["source"] == "own: sim_c10_e0.05, repeats" and i == 0):
            seen.add("optimum " + case["model"])
    g = load_golden("opg.json")
    assert n == g["kept"] and g["kept"] + g["dropped"] == g["candidates"] == grad["kept"] == 70
    assert g["dropped"] <= 10
    assert seen >= {"basic/no tail", "basic/tail", "repeats/no tail", "repeats/tail", "full H10k_rep", "e = 0", "clamped",
                    "optimum basic", "optimum repeats"}
    hess = load_golden("hessian.json")
    assert g["worst_identity_check"] <= 1e-20 and 0 < g["points_identity_checked"] <= hess["kept"]
    opt = load_golden("own_optimum.json")["models"]["repeats"]
    rep = next(c for c in g["cases"] if c["source"] == "own: sim_c10_e0.05, repeats")
    assert rep["points"][0] == [opt[k] for k in NAMES5]
    B = np.array(rep["opg"][0])
    assert not B[3].any() and not B[4].any() and B[0, 0] > 0 and B[1, 1] > 0  # q1 = 1: (1 - q1) annihilates q2's and q's scores


def test_every_stored_matrix_is_positive_semidefinite():
    """B is a sum of h r r^T (h > 0) and tail S S^T (tail > 0): positive semi-definite.  Scaled to M = B_kl / sqrt(B_kk B_ll)
    over the rows with B_kk > 0 (|M_kl| <= 1 by Cauchy-Schwarz, unit diagonal) the stored doubles are off the exact matrix
    by at most eps an entry, P eps in norm, and eigvalsh by about P eps ||M|| <= P^2 eps more: the smallest eigenvalue
    may not be below -4 P^2 eps."""
    worst = 0.0
    for g, case, i, point in _fixture_points():
        B = np.array(case["opg"][i])
        assert case["tail"] >= 0
        live = [d for d in range(len(B)) if B[d, d] > 0.0]
        assert not B[[d for d in range(len(B)) if d not in live]].any()  # a zero diagonal entry: a zero row
        if not live:
            continue
        scale = 1.0 / np.sqrt(np.diag(B)[live])
        M = B[np.ix_(live, live)] * np.outer(scale, scale)
        assert np.all(np.abs(M) <= 1.0 + 4 * EPS), (case["source"], point)
        low = float(np.linalg.eigvalsh(M)[0])
        worst = min(worst, low)
        assert low >= -4.0 * len(live) ** 2 * EPS, (case["source"], point, low)
    print("smallest eigenvalue of a scaled stored matrix: %.3g" % worst)


def test_entry_point_declared_and_bound(hip_lib):
    from covest_amd import _capi
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+covest_eval_points_opg\s*\(\s*covest_model\s*\*\s*m\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*"
                     r"\s*params\s*,\s*double\s*\*\s*out_ll\s*,\s*double\s*\*\s*out_grad\s*,\s*double\s*\*\s*out_opg\s*\)", text)
    assert "covest_eval_points_opg" in _capi.EXPORTS
    assert hasattr(hip_lib, "covest_eval_points_opg")
    assert hip_lib.covest_abi_version() == 1
    from covest_amd import BasicModel, RepeatsModel
    for cls in (BasicModel, RepeatsModel):
        assert callable(cls.loglikelihood_score_outer_points) and callable(cls.compute_loglikelihood_score_outer)
    import covest_amd
    from covest_amd.information import sandwich_covariance
    assert covest_amd.sandwich_covariance is sandwich_covariance
