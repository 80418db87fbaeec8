"""The derivative kernel (ll_deriv.hip: K-grad, K-hess, K-opg) at the shapes its layout can break, against the 50-digit
restatement of tests/golden/deriv_shapes.json (tests/golden/make_golden_deriv_shapes.py): every error-class count S that
cuts a wave differently, threshold_o - 1 below, on and past the tile, key counts around the wave and the 256-key segment,
zero-count, unordered and isolated keys, the parameters' edges -- and a call of more points than one launch takes, and a
counted key with a subnormal p_j.  The tolerances are the other derivative tests' (tests/parity_helpers.py)."""
import functools
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist, rel_err
from parity_helpers import TOL, _grad_bound, _hess_bound, _model, _opg_bound, _opg_slack, _tail_delta

pytestmark = pytest.mark.gpu

MODES = {"grad": "loglikelihood_gradient_points", "hess": "loglikelihood_hessian_points", "opg": "loglikelihood_score_outer_points"}
POINTS_PER_LAUNCH = 16384  # ll_deriv.hip kDerivPointsPerLaunch


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_golden("deriv_shapes.json")


def _hist_of(case):
    h = _fixture()["hists"][case["hist"]]
    return dict(zip(h["keys"], h["counts"]))  # (dictionary order is part of the input)


def _square(tri, P):
    M = np.zeros((P, P))
    at = 0
    for k in range(P):
        for l in range(k, P):
            M[k, l] = M[l, k] = tri[at]
            at += 1
    return M


def _evaluate(m, mode, points):
    out = getattr(m, MODES[mode])(points)
    return out if len(out) == 3 else (out[0], out[1], None)


@pytest.mark.parametrize("mode", list(MODES))
def test_every_shape_point(hip_lib, mode):
    """ll to 1e-9; per gradient component 1e-9 Cg_k plus the tail term of _grad_bound; per Hessian / outer-product entry
    1e-9 C_kl + s_kl (tests/test_gpu_hessian.py, tests/test_gpu_opg.py: the same helpers).  No fixture point is left out.
    Printed: the worst |diff| / C per shape class (keys, tile, feature, param), the figures of DESIGN.md 6e, 6f, 6j."""
    g = _fixture()
    n = 0
    worst = {}  # (shape class, quantity) -> worst |diff| / C

    def note(cls, what, v):
        for key in (cls, "all"):
            worst[(key, what)] = max(worst.get((key, what), 0.0), v)

    for case in g["cases"]:
        m = _model(case, hist=_hist_of(case))
        P = m.param_count
        ll, grad, mat = _evaluate(m, mode, case["points"])
        delta = _tail_delta(case["n_keys"])
        tail = case["tail"]
        for i, point in enumerate(case["points"]):
            n += 1
            cls = case["cls"][i][0].split("/")[0]
            what = (case["cls"][i], point)
            assert int(m.get_hist_threshold_values([m.fit_to_bounds(point)[2:5]])[0]) == case["T"][i] if P == 5 else True
            e = rel_err(float(ll[i]), case["ll"][i])
            note(cls, "ll rel", e)
            assert e <= TOL, (what, float(ll[i]), case["ll"][i])
            sp = case["sp"][i]
            for d, want in enumerate(case["grad"][i]):
                C = case["Cg"][i][d]
                bound = _grad_bound(tail, sp, C, case["D"][i][d], delta)
                diff = abs(float(grad[i, d]) - want)
                if C > 0:
                    note(cls, "|dg| / Cg", diff / C)
                assert diff <= bound, (what, d, float(grad[i, d]), want, diff, bound)
            if mode == "grad":
                continue
            want_m = _square(case["hess" if mode == "hess" else "opg"][i], P)
            C_m = _square(case["C" if mode == "hess" else "Cb"][i], P)
            D2 = _square(case["D2"][i], P)
            D = case["D"][i]
            for k in range(P):
                for l in range(P):
                    if mode == "hess":
                        bound = _hess_bound(tail, sp, C_m[k, l], D2[k, l], D[k], D[l], delta)
                    else:
                        bound = _opg_bound(C_m[k, l], _opg_slack(tail, sp, D[k], D[l], delta))
                    diff = abs(float(mat[i, k, l]) - want_m[k, l])
                    if C_m[k, l] > 0:
                        note(cls, "|dM| / C", diff / C_m[k, l])
                    assert diff <= bound, (what, k, l, float(mat[i, k, l]), want_m[k, l], diff, bound)
        m.close()
    assert n == g["kept"]
    for (cls, what), v in sorted(worst.items()):
        print("%s, %d points, %-8s worst %-10s %.3g" % (mode, n, cls, what, v))


@pytest.mark.parametrize("mode", list(MODES))
def test_zero_pj_is_minus_inf_and_nan(hip_lib, mode):
    """The isolated key with p_j = 0 in a double: LL = -inf as K-direct has it, every derivative entry NaN (the convention
    of test_clamp_and_nan_conventions), and a finite point beside it in the same call is untouched."""
    g = _fixture()
    (case,) = g["neg_inf"]
    m = _model(case, hist=_hist_of(case))
    beside = next(c for c in g["cases"] if c["hist"] == case["hist"] and c["model"] == case["model"])
    ll, grad, mat = _evaluate(m, mode, [case["point"], beside["points"][0]])
    assert ll[0] == -math.inf and np.all(np.isnan(grad[0])) and (mat is None or np.all(np.isnan(mat[0])))
    assert ll[0] == m.loglikelihood_points([case["point"]], kernel="direct")[0]
    assert rel_err(float(ll[1]), beside["ll"][0]) <= TOL and np.all(np.isfinite(grad[1])) and (mat is None or np.all(np.isfinite(mat[1])))
    m.close()


def test_modes_agree_at_every_shape(hip_lib):
    """K-hess's and K-opg's value and gradient are K-grad's bits (ll_deriv.hip's header: the same first-order arithmetic);
    the value is K-direct's to 1e-11 relative; the matrices are symmetric bit for bit."""
    g = _fixture()
    n, worst = 0, 0.0
    for case in g["cases"]:
        m = _model(case, hist=_hist_of(case))
        ll, grad = m.loglikelihood_gradient_points(case["points"])
        direct = m.loglikelihood_points(case["points"], kernel="direct")
        for mode in ("hess", "opg"):
            ll_m, grad_m, mat = _evaluate(m, mode, case["points"])
            assert ll_m.tobytes() == ll.tobytes() and grad_m.tobytes() == grad.tobytes(), (mode, case["cls"])
            for i in range(len(case["points"])):
                assert mat[i].tobytes() == np.ascontiguousarray(mat[i].T).tobytes(), (mode, case["cls"][i])
        for i, point in enumerate(case["points"]):
            n += 1
            e = rel_err(float(ll[i]), float(direct[i]))
            worst = max(worst, e)
            assert e <= 1e-11, (case["cls"][i], point, float(ll[i]), float(direct[i]))
        m.close()
    assert n == g["kept"]
    print("%d points: value against K-direct, worst rel %.3g" % (n, worst))


def _known_points(kind, mode):
    """The sim_c10_e0.05 points of the mode's own fixture: [(point, ll, grad, Cg, matrix or None, C or None)] (no tail)."""
    g = load_golden({"grad": "gradient.json", "hess": "hessian.json", "opg": "opg.json"}[mode])
    out = []
    for case in g["cases"]:
        if case["hist"] != "sim_c10_e0.05" or case["model"] != kind or case["tail"] != 0 or case["max_error"] != 8:
            continue
        if (case["k"], case["r"]) != (21, 100) or any(key in case for key in ("threshold", "max_cov", "min_single_copy_ratio")):
            continue
        for i, p in enumerate(case["points"]):
            out.append((p, case["ll"][i], case["grad"][i], case["C" if mode == "grad" else "Cg"][i],
                        None if mode == "grad" else case[mode][i], None if mode == "grad" else case["C"][i]))
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_more_points_than_one_launch(hip_lib, kind, mode):
    """16384 + 16384 + 3 points in one call: launch_ll_deriv cuts it into three launches and offsets the parameters, the
    thresholds and the outputs of each.  At the first and last index of every launch (and 16385) sits a point of the
    mode's own fixture: right against the 50-digit values, and bit for bit what the point gives alone.  The whole call is
    bit for bit the same list evaluated in pieces cut at 10 000 and 20 000.  Repeats: threshold_o varies from point to
    point across both launch boundaries."""
    n = 2 * POINTS_PER_LAUNCH + 3
    case = {"model": kind, "hist": "sim_c10_e0.05", "k": 21, "r": 100, "tail": 0, "max_error": 8}
    m = _model(case)
    rng = np.random.default_rng(23)
    if kind == "repeats":
        pts = np.column_stack([rng.uniform(5.0, 15.0, n), rng.uniform(0.005, 0.1, n), rng.uniform(0.3, 1.0, n), rng.uniform(0.0, 1.0, n),
                               rng.uniform(0.15, 1.0, n)])
    else:
        pts = np.column_stack([rng.uniform(5.0, 15.0, n), rng.uniform(0.005, 0.1, n)])
    known = _known_points(kind, mode)
    assert known
    places = [0, POINTS_PER_LAUNCH - 1, POINTS_PER_LAUNCH, POINTS_PER_LAUNCH + 1, 2 * POINTS_PER_LAUNCH - 1, 2 * POINTS_PER_LAUNCH, n - 1]
    for j, at in enumerate(places):
        pts[at] = known[j % len(known)][0]
    if kind == "repeats":
        T = m.get_hist_threshold_values(np.array([m.fit_to_bounds(p)[2:5] for p in pts]))
        for edge in (POINTS_PER_LAUNCH, 2 * POINTS_PER_LAUNCH):
            assert len(set(T[edge - 8:edge].tolist())) > 1 and len(set(T[edge:edge + 3].tolist()) | set(T[edge - 8:edge].tolist())) > 2, T[edge - 8:edge + 3]
    whole = _evaluate(m, mode, pts)
    P = m.param_count
    for j, at in enumerate(places):
        point, ll, grad, Cg, mat, C = known[j % len(known)]
        assert rel_err(float(whole[0][at]), ll) <= TOL, (at, float(whole[0][at]), ll)
        for d in range(P):
            assert abs(float(whole[1][at, d]) - grad[d]) <= _grad_bound(0, 0.0, Cg[d], 0.0, 0.0), (at, d)
        if mat is not None:
            for k in range(P):
                for l in range(P):
                    assert abs(float(whole[2][at, k, l]) - mat[k][l]) <= TOL * C[k][l], (at, k, l)
        alone = _evaluate(m, mode, [point])
        for a, b in zip(whole, alone):
            assert a is None or a[at].tobytes() == b[0].tobytes(), at
    pieces = [_evaluate(m, mode, pts[lo:hi]) for lo, hi in ((0, 10000), (10000, 20000), (20000, n))]
    for q, a in enumerate(whole):
        if a is not None:
            assert a.shape[0] == n and a.tobytes() == np.concatenate([p[q] for p in pieces]).tobytes(), q
    assert np.all(np.isfinite(whole[0])) and np.all(np.isfinite(whole[1]))
    m.close()


@pytest.mark.parametrize("kind", ["basic", "repeats"])
def test_subnormal_pj(hip_lib, kind):
    """A counted key (the isolated one, count 2) whose p_j is a subnormal double while LL is finite.  The value is
    K-direct's.  The gradient: the key's score d_k p / p is a quotient of two subnormals; what a correct double evaluation
    can deliver there is the fixture's `bound` = h |d_k p / p| 2^-52 / (p / 2^-1074) for that key, beside the usual
    1e-9 Cg_k.  K-hess and K-opg return K-grad's bits there too, and no NaN at a finite LL."""
    g = _fixture()
    (case,) = [c for c in g["subnormal"] if c["model"] == kind]
    assert 0.0 < case["p"] < 2.2250738585072014e-308
    m = _model(case, hist=_hist_of(case))
    ll, grad = m.loglikelihood_gradient_points([case["point"]])
    direct = m.loglikelihood_points([case["point"]], kernel="direct")
    print("%s: p_j %.6g (%.3g units of 2^-1074); ll %.17g, K-direct %.17g, 50 digits %.17g" % (
        kind, case["p"], case["p"] / 2.0 ** -1074, ll[0], direct[0], case["ll"]))
    for d in range(m.param_count):
        diff = abs(float(grad[0, d]) - case["grad"][d])
        print("    d%d: got %.17g want %.17g |diff| %.3g = %.3g Cg; bound %.3g + %.3g" % (
            d, grad[0, d], case["grad"][d], diff, diff / case["Cg"][d] if case["Cg"][d] else 0.0, case["bound"][d], TOL * case["Cg"][d]))
    assert math.isfinite(ll[0]) and rel_err(float(ll[0]), float(direct[0])) <= 1e-11
    assert np.all(np.isfinite(grad[0]))
    for d in range(m.param_count):
        assert abs(float(grad[0, d]) - case["grad"][d]) <= case["bound"][d] + TOL * case["Cg"][d], d
    for mode in ("hess", "opg"):
        ll_m, grad_m, mat = _evaluate(m, mode, [case["point"]])
        assert ll_m.tobytes() == ll.tobytes() and grad_m.tobytes() == grad.tobytes(), mode
        assert np.all(np.isfinite(mat)), mode
    m.close()
