"""The committed fixture tests/golden/deriv_shapes.json without a GPU: its values against the C oracle, its thresholds
against the model's host code, and the counts and coverage conditions its generator
(tests/golden/make_golden_deriv_shapes.py) asserted, on the file as committed."""
import math

import numpy as np

from conftest import load_golden, rel_err
from parity_helpers import K_TAIL, TOL, _model, _tail_slack

KEY_COUNTS = (1, 64, 65, 255, 256, 257, 513)
TILE_S = (1, 2, 6, 9, 22, 32, 64)
FEATURES = ("zero count in the middle", "zero count last of the last segment", "descending", "shuffled", "gaps, above 1",
            "isolated key")
PARAMS = ("e = 0", "e = 1e-09", "e = 0.5", "c on its bound", "o lambda > 200", "outside its bound")
PARAMS_Q = ("q = 0", "q = 1", "q1 = 1", "q2 = 0", "q2 = 1")


def _hist_of(g, case):
    h = g["hists"][case["hist"]]
    return dict(zip(h["keys"], h["counts"]))


def _tile_edges(S):
    OT = 64 // S
    return sorted({v for v in (1, 2, 3, 4, OT - 1, OT, OT + 1, 2 * OT + 1) if v >= 1})


def test_values_are_the_oracles(oracle):
    """Every ll is the C oracle's log-likelihood of the point (it clamps as compute_loglikelihood does) to 1e-9 relative,
    the parity suite's agreement; the subnormal points too; the -inf case is -inf there."""
    g = load_golden("deriv_shapes.json")
    n, worst = 0, 0.0
    for case in g["cases"] + [dict(c, points=[c["point"]], ll=[c["ll"]]) for c in g["subnormal"]]:
        om = oracle.OracleModel(case["model"], case["k"], case["r"], _hist_of(g, case), case["tail"], max_error=case["max_error"],
                                threshold=case.get("threshold", 1e-8))
        for point, ll in zip(case["points"], case["ll"]):
            n += 1
            got = om.compute_loglikelihood(*point)
            e = rel_err(got, ll)
            worst = max(worst, e)
            assert e <= TOL, (case["hist"], case["max_error"], point, got, ll, e)
    assert n == g["kept"] + len(g["subnormal"])
    print("%d values against the oracle, worst rel %.3g" % (n, worst))
    (case,) = g["neg_inf"]
    om = oracle.OracleModel(case["model"], case["k"], case["r"], _hist_of(g, case), case["tail"], max_error=case["max_error"])
    assert om.compute_loglikelihood(*case["point"]) == -math.inf and case["log10_p"] < -400
    assert om.compute_probabilities(*case["point"])[case["key"]] == 0.0


def test_thresholds_are_the_models(hip_lib):
    """Every stored T is get_hist_threshold_values at the clamped point (2 for the basic model: one copy number), and the
    class a point stands for names it."""
    g = load_golden("deriv_shapes.json")
    for case in g["cases"] + [dict(c, points=[c["point"]], T=[c["T"]], cls=[c["cls"]]) for c in g["subnormal"] + g["neg_inf"]]:
        m = _model(case, hist=_hist_of(g, case))
        for point, T, cls in zip(case["points"], case["T"], case["cls"]):
            if case["model"] == "basic":
                assert T == 2
                continue
            assert T == int(m.get_hist_threshold_values([m.fit_to_bounds(point)[2:5]])[0]), (cls, point)
            S, OT = case["max_error"], 64 // case["max_error"]
            for c in cls:
                if c.startswith("tile/") and not c.endswith("hundreds"):
                    assert c == "tile/S%d/%d" % (S, T - 1)
                if c == "tile/S22/hundreds":
                    assert S == 22 and T - 1 >= 200
                if c == "keys/repeats/below OT":
                    assert T - 1 < OT
                if c == "keys/repeats/tiles and one":
                    assert T - 1 > 2 * OT and (T - 1) % OT == 1


def test_fixture_shape_counts_and_coverage():
    """Kept and dropped counts, the selection rule on every kept point, and the coverage the issue sets: every (model,
    key count), every (S, threshold_o - 1) pair, every feature and parameter edge, each model with and without a tail."""
    g = load_golden("deriv_shapes.json")
    assert g["k_tail"] == K_TAIL
    n, seen = 0, {}
    for case in g["cases"]:
        P = 5 if case["model"] == "repeats" else 2
        NP = P * (P + 1) // 2
        hist = _hist_of(g, case)
        assert case["n_keys"] == len(hist) == len(g["hists"][case["hist"]]["keys"])
        assert case["max_error"] <= min(case["k"] + 1, 64)
        delta = K_TAIL * 2.0 ** -52 * case["n_keys"]
        tail = case["tail"]
        for i, point in enumerate(case["points"]):
            n += 1
            for c in case["cls"][i] + ["%s/%s" % (case["model"], "tail0" if tail == 0 else "tail+")]:
                seen[c] = seen.get(c, 0) + 1
            ll, sp = case["ll"][i], case["sp"][i]
            assert math.isfinite(ll) and len(point) == len(case["grad"][i]) == len(case["Cg"][i]) == len(case["D"][i]) == P
            pairs = [(k, l) for k in range(P) for l in range(k, P)]
            H, C, D2, B, Cb = (np.array(case[name][i]) for name in ("hess", "C", "D2", "opg", "Cb"))
            assert H.shape == C.shape == D2.shape == B.shape == Cb.shape == (NP,)
            assert np.all(np.abs(H) <= C * (1 + 1e-12)) and np.all(np.abs(B) <= Cb * (1 + 1e-12))
            assert np.all(np.abs(case["grad"][i]) <= np.array(case["Cg"][i]) * (1 + 1e-12))
            moved, D = case["moved"][i], case["D"][i]
            assert moved == [float(a) != float(b) for a, b in zip(point, _clamp(case, point))]
            for at, (k, l) in enumerate(pairs):
                if moved[k] or moved[l]:
                    assert H[at] == 0.0 and B[at] == 0.0
                elif k == l:
                    assert B[at] >= 0.0 and abs(B[at] - Cb[at]) <= 1e-14 * Cb[at]  # a sum of squares: its own condition sum
            for d in range(P):
                assert not moved[d] or case["grad"][i][d] == 0.0
            if tail:  # the rule the generator selected by
                assert abs(1 - sp) >= 1e-6 and _tail_slack(tail, ll, sp, case["n_keys"])[1] is None
                if sp < 1:
                    for d in range(P):
                        if not moved[d]:
                            assert 1e-9 * case["Cg"][i][d] * (1 + 1e-9) >= abs(tail) * D[d] * delta / (1 - sp) ** 2
                    for at, (k, l) in enumerate(pairs):
                        if not (moved[k] or moved[l]):
                            s_h = abs(tail) * (D2[at] * delta / (1 - sp) ** 2 + 2 * D[k] * D[l] * delta / (1 - sp) ** 3)
                            s_b = abs(tail) * 2 * D[k] * D[l] * delta / (1 - sp) ** 3
                            assert s_h <= 1e-9 * C[at] * (1 + 1e-9) and s_b <= 1e-9 * Cb[at] * (1 + 1e-9)
    for c in g["subnormal"] + g["neg_inf"]:
        for name in c["cls"]:
            seen[name] = seen.get(name, 0) + 1
    assert n == g["kept"] and g["kept"] + g["dropped"] + len(g["subnormal"]) + len(g["neg_inf"]) == g["candidates"]
    assert 100 <= g["kept"] <= 150 and g["dropped"] <= 0.10 * g["candidates"]
    assert seen == g["classes"]
    need = ["keys/%s/%d" % (model, k) for model in ("basic", "repeats") for k in KEY_COUNTS]
    need += ["keys/%s/%d/%s" % (model, k, t) for model in ("basic", "repeats") for k in KEY_COUNTS for t in ("tail0", "tail+")]
    need += ["keys/repeats/below OT", "keys/repeats/tiles and one", "tile/S22/hundreds"]
    need += ["tile/S%d/%d" % (S, v) for S in TILE_S for v in _tile_edges(S)]
    need += ["%s/%s" % (model, t) for model in ("basic", "repeats") for t in ("tail0", "tail+")]
    need += ["feature/%s/%s" % (f, model) for f in FEATURES for model in ("basic", "repeats")]
    need += ["feature/isolated key, p = 0/basic", "subnormal/basic", "subnormal/repeats"]
    need += ["param/%s/%s" % (p, model) for p in PARAMS for model in ("basic", "repeats")] + ["param/%s/repeats" % p for p in PARAMS_Q]
    assert not [c for c in need if not seen.get(c)], [c for c in need if not seen.get(c)]
    assert g["worst_diff_check"] <= 1e-20 and g["entries_diff_checked"] > 0
    # the shapes themselves
    H = g["hists"]
    for k in KEY_COUNTS:
        assert len(H["keys%d" % k]["keys"]) == k and all(H["keys%d" % k]["counts"])
    assert H["zero_mid300"]["counts"][149] == 0 and H["zero_last512"]["counts"][-1] == 0 and len(H["zero_last512"]["keys"]) == 512
    assert H["desc300"]["keys"] == sorted(H["desc300"]["keys"], reverse=True)
    assert H["shuffled300"]["keys"] != sorted(H["shuffled300"]["keys"]) and sorted(H["shuffled300"]["keys"]) == list(range(1, 301))
    assert H["gaps130"]["keys"][0] > 1 and min(np.diff(H["gaps130"]["keys"])) >= 2
    iso = H["isolated257"]
    assert len(iso["keys"]) == 257 and iso["keys"][256] >= 1000 and iso["counts"][256] == 2 and max(iso["keys"][:256]) == 256
    for c in g["subnormal"]:
        assert 2.0 ** -1064 < c["p"] < 2.0 ** -1022 and math.isfinite(c["ll"]) and c["h"] == 2
        assert all(b >= 0.0 for b in c["bound"]) and len(c["bound"]) == len(c["grad"])


def _clamp(case, point):
    bounds = [(0.01, None), (0, 0.5)] + ([(case.get("min_single_copy_ratio", 0.3), 1), (0, 1), (0, 1)] if case["model"] == "repeats" else [])
    return [lo if lo is not None and v < lo else hi if hi is not None and v > hi else v for v, (lo, hi) in zip(point, bounds)]
