"""The gradient of a histogram batch without a device: the three entry points are exported, declared
and bound; the Python argument rules refuse before the library is asked; refit="lockstep-gradient" refuses finite
differences; a lock-step round asks ONE request per live replicate and maps the batch's gradient into optimiser space
(on stand-ins for the model and the batch, in the manner of tests/test_gradient_cpu.py); the committed fixture is the
shapes' and obeys the rule it was selected by; and the chunk arithmetic of the gradient's table (csrc/batch_host.h) runs
in a program of its own under the address and undefined-behaviour sanitizers."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_grad_shapes as S
from conftest import REPO, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")
DECLARATIONS = {
    "covest_batch_eval_cross_grad": r"covest_batch\s*\*\s*b\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*\s*params\s*,\s*double\s*\*\s*out",
    "covest_batch_eval_pairs_grad": r"covest_batch\s*\*\s*b\s*,\s*int64_t\s+n\s*,\s*const\s+int64_t\s*\*\s*hist_index\s*,\s*const\s+double\s*\*"
                                    r"\s*params\s*,\s*double\s*\*\s*out",
    "covest_batch_score_table": r"covest_batch\s*\*\s*b\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*\s*params\s*,\s*double\s*\*\s*out_rows\s*,"
                                r"\s*double\s*\*\s*out_tail",
}


def test_the_entry_points_are_exported_declared_and_bound(hip_lib):
    from covest_amd import HistogramBatch, _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "covest_amd.h")).read(), flags=re.S)
    for name, args in DECLARATIONS.items():
        assert name in _capi.EXPORTS
        assert hasattr(hip_lib, name), "libcovest_amd.so does not export %s" % name
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert hip_lib.covest_abi_version() == 1
    for method in ("loglikelihood_gradient_cross", "loglikelihood_gradient_pairs", "score_table"):
        assert callable(getattr(HistogramBatch, method))


class _NeverAsked:
    """A model whose handle must not be asked for: the argument rules come first."""
    params = ("coverage", "error_rate")
    param_count = 2
    tail = 0
    hist = {1: 10, 2: 5, 3: 0}

    @property
    def handle(self):
        raise AssertionError("the library was asked before the arguments were checked")


def test_argument_rules_raise_before_the_library_is_asked():
    from covest_amd import HistogramBatch
    batch = HistogramBatch.__new__(HistogramBatch)  # (no handle: whatever reaches the library fails the test)
    batch.model, batch._n, batch._n_keys, batch._handle = _NeverAsked(), 3, 3, None
    for index, points in (([0, 3], [[10.0, 0.05], [11.0, 0.05]]), ([-1], [[10.0, 0.05]]), ([0.5], [[10.0, 0.05]]),
                          ([math.nan], [[10.0, 0.05]]), ([0], [[10.0, 0.05], [11.0, 0.05]]), ([0, 1], [[10.0, 0.05]])):
        with pytest.raises(ValueError) as err:
            batch.loglikelihood_gradient_pairs(index, points)
        assert "closed" not in str(err.value)  # (the rule, not the missing handle)
    with pytest.raises(ValueError):
        batch.loglikelihood_gradient_cross([[10.0, 0.05, 0.5]])  # not a multiple of the parameter count
    for call in (lambda: batch.loglikelihood_gradient_cross([[10.0, 0.05]]), lambda: batch.score_table([[10.0, 0.05]]),
                 lambda: batch.loglikelihood_gradient_pairs([0], [[10.0, 0.05]])):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_route_and_its_gradient_option():
    from covest_amd import parametric_bootstrap
    with pytest.raises(ValueError, match="gradient"):
        parametric_bootstrap(_NeverAsked(), [10.0, 0.05], replicates=2, refit="lockstep-gradient", gradient="fd")
    with pytest.raises(ValueError, match="lockstep-gradient"):  # (the old route's refusal names the new one)
        parametric_bootstrap(_NeverAsked(), [10.0, 0.05], replicates=2, refit="lockstep", gradient="analytic")
    with pytest.raises(ValueError, match="refit"):
        parametric_bootstrap(_NeverAsked(), [10.0, 0.05], replicates=2, refit="lockstep-hessian")


# ---------------------------------------------------------------------------------------------- the lock-step round
class _StubModel:
    bounds = ((0.01, None), (0, 0.5), (0.3, 1), (0, 1), (0, 1))
    params = ('coverage', 'error_rate', 'q1', 'q2', 'q')


class _RecordingBatch:
    """A batch whose replicate b has its optimum at coverage 10 + b: smooth, with its gradient in closed form.  It records
    every call."""

    def __init__(self, n):
        self.n = n
        self.gradient_calls = []  # per call: the list of replicates asked
        self.points = []          # per call: the model-space points
        self.value_calls = 0

    def _ll(self, b, p):
        c, e, q1, q2, q = p
        return -(1e6 * ((math.log(c) - math.log(10.0 + b)) ** 2 + 40 * (e - 0.03) ** 2 + (q1 - 0.9) ** 2 + 0.5 * (q2 - 0.4) ** 2
                        + (q - 0.2) ** 4) + 3.25e7)

    def loglikelihood_gradient_pairs(self, index, points):
        points = np.asarray(points, dtype=np.float64)
        self.gradient_calls.append([int(b) for b in index])
        self.points.append(points.copy())
        ll = np.array([self._ll(b, p) for b, p in zip(index, points)])
        grad = np.array([[-1e6 * 2 * (math.log(c) - math.log(10.0 + b)) / c, -1e6 * 80 * (e - 0.03), -1e6 * 2 * (q1 - 0.9),
                          -1e6 * (q2 - 0.4), -1e6 * 4 * (q - 0.2) ** 3] for b, (c, e, q1, q2, q) in zip(index, points)])
        return ll, grad

    def loglikelihood_pairs(self, index, points):
        self.value_calls += 1
        return np.array([self._ll(b, p) for b, p in zip(index, np.asarray(points, dtype=np.float64))])

    def close(self):
        raise AssertionError("a batch that was handed in stays the caller's")


def test_a_round_is_one_request_per_live_replicate():
    from covest_amd.bootstrap import _refit_lockstep
    B = 5
    batch = _RecordingBatch(B)
    start = [9.0, 0.04, 0.8, 0.5, 0.3]
    est, ok, ll = _refit_lockstep(_StubModel(), start, B, 0, 0, None, {}, analytic=True, batch=batch)
    assert ok.all() and est.shape == (B, 5)
    # (L-BFGS-B stops at a relative change of 2.2e-9 of an objective of 3.25e7, i.e. 0.07: 1e6 (d log c)^2 = 0.07 is
    # 2.7e-4 in log c, 4e-3 in c at 14; 4e7 (d e)^2 = 0.07 is 4e-5; 1e6 (d q1)^2 = 0.07 is 2.7e-4)
    for b in range(B):
        assert abs(est[b, 0] - (10.0 + b)) < 0.01 and abs(est[b, 1] - 0.03) < 1e-4 and abs(est[b, 2] - 0.9) < 1e-3
    # one request per live replicate a round -- not P + 1 --, each replicate at most once, in ascending order
    assert batch.gradient_calls[0] == list(range(B))
    for asked in batch.gradient_calls:
        assert asked == sorted(set(asked)) and 1 <= len(asked) <= B
    for later, earlier in zip(batch.gradient_calls[1:], batch.gradient_calls):
        assert set(later) <= set(earlier)  # a replicate that finished does not come back
    assert batch.value_calls == 1  # (the log-likelihoods at the estimates, once)
    assert np.array_equal(ll, batch.loglikelihood_pairs(np.arange(B), est))


def test_the_conversion_to_optimiser_space():
    """err_scale and fix, as CoverageEstimator.negll_gradient_points has them: the helper both use."""
    from covest_amd.bootstrap import _refit_lockstep
    from covest_amd.estimator import CoverageEstimator
    fix = [None, None, 0.7, None, 0.25]
    B = 3
    batch = _RecordingBatch(B)
    start = [9.0, 0.04, 0.5, 0.5, 0.5]
    est, ok, _ = _refit_lockstep(_StubModel(), start, B, 0, 0, fix, {"err_scale": 10}, analytic=True, batch=batch)
    assert ok.all()
    for pts in batch.points:  # what the batch is asked is in MODEL space: the fixed values, the error rate unscaled
        assert np.all(pts[:, 2] == 0.7) and np.all(pts[:, 4] == 0.25) and np.all(pts[:, 1] <= 0.5)
    assert np.array_equal(batch.points[0], np.repeat([[9.0, 0.04, 0.7, 0.5, 0.25]], B, axis=0))
    # (as on every route a fixed parameter's entry of the estimate is the start's: its component of the gradient is 0)
    assert np.all(est[:, 2] == start[2]) and np.all(est[:, 4] == start[4])
    for b in range(B):
        assert abs(est[b, 0] - (10.0 + b)) < 0.01 and abs(est[b, 1] - 0.03) < 1e-4 and abs(est[b, 3] - 0.4) < 1e-3
    e = CoverageEstimator(_StubModel(), err_scale=10, fix=fix, gradient="analytic")
    ll, grad = batch.loglikelihood_gradient_pairs([1], [[9.0, 0.04, 0.7, 0.5, 0.25]])
    rows = e._optimiser_rows(ll, grad)
    assert rows.shape == (1, 6) and rows[0, 0] == -ll[0]
    assert rows[0, 1] == -grad[0, 0] and rows[0, 2] == -grad[0, 1] / 10 and rows[0, 4] == -grad[0, 3]
    assert rows[0, 3] == 0.0 and rows[0, 5] == 0.0
    with pytest.raises(ValueError):  # the route's estimators are analytic ones: their refusals hold
        _refit_lockstep(_StubModel(), start, B, 0, 0, None, {"batched": False}, analytic=True, batch=batch)


# ---------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_is_the_shapes_and_obeys_its_rule():
    g = load_golden("batch_grad.json")
    assert list(g["shapes"]) == list(S.SHAPES)
    assert os.path.getsize(os.path.join(HERE, "golden", "batch_grad.json")) <= os.path.getsize(os.path.join(HERE, "golden", "deriv_shapes.json"))
    total = dropped = 0
    seen = {"basic": {"k": set(), "B": set(), "n": set()}, "repeats": {"k": set(), "B": set(), "n": set()}}
    for name, rec in g["shapes"].items():
        case = S.shape(name)
        kind, n_keys, B, n, _ = S.SHAPES[name]
        P = 2 if kind == "basic" else 5
        assert (rec["model"], rec["n_keys"], rec["B"], rec["n"]) == (kind, n_keys, B, n)
        assert np.array_equal(np.array(rec["points"]), case["points"]) and rec["row_sums"] == case["counts"].sum(axis=1).tolist()
        assert rec["tails"] == case["tails"].tolist()
        if not case["dead"]:
            for axis, v in (("k", n_keys), ("B", B), ("n", n)):
                seen[kind][axis].add(v)
        total += B * n
        dropped += len(rec["dropped"])
        assert len(rec["dropped"]) <= 0.05 * B * n
        delta = g["k_tail"] * 2.0 ** -52 * n_keys
        gone = {(d[0], d[1]) for d in rec["dropped"]} | {tuple(s) for s in rec["special"]}
        for b in range(B):
            tail = rec["tails"][b]
            for i in range(n):
                if (b, i) in gone:
                    continue
                sp = rec["sp"][i]
                assert math.isfinite(rec["ll"][b][i]) and len(rec["grad"][b][i]) == len(rec["Cg"][b][i]) == len(rec["D"][i]) == P
                for k in range(P):
                    assert abs(rec["grad"][b][i][k]) <= rec["Cg"][b][i][k] * (1 + 1e-8)
                    if rec["moved"][i][k]:
                        assert rec["grad"][b][i][k] == 0.0
                    elif tail and sp < 1:
                        assert abs(1 - sp) >= 1e-6
                        assert 1e-9 * rec["Cg"][b][i][k] * (1 + 1e-8) >= tail * rec["D"][i][k] * delta / (1 - sp) ** 2
        if "zero_tail0" in case["rows"]:
            b = case["rows"]["zero_tail0"]
            assert not np.array(rec["ll"][b]).any() and not np.array(rec["grad"][b]).any()
    assert (total, dropped) == (g["entries"], g["dropped"]) and dropped <= 0.05 * total
    for kind, rows in (("basic", {1, 21, 22}), ("repeats", {1, 10, 11})):
        assert seen[kind]["k"] == {1, 63, 65, 255, 256, 257} and seen[kind]["B"] >= {1, 15, 17, 65} and seen[kind]["n"] == rows
    lot = g["shapes"]["repeats-k65-B5-n10-lot"]
    assert [t - 1 for t in lot["T"][:len(S.LOT_TM1)]] == list(S.LOT_TM1)


def test_the_chunk_arithmetic_under_sanitizers(tmp_path):
    cxx = next((shutil.which(n) for n in (os.environ.get("CXX"), "c++", "g++", "clang++") if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "batch_grad_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "batch_grad_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "batch_grad_host_check ok" in run.stdout, run.stdout + run.stderr
