"""The parametric bootstrap without a device: the thresholds of a draw against the numpy
restatement (tests/draw_reference.py) bit for bit, the refusals, the bookkeeping of model_cells, the summary arithmetic
of parametric_bootstrap over a stubbed refit, the record of print_output, and the host code behind abi_draw.cpp
(csrc/draw_host.h) in a program of its own under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import draw_reference as ref
from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")
TOP = 1 << 63


def _shapes():
    rng = np.random.default_rng(20240613)
    big = rng.random(10001)
    big[rng.random(10001) < 0.1] = 0.0
    big[0] = 1.0
    spread = np.array([1e-300, 1e-200, 1e-100, 1e-18, 1.0, 5e-324])
    total_37 = rng.random(50)
    total_37 *= 3.7 / total_37.sum()
    total_tiny = rng.random(50)
    total_tiny *= 1e-12 / total_tiny.sum()
    return {"m1": [0.25], "one_zero": [1, 0], "zero_one": [0, 1], "middle": [0, 0, 5, 0, 0], "spread": spread,
            "denormals": [5e-324, 5e-324, 1e-323], "big": big, "total_3.7": total_37, "total_1e-12": total_tiny}


@pytest.mark.parametrize("name", sorted(_shapes()))
def test_thresholds_equal_the_restatement_bit_for_bit(hip_lib, name):
    from covest_amd import draw_thresholds
    w = np.asarray(_shapes()[name], dtype=np.float64)
    got, want = draw_thresholds(w), ref.thresholds(w)
    assert got.dtype == np.uint64 and got.shape == w.shape
    assert np.array_equal(got, want)
    t = [int(v) for v in got]
    assert all(a <= b for a, b in zip(t, t[1:])) and t[-1] == TOP
    for i, v in enumerate(w):
        if v == 0.0:
            assert t[i] == (t[i - 1] if i else 0)


def test_kernel_constants_agree_with_the_python_side():
    from covest_amd import bootstrap
    text = open(os.path.join(CSRC, "kernels.h")).read()

    def const(name):
        return eval(re.search(r"constexpr (?:int|long long) %s = ([^;]+);" % name, text).group(1))

    assert const("kDrawMaxCells") == bootstrap.MAX_CELLS
    assert const("kDrawLdsBothCells") == bootstrap.LDS_BOTH_CELLS
    assert const("kDrawLdsThrCells") == bootstrap.LDS_THRESHOLD_CELLS
    assert 1 << const("kDrawGuideBits") == bootstrap.GUIDE_SIZE
    assert const("kDrawChunk") == bootstrap.CHUNK_DRAWS
    header = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    assert "#define COVEST_DRAW_MAX_CELLS %d" % bootstrap.MAX_CELLS in header


def test_every_refusal_comes_before_the_library(monkeypatch):
    from covest_amd import _capi, bootstrap

    def no_library():
        raise AssertionError("the library was asked")

    monkeypatch.setattr(_capi, "lib", no_library)
    nan, inf = float("nan"), float("inf")
    for bad in ([1.0, -1e-300], [nan, 1.0], [1.0, inf], [0.0, 0.0, 0.0], [1.7e308, 1.7e308], [], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            bootstrap.draw_thresholds(bad)
        with pytest.raises(ValueError):
            bootstrap.draw_histograms(bad, 10, 1)
    ok = [1.0, 2.0]
    for kwargs in (dict(n_draws=-1, replicates=1), dict(n_draws=1, replicates=-1), dict(n_draws=1.5, replicates=1),
                   dict(n_draws=1, replicates=1, first_replicate=-1), dict(n_draws=1, replicates=1, first_replicate=1 << 32),
                   dict(n_draws=1, replicates=2, first_replicate=(1 << 32) - 1), dict(n_draws=1, replicates=1, seed=1 << 64),
                   dict(n_draws=1, replicates=1, seed=-1)):
        with pytest.raises(ValueError):
            bootstrap.draw_histograms(ok, **kwargs)
        with pytest.raises(ValueError):
            bootstrap.draw_histograms_device(1, 2, kwargs["n_draws"], kwargs["replicates"], 1,
                                             **{k: v for k, v in kwargs.items() if k in ("seed", "first_replicate")})
    with pytest.raises(ValueError):
        bootstrap.draw_histograms(np.ones(bootstrap.MAX_CELLS + 1), 1, 1)
    with pytest.raises(ValueError):
        bootstrap.draw_histograms_device(1, 0, 1, 1, 1)
    with pytest.raises(AssertionError):  # ... and what passes them does ask
        bootstrap.draw_histograms(ok, 1, 1, first_replicate=(1 << 32) - 1)


def test_the_library_refuses_what_python_refuses(hip_lib):
    """The C entry points' own refusals (no device is asked for: this machine may have none)."""
    import ctypes
    from covest_amd import _capi
    out = np.zeros(8, dtype=np.int64)
    thr = np.zeros(4, dtype=np.uint64)

    def host(w, n, first, reps, m=None):
        w = np.asarray(w, dtype=np.float64)
        return hip_lib.covest_draw_histograms(-1, len(w) if m is None else m, w.ctypes.data, n, first, reps, 0, out.ctypes.data)

    nan, inf = float("nan"), float("inf")
    for w in ([1.0, -1.0], [nan, 1.0], [1.0, inf], [0.0, 0.0], [1.7e308, 1.7e308]):
        assert host(w, 1, 0, 1) == _capi.COVEST_E_INVALID
        w = np.asarray(w)
        assert hip_lib.covest_draw_thresholds(len(w), w.ctypes.data, thr.ctypes.data) == _capi.COVEST_E_INVALID
    good = [1.0, 1.0]
    assert host(good, 1, 0, 1, m=0) == _capi.COVEST_E_INVALID
    assert host(good, -1, 0, 1) == _capi.COVEST_E_INVALID
    assert host(good, 1, 0, -1) == _capi.COVEST_E_INVALID
    assert host(good, 1, 1 << 32, 1) == _capi.COVEST_E_INVALID
    assert host(good, 1, (1 << 32) - 1, 2) == _capi.COVEST_E_INVALID
    assert b"replicate index" in hip_lib.covest_last_error()
    dev = hip_lib.covest_draw_histograms_device
    assert dev(-1, 0, 1, 1, 0, 1, 0, 1, None) == _capi.COVEST_E_INVALID
    assert dev(-1, 2, 1, -1, 0, 1, 0, 1, None) == _capi.COVEST_E_INVALID
    assert dev(-1, 2, 1, 1, 0, -1, 0, 1, None) == _capi.COVEST_E_INVALID
    assert dev(-1, 2, 1, 1, 1 << 32, 1, 0, 1, None) == _capi.COVEST_E_INVALID
    assert dev(-1, 65537, 1, 1, 0, 1, 0, 1, None) == _capi.COVEST_E_INVALID
    # nothing to do, or nothing to draw: fine without a device
    out[:] = 7
    assert host(good, 5, 0, 0) == 0 and out[0] == 7
    assert dev(-1, 2, None, 5, 3, 0, 0, None, None) == 0
    assert host(good, 0, (1 << 32) - 2, 2) == 0 and not out[:4].any() and out[4] == 7
    assert ctypes.c_int(hip_lib.covest_draw_thresholds(0, thr.ctypes.data, thr.ctypes.data)).value == _capi.COVEST_E_INVALID


class _StubModel:
    """What model_cells and parametric_bootstrap touch of a model, with made-up probabilities."""
    params = ("coverage", "error_rate")
    bounds = ((0.01, 50), (0, 0.5))
    k, r, max_error, device = 21, 100, 8, -1

    def __init__(self, hist, tail):
        self.hist, self.tail, self.seen = hist, tail, None

    def fit_to_bounds(self, args):
        return [min(max(a, lo), hi) for a, (lo, hi) in zip(args, self.bounds)]

    def compute_probabilities(self, *args):
        self.seen = list(args)
        return {j: 0.5 ** (at + 2) for at, j in enumerate(sorted(self.hist))}  # (another order than the histogram's)

    def correct_c(self, c):
        return c * (self.r - self.k + 1) / self.r


def test_model_cells_bookkeeping():
    from covest_amd import model_cells
    hist = {7: 3, 2: 10, 5: 0}
    m = _StubModel(hist, 0)
    keys, w, has_tail = model_cells(m, [80.0, -1.0])
    assert m.seen == [50, 0]  # after fit_to_bounds
    assert keys.tolist() == [7, 2, 5] and not has_tail  # the histogram's order, zero counts kept, no tail cell
    assert w.tolist() == [0.5 ** 4, 0.5 ** 2, 0.5 ** 3]
    keys, w, has_tail = model_cells(_StubModel(hist, 4), [10.0, 0.1])
    assert has_tail and keys.tolist() == [7, 2, 5] and len(w) == 4
    assert w[3] == 1.0 - (0.5 ** 4 + 0.5 ** 2 + 0.5 ** 3)


def test_summary_arithmetic_over_a_stubbed_refit(monkeypatch):
    from covest_amd import bootstrap
    hist = {1: 40, 2: 50, 3: 10}
    model = _StubModel(hist, 0)
    rows = np.array([[10.0, 0.05], [12.0, 0.0], [11.0, 0.07], [50.0, 0.5], [9.0, 0.06]])
    ok = [True, True, True, False, True]
    seen = {}

    def draws(weights, n_draws, replicates, seed=0, first_replicate=0, device=-1):
        seen.update(n=n_draws, reps=replicates, seed=seed, m=len(weights))
        return np.tile(np.array([[30, 60, 10]], dtype=np.int64), (replicates, 1))

    def refit(m, keys, counts, tail, estimate, fix, options):
        b = seen.setdefault("calls", 0)
        seen["calls"] = b + 1
        assert keys.tolist() == [1, 2, 3] and counts.tolist() == [30, 60, 10] and tail == 0 and options == {"gradient": "analytic"}
        return list(rows[b]), ok[b], -100.0 - b

    monkeypatch.setattr(bootstrap, "draw_histograms", draws)
    monkeypatch.setattr(bootstrap, "_refit", refit)
    out = bootstrap.parametric_bootstrap(model, [10.5, 0.04], replicates=5, seed=9, level=0.5, hist_orig={1: 100, 2: 450},
                                         sample_factor=2, gradient="analytic")
    assert seen["n"] == 100 and seen["reps"] == 5 and seen["seed"] == 9 and seen["m"] == 3
    assert out["replicates"] == 5 and out["seed"] == 9 and out["n_draws"] == 100 and out["failed"] == 1
    assert np.array_equal(out["estimates"], rows) and out["success"].tolist() == ok
    assert out["loglikelihood"].tolist() == [-100.0, -101.0, -102.0, -103.0, -104.0]
    assert out["at_bound"].tolist() == [[False, False], [False, True], [False, False], [True, True], [False, False]]
    good = rows[[0, 1, 2, 4]]  # the failed replicate is left out
    assert out["mean"] == {"coverage": 10.5, "error_rate": pytest.approx(0.045)}
    assert out["bias"]["coverage"] == 0.0 and out["bias"]["error_rate"] == pytest.approx(0.005)
    assert out["standard_errors"]["coverage"] == pytest.approx(np.sqrt(5.0 / 3.0))
    assert out["standard_errors"]["error_rate"] == pytest.approx(good[:, 1].std(ddof=1))
    assert out["percentile_intervals"]["coverage"] == pytest.approx([9.75, 11.25])  # quartiles of 9, 10, 11, 12
    sizes = 1000.0 / (good[:, 0] * 2 * 0.8)
    assert out["genome_size"]["mean"] == pytest.approx(sizes.mean())
    assert out["genome_size"]["standard_error"] == pytest.approx(sizes.std(ddof=1))
    assert out["genome_size"]["interval"] == pytest.approx(list(np.percentile(sizes, [25, 75])))
    # a fixed parameter
    seen.pop("calls")
    fixed = bootstrap.parametric_bootstrap(model, [10.5, 0.04], replicates=5, fix=[None, 0.04], gradient="analytic")
    for key in ("mean", "bias", "standard_errors", "percentile_intervals"):
        assert fixed[key]["error_rate"] is None and fixed[key]["coverage"] is not None
    assert "genome_size" not in fixed
    # with a tail: its cell is the last column, and it is the replicate's tail
    tailed = _StubModel(hist, 7)
    monkeypatch.setattr(bootstrap, "draw_histograms", lambda w, n, reps, **kw: np.tile(np.array([[1, 2, 3, 4]]), (reps, 1)))
    monkeypatch.setattr(bootstrap, "_refit", lambda m, keys, counts, tail, *a: (
        [10.0, 0.1], counts.tolist() == [1, 2, 3] and tail == 4, 0.0))
    assert bootstrap.parametric_bootstrap(tailed, [10.0, 0.1], replicates=2)["failed"] == 0


# print_output(hist, model, True, 2, estimated=(10.0, 0.05), guess=(9.0, 0.04), orig=(10.0, None), reads_size=50000,
# silent=True, orig_sample_factor=3) of the parent commit, the likelihood stubbed as below
_PARENT_RECORD = {
    'model': 'basic', 'hist_size': 3, 'sample_factor': 2, 'orig_sample_factor': 3, 'success': True, 'version': '0.1.0',
    'starting_points': 1, 'use_grid_search': False, 'guessed_coverage': 18.0, 'guessed_error_rate': 0.04,
    'guessed_loglikelihood': -9.04, 'coverage': 20.0, 'error_rate': 0.05, 'orig_coverage': 60.0,
    'loglikelihood': -10.05, 'genome_size': 62, 'genome_size_reads': 833, 'provided_coverage': 20.0,
    'provided_loglikelihood': -10.05,
}


def test_print_output_without_and_with_a_bootstrap(monkeypatch):
    from covest_amd import BasicModel, print_output
    hist = {1: 100, 2: 450}
    model = BasicModel(21, 100, {1: 10, 2: 5, 3: 1}, 0, max_error=8)
    monkeypatch.setattr(model, "compute_loglikelihood", lambda c, e: -(c + e))
    args = dict(estimated=(10.0, 0.05), guess=(9.0, 0.04), orig=(10.0, None), reads_size=50000, silent=True,
                orig_sample_factor=3)
    plain = print_output(hist, model, True, 2, **args)
    assert plain == _PARENT_RECORD and list(plain) == list(_PARENT_RECORD)
    boot = {"replicates": 16, "failed": 1,
            "bias": {"coverage": 0.25, "error_rate": None}, "standard_errors": {"coverage": 0.5, "error_rate": None},
            "percentile_intervals": {"coverage": [9.0, 11.0], "error_rate": None},
            "genome_size": {"mean": 60.0, "standard_error": 2.0, "interval": [55.0, 65.0]}}
    record = print_output(hist, model, True, 2, bootstrap=boot, **args)
    added = {k: v for k, v in record.items() if k not in plain}
    assert {k: record[k] for k in plain} == plain
    assert added == {"bootstrap_replicates": 16, "bootstrap_failed": 1, "bootstrap_bias_coverage": 0.5,
                     "bootstrap_se_coverage": 1.0, "bootstrap_interval_coverage": [18.0, 22.0],
                     "bootstrap_interval_genome_size": [55.0, 65.0]}


def test_host_code_of_the_draw_entry_points_under_sanitizers(tmp_path):
    cxx = next((shutil.which(n) for n in (os.environ.get("CXX"), "c++", "g++", "clang++") if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "draw_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "draw_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "draw_host_check ok" in run.stdout, run.stdout + run.stderr
