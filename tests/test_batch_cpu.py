"""Histogram batches without a device: the new entry points are exported, the Python argument
rules refuse before the library is asked, the lock-step bootstrap refuses an analytic gradient, nothing computes without
a device, and the host code behind abi_batch.cpp (csrc/batch_host.h: argument rules, the chunking of a point list
against the table budget, the cut of launches, the exactly rounded sum of the tail cell) runs in a program of its own
under the address and undefined-behaviour sanitizers."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")
BATCH_SYMBOLS = ("covest_batch_create", "covest_batch_draw", "covest_batch_counts", "covest_batch_eval_cross",
                 "covest_batch_eval_pairs", "covest_batch_argmin_cross", "covest_batch_info", "covest_batch_destroy")


class _NeverAsked:
    """A model whose handle must not be asked for: the argument rules come first."""
    params = ("coverage", "error_rate")
    param_count = 2
    tail = 0
    hist = {1: 10, 2: 5, 3: 0}

    @property
    def handle(self):
        raise AssertionError("the library was asked before the arguments were checked")


def test_the_batch_symbols_are_exported(hip_lib):
    from covest_amd import _capi
    for name in BATCH_SYMBOLS:
        assert name in _capi.EXPORTS
        assert hasattr(hip_lib, name), "libcovest_amd.so does not export %s" % name
    import covest_amd
    assert covest_amd.HistogramBatch is covest_amd.batch.HistogramBatch


def test_kernel_constants_agree_with_the_host_header_and_python():
    from covest_amd import batch
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    host = open(os.path.join(CSRC, "batch_host.h")).read()

    def const(text, name):
        return eval(re.search(r"constexpr int64_t %s = ([^;]+);" % name, text).group(1).replace("(int64_t)", ""))

    assert const(kernels, "kBatchTableBytes") == const(host, "kBatchHostTableBytes") == 256 << 20
    assert const(kernels, "kBatchMaxHist") == const(host, "kBatchHostMaxHist") == batch.MAX_HISTOGRAMS
    assert const(host, "kBatchHostMaxBlocks") == 1 << 23


@pytest.mark.parametrize("counts, tails", [
    (np.zeros((2, 4)), None),                    # a column too many
    (np.zeros((2, 2)), None),                    # one too few
    (np.zeros((2, 3, 1)), None),                 # not a matrix
    (np.zeros(5), None),                         # a vector that is no single histogram
    ([[1.0, -1.0, 0.0]], None),                  # a negative count
    ([[1.0, math.nan, 0.0]], None),
    ([[1.0, math.inf, 0.0]], None),
    (np.zeros((2, 3)), [0.0]),                   # tails: one per histogram
    (np.zeros((2, 3)), [0.0, -1.0]),
    (np.zeros((2, 3)), [0.0, math.nan]),
    (np.zeros((2, 3)), [math.inf, 0.0]),
])
def test_constructor_rules_raise_before_the_library_is_asked(counts, tails):
    from covest_amd import HistogramBatch
    with pytest.raises(ValueError):
        HistogramBatch(_NeverAsked(), counts, tails)


def test_draw_rules_raise_before_the_library_is_asked():
    from covest_amd import HistogramBatch
    for kwargs in (dict(replicates=-1), dict(replicates=1, seed=-1), dict(replicates=1, seed=1 << 64),
                   dict(replicates=1, first_replicate=1 << 32), dict(replicates=1, n_draws=-5),
                   dict(replicates=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            HistogramBatch.draw(_NeverAsked(), [10.0, 0.05], **kwargs)
    with pytest.raises(ValueError):
        HistogramBatch.draw(_NeverAsked(), [10.0, 0.05, 0.5], replicates=1)  # a parameter too many


def test_index_and_point_rules_raise_before_the_library_is_asked():
    from covest_amd import HistogramBatch
    from covest_amd.batch import _index_array
    assert _index_array([2, 0, 2], 3).tolist() == [2, 0, 2] and _index_array([], 0).size == 0
    for index, n_hist in (([3], 3), ([-1], 3), ([0], 0), ([0.5], 3), ([math.nan], 3)):
        with pytest.raises(ValueError):
            _index_array(index, n_hist)
    batch = HistogramBatch.__new__(HistogramBatch)  # (no handle: whatever reaches the library fails the test)
    batch.model, batch._n, batch._n_keys, batch._handle = _NeverAsked(), 3, 3, None
    with pytest.raises(ValueError):
        batch.loglikelihood_pairs([0, 3], [[10.0, 0.05], [11.0, 0.05]])
    with pytest.raises(ValueError):
        batch.loglikelihood_pairs([0], [[10.0, 0.05], [11.0, 0.05]])  # one index per point
    with pytest.raises(ValueError):
        batch.loglikelihood_cross([[10.0, 0.05]])  # closed
    assert len(batch) == 3
    batch.close()
    batch.close()


def test_lockstep_refuses_an_analytic_gradient_and_unknown_routes():
    from covest_amd import parametric_bootstrap
    with pytest.raises(ValueError, match="gradient"):
        parametric_bootstrap(_NeverAsked(), [10.0, 0.05], replicates=2, refit="lockstep", gradient="analytic")
    with pytest.raises(ValueError, match="refit"):
        parametric_bootstrap(_NeverAsked(), [10.0, 0.05], replicates=2, refit="together")


def test_a_batch_fails_loudly_without_a_device(hip_lib):
    """No CPU path: without a device the constructor raises; with one, the same call gives a batch."""
    from covest_amd import BasicModel, HistogramBatch, _capi
    model = BasicModel(21, 100, {1: 10, 2: 5, 3: 0}, 0, max_error=8)
    counts = [[10.0, 5.0, 0.0], [0.0, 0.0, 0.0]]
    if hip_lib.covest_device_count() > 0:
        batch = HistogramBatch(model, counts)
        assert len(batch) == 2
        batch.close()
    else:
        with pytest.raises(_capi.CovestHipError):
            HistogramBatch(model, counts)
        with pytest.raises(_capi.CovestHipError):
            HistogramBatch.draw(model, [10.0, 0.05], replicates=2)
    model.close()


def test_host_code_of_the_batch_entry_points_under_sanitizers(tmp_path):
    cxx = next((shutil.which(n) for n in (os.environ.get("CXX"), "c++", "g++", "clang++") if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "batch_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "batch_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "batch_host_check ok" in run.stdout, run.stdout + run.stderr
