"""The Hessian of a histogram batch without a device: the three entry points are exported, declared
and bound and refuse a missing batch with COVEST_E_INVALID; the Python argument rules refuse before the library is asked;
the packed triangle is unpacked bit-symmetric; the committed fixture is the shapes' and obeys the rule it was selected by;
and the host arithmetic of the second-order table (csrc/batch_host.h) runs in a program of its own under the address and
undefined-behaviour sanitizers.  Nothing loaded into Python runs under a sanitizer."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_hess_shapes as S
from conftest import REPO, load_golden

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")
_CROSS = r"covest_batch\s*\*\s*b\s*,\s*int64_t\s+n\s*,\s*const\s+double\s*\*\s*params\s*,\s*double\s*\*\s*out"
DECLARATIONS = {
    "covest_batch_eval_cross_hess": _CROSS,
    "covest_batch_eval_pairs_hess": r"covest_batch\s*\*\s*b\s*,\s*int64_t\s+n\s*,\s*const\s+int64_t\s*\*\s*hist_index\s*,\s*const\s+double\s*\*"
                                    r"\s*params\s*,\s*double\s*\*\s*out",
    "covest_batch_score_table2": _CROSS + r"_rows\s*,\s*double\s*\*\s*out_tail",
}


def test_the_entry_points_are_exported_declared_and_bound(hip_lib):
    from covest_amd import HistogramBatch, _capi, observed_information_batch
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "covest_amd.h")).read(), flags=re.S)
    for name, args in DECLARATIONS.items():
        assert name in _capi.EXPORTS
        assert hasattr(hip_lib, name), "libcovest_amd.so does not export %s" % name
        assert getattr(hip_lib, name).argtypes is not None, name
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert hip_lib.covest_abi_version() == 1
    assert re.search(r"#define\s+COVEST_ABI_VERSION\s+1\b", text)
    for method in ("loglikelihood_hessian_cross", "loglikelihood_hessian_pairs", "score_table"):
        assert callable(getattr(HistogramBatch, method))
    assert callable(observed_information_batch)


def test_a_missing_batch_is_invalid_without_a_device(hip_lib):
    from covest_amd import _capi
    buf = np.zeros(64)
    idx = np.zeros(1, dtype=np.int64)
    assert hip_lib.covest_batch_eval_cross_hess(None, 1, buf.ctypes.data, buf.ctypes.data) == _capi.COVEST_E_INVALID
    assert hip_lib.covest_batch_eval_pairs_hess(None, 1, idx.ctypes.data, buf.ctypes.data, buf.ctypes.data) == _capi.COVEST_E_INVALID
    assert hip_lib.covest_batch_score_table2(None, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == _capi.COVEST_E_INVALID
    assert hip_lib.covest_batch_eval_cross_hess(None, -1, None, None) == _capi.COVEST_E_INVALID


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
    from covest_amd import HistogramBatch, observed_information_batch
    batch = HistogramBatch.__new__(HistogramBatch)  # (no handle: whatever reaches the library fails the test)
    batch.model, batch._n, batch._n_keys, batch._handle = _NeverAsked(), 3, 3, None
    for index, points in (([0, 3], [[10.0, 0.05], [11.0, 0.05]]), ([-1], [[10.0, 0.05]]), ([0.5], [[10.0, 0.05]]),
                          ([math.nan], [[10.0, 0.05]]), ([0], [[10.0, 0.05], [11.0, 0.05]]), ([0, 1], [[10.0, 0.05]])):
        with pytest.raises(ValueError) as err:
            batch.loglikelihood_hessian_pairs(index, points)
        assert "closed" not in str(err.value)  # (the rule, not the missing handle)
    with pytest.raises(ValueError):
        batch.loglikelihood_hessian_cross([[10.0, 0.05, 0.5]])  # not a multiple of the parameter count
    with pytest.raises(ValueError, match="order"):
        batch.score_table([[10.0, 0.05]], order=3)
    with pytest.raises(ValueError, match="one estimate per histogram"):
        observed_information_batch(batch, [[10.0, 0.05]])
    with pytest.raises(ValueError, match="fix"):
        observed_information_batch(batch, [[10.0, 0.05]] * 3, fix=[None])
    for call in (lambda: batch.loglikelihood_hessian_cross([[10.0, 0.05]]), lambda: batch.score_table([[10.0, 0.05]], order=2),
                 lambda: batch.loglikelihood_hessian_pairs([0], [[10.0, 0.05]])):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_triangle_is_unpacked_symmetric():
    from covest_amd.batch import _unpack_hessian, pair_index
    for P in (2, 5):
        pairs = [(k, l) for k in range(P) for l in range(k, P)]
        assert [pair_index(P, k, l) for k, l in pairs] == list(range(P * (P + 1) // 2))
        packed = np.random.default_rng(P).standard_normal((3, 4, len(pairs)))
        packed[0, 0, 1] = math.nan
        H = _unpack_hessian(packed, P)
        assert H.shape == (3, 4, P, P)
        assert np.ascontiguousarray(H.swapaxes(-1, -2)).tobytes() == H.tobytes()
        for at, (k, l) in enumerate(pairs):
            assert np.array_equal(H[..., k, l], packed[..., at], equal_nan=True)
    assert S.rows_per_point("basic") == 6 and S.rows_per_point("repeats") == 21


def test_the_fixture_is_the_shapes_and_obeys_its_rule():
    g, grad = load_golden("batch_hess.json"), load_golden("batch_grad.json")
    assert list(g["shapes"]) == list(S.SHAPES) and list(S.SHAPES)[:len(S.S.SHAPES)] == list(S.S.SHAPES)
    size = os.path.getsize(os.path.join(HERE, "golden", "batch_hess.json"))
    assert size <= os.path.getsize(os.path.join(HERE, "golden", "kmer_hist.json")) and size < 1 << 20
    total = dropped = 0
    for name, rec in g["shapes"].items():
        case = S.shape(name)
        kind, n_keys, B, n, _ = S.SHAPES[name]
        P = 2 if kind == "basic" else 5
        NP = P * (P + 1) // 2
        assert (rec["model"], rec["n_keys"], rec["B"], rec["n"], rec["base"]) == (kind, n_keys, B, n, case["base"])
        assert np.array_equal(np.array(rec["points"]), case["points"]) and rec["row_sums"] == case["counts"].sum(axis=1).tolist()
        assert rec["tails"] == case["tails"].tolist() and rec["rows"] == S.stored_rows(name)
        # the stated subset: every row below B = 15; else at least the own row, the two zero rows, the first and last seeded
        named = set(case["rows"].values())
        if B < 15:
            assert rec["rows"] == list(range(B))
        else:
            seeded = [b for b in range(B) if b not in named]
            assert named <= set(rec["rows"]) and {seeded[0], seeded[-1]} <= set(rec["rows"])
        base = grad["shapes"][rec["base"]]  # ll and grad of the same (b, i) are pinned there
        assert base["points"][:n] == rec["points"] and base["tails"][:B] == rec["tails"] and base["moved"][:n] == rec["moved"]
        assert np.allclose(base["sp"][:n], rec["sp"], rtol=1e-14, atol=0) and np.allclose(base["D"][:n], rec["D"], rtol=1e-14, atol=0)
        total += len(rec["rows"]) * n
        dropped += len(rec["dropped"])
        assert len(rec["dropped"]) <= 0.05 * len(rec["rows"]) * n
        delta = g["k_tail"] * 2.0 ** -52 * n_keys
        gone = {(d[0], d[1]) for d in rec["dropped"]} | {tuple(s) for s in rec["special"]}
        for at, b in enumerate(rec["rows"]):
            tail = rec["tails"][b]
            for i in range(n):
                if (b, i) in gone:
                    assert [b, i] not in rec["special"] or rec["hess"][at][i] is None
                    continue
                sp, H, C = rec["sp"][i], rec["hess"][at][i], rec["C"][at][i]
                assert len(H) == len(C) == len(rec["D2"][i]) == NP and all(math.isfinite(v) for v in H)
                for k in range(P):
                    for l in range(k, P):
                        q = k * P - k * (k - 1) // 2 + (l - k)
                        assert abs(H[q]) <= C[q] * (1 + 1e-8)
                        if rec["moved"][i][k] or rec["moved"][i][l]:
                            assert H[q] == 0.0
                        elif tail and sp < 1:
                            assert abs(1 - sp) >= 1e-6
                            s_kl = tail * (rec["D2"][i][q] * delta / (1 - sp) ** 2 + 2 * rec["D"][i][k] * rec["D"][i][l] * delta / (1 - sp) ** 3)
                            assert s_kl <= 1e-9 * C[q] * (1 + 1e-8)
        if "zero_tail0" in case["rows"]:
            at = rec["rows"].index(case["rows"]["zero_tail0"])
            assert not np.array(rec["hess"][at]).any()
    assert (total, dropped) == (g["entries"], g["dropped"]) and dropped <= 0.05 * total
    # the new edge: 21 n rows of the repeat model one short of a wave's 64 and beyond it (n = 3, 4)
    assert (S.SHAPES["repeats-k65-B5-n3"][3], S.SHAPES["repeats-k65-B5-n4"][3]) == (3, 4) and 21 * 3 < 64 < 21 * 4
    # (the basic model's 6 n rows: n = 21 and 22 of the old shapes lie either side of the second wave's end, 126 < 128 < 132)
    assert {S.SHAPES[name][3] for name in S.SHAPES if name.startswith("basic")} >= {21, 22}


def test_the_host_arithmetic_under_sanitizers(tmp_path):
    cxx = next((shutil.which(n) for n in (os.environ.get("CXX"), "c++", "g++", "clang++") if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "batch_hess_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "batch_hess_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "batch_hess_host_check ok" in run.stdout, run.stdout + run.stderr
