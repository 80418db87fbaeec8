"""The truncated-Poisson entry points (covest_truncated_poisson, covest_truncated_poisson_table, covest_amd.poisson)
as far as a machine without a GPU can see them: the symbols, the log-domain fixture tests/golden/tp_log.json against
its generator's conditions, and the argument checks, which come before any device call."""
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden

NEW = ("covest_truncated_poisson", "covest_truncated_poisson_table")
EPS = 2.0 ** -52
TINY = 2.2250738585072014e-308  # the smallest normal double


def test_header_binding_and_library_have_the_two_symbols(hip_lib):
    from covest_amd import _capi
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(covest_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.covest_abi_version() == 1
    import covest_amd
    assert covest_amd.poisson.truncated_poisson is covest_amd.truncated_poisson


def _residual(l):
    n = 0
    while l > 200.0:
        l -= 200.0
        n += 1
    return n, l


def test_tp_log_fixture_meets_its_generators_conditions():
    """Every (l, j) of tp_table.json, of tp_bitwise.json's edges with l > 0 and of its +inf rows is there unless l lies
    just above a multiple of 200 (l / l_res > 1e5); those are at most 5 % of the cases; every value is finite; and exp of
    a value gives the reference's finite normal value back.  The generator asserts 1e-15 at 50 digits; a double can
    confirm it only up to what the stored value's own rounding (eps |v| / 2) and libm's exp (an ulp) add:
    1e-15 + eps (|v| + 2)."""
    g = load_golden("tp_log.json")
    table, bitwise = load_golden("tp_table.json"), load_golden("tp_bitwise.json")
    cases = [tuple(r) for r in table["rows"]] + [tuple(r) for r in bitwise["edges"] if r[0] > 0]
    cases += [tuple(r) for r in bitwise["rows"] if r[2] == math.inf]
    cases = list({(l, j): (l, j, ref) for l, j, ref in reversed(cases)}.values())  # (a pair two sources hold: one case)
    have = {(r[0], r[1]): r[2] for r in g["rows"]}
    assert len(have) == len(g["rows"]) and g["cases"] == len(cases) and g["digits"] == 50
    n_skipped = 0
    for l, j, ref in cases:
        n, res = _residual(l)
        if n > 0 and l / res > g["skip_ratio"]:
            n_skipped += 1
            assert (l, j) not in have
            continue
        v = have[(l, j)]
        assert math.isfinite(v), (l, j)
        if math.isfinite(ref) and ref >= TINY:
            assert abs(math.exp(v) / ref - 1.0) <= 1e-15 + EPS * (abs(v) + 2.0), (l, j, v, ref)
        elif ref == 0.0:
            assert v < -745.13, (l, j, v)  # at most half a grid step of the doubles: ln 2^-1075 = -745.133
    assert n_skipped == g["skipped"] == len(cases) - len(g["rows"])
    assert n_skipped <= 0.05 * len(cases)
    assert sum(1 for r in cases if r[2] == math.inf) == 5


def test_raises_without_a_device(hip_lib):
    from covest_amd import _capi, poisson
    if hip_lib.covest_device_count() > 0:
        pytest.skip("a HIP device is present")
    for call in (lambda: poisson.truncated_poisson(3.0, 2),
                 lambda: poisson.truncated_poisson_many([1.0, 2.0], [1, 2], "log"),
                 lambda: poisson.truncated_poisson_table([1.0, 2.0], [1, 2, 3])):
        with pytest.raises(_capi.CovestHipError) as e:
            call()
        assert "(-2)" in str(e.value), str(e.value)  # COVEST_E_NO_DEVICE: never computed elsewhere


def test_invalid_arguments_are_refused_before_any_device_call(hip_lib):
    """COVEST_E_INVALID (-1) whether or not there is a device: on a machine without one a call that reached the
    device would answer COVEST_E_NO_DEVICE (-2) instead.  And a call with nothing to do returns without one."""
    import ctypes
    from covest_amd import _capi, poisson

    def refused(call):
        with pytest.raises(_capi.CovestHipError) as e:
            call()
        assert "(-1)" in str(e.value), str(e.value)

    refused(lambda: poisson.truncated_poisson(3.0, 0))
    refused(lambda: poisson.truncated_poisson_many([1.0, 2.0], [3, -1]))
    refused(lambda: poisson.truncated_poisson_many([1.0], [(1 << 22) + 1]))
    refused(lambda: poisson.truncated_poisson_table([1.0], [2, 2]))
    refused(lambda: poisson.truncated_poisson_table([1.0], [3, 2]))
    refused(lambda: poisson.truncated_poisson_table([1.0], [0, 1]))
    refused(lambda: poisson.truncated_poisson_table([1.0], [16384, 16385]))
    one, key, out = np.ones(1), np.ones(1, dtype=np.int64), np.empty(1)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    for mode in (-1, 3):
        assert hip_lib.covest_truncated_poisson(-1, 1, one.ctypes.data_as(dp), key.ctypes.data_as(ip), mode,
                                                out.ctypes.data_as(dp)) == -1
    assert hip_lib.covest_truncated_poisson(-1, -1, None, None, 0, None) == -1
    assert hip_lib.covest_truncated_poisson(-1, 1, None, key.ctypes.data_as(ip), 0, out.ctypes.data_as(dp)) == -1
    with pytest.raises(ValueError):
        poisson.truncated_poisson_many([1.0], [1], mode="exact")
    with pytest.raises(ValueError):
        poisson.truncated_poisson_many([1.0], [1.5])
    assert poisson.truncated_poisson_many([], []).shape == (0,)
    assert poisson.truncated_poisson_table([], [1, 2]).shape == (0, 2)
    assert poisson.truncated_poisson_table([1.0], []).shape == (1, 0)
