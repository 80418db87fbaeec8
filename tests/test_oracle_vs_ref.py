"""The oracle's truncated_poisson must agree bit for bit with the reference's own C extension: with the values
that extension returned, stored in tests/golden/tp_bitwise.json (make_golden.py section tpbits), and -- where the
extension itself has been built into oracle/_ref -- with the extension as well."""
import glob
import importlib.util
import math
import os
import random

from conftest import REPO, load_golden


def _load_ref():
    hits = glob.glob(os.path.join(REPO, "oracle", "_ref", "covest_poisson*.so"))
    if not hits:
        return None
    spec = importlib.util.spec_from_file_location("covest_poisson", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_truncated_poisson_bitwise(oracle):
    fix = load_golden("tp_bitwise.json")
    ref = _load_ref()
    rnd = random.Random(11)
    assert len(fix["rows"]) == 3000
    for l, j, want in fix["rows"]:
        assert (l, j) == (math.exp(rnd.uniform(math.log(1e-10), math.log(2e4))),
                          int(math.exp(rnd.uniform(0, math.log(12000)))))
        a = oracle.truncated_poisson(l, j)
        assert a == want or (a != a and want != want), (l, j, a, want)
        if ref is not None:
            b = ref.truncated_poisson(l, j)
            assert a == b or (a != a and b != b), (l, j, a, b)
    edges = [(l, j) for l in (199.99999999, 200.0, 200.00000001, 400.0, 400.000000001, 1e-8, 1.0000001e-8)
             for j in (1, 5, 300)]
    assert [(l, j) for l, j, _ in fix["edges"]] == edges
    for l, j, want in fix["edges"]:
        assert oracle.truncated_poisson(l, j) == want
        if ref is not None:
            assert oracle.truncated_poisson(l, j) == ref.truncated_poisson(l, j)
