"""Posterior classes without a GPU: the yardstick against the CPU oracle, the fixture's invariants, and the numpy side
(PosteriorClasses, print_output) on hand-made arrays.  No number here comes from the device code."""
import math

import numpy as np
import pytest

from conftest import load_golden
import posterior_reference as ref
from covest_amd import BasicModel, RepeatsModel, print_output
from covest_amd.posterior import PosteriorClasses, posterior_classes

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return load_golden("posterior.json")


def _case(golden, name):
    return next(c for c in golden["cases"] if c["name"] == name)


@pytest.mark.parametrize("name", ["basic_s8", "rep_t9"])
def test_restatement_reproduces_the_oracle(oracle, golden, name):
    """exp(ln p_j) of the 50-digit restatement against the oracle's compute_probabilities, 1e-12 relative wherever that
    value is a normal double: recomputed here, and the stored numbers are the recomputed ones."""
    cs = _case(golden, name)
    got, _ = ref.compute_case(cs)
    assert got["T"] == cs["T"]
    m = oracle.OracleModel(cs["kind"], cs["k"], cs["r"], {int(j): 1 for j in cs["keys"]}, 0, max_error=cs["max_error"],
                           threshold=cs["threshold"])
    want = m.compute_probabilities(*cs["point"])
    checked = 0
    for j in cs["eval_keys"]:
        row = got["rows"][str(j)]
        assert row == cs["rows"][str(j)]
        if math.isfinite(want[j]) and want[j] >= ref.TINY:
            assert abs(math.exp(row["ln_p"]) / want[j] - 1) <= 1e-12, (name, j)
            checked += 1
    assert checked == len(cs["eval_keys"])


def test_fixture_invariants(golden):
    assert golden["skipped"] <= 0.05 * golden["candidates"]
    assert len(golden["cases"]) + golden["skipped"] == golden["candidates"]
    by_name = {c["name"]: c for c in golden["cases"]}
    kinds = {c["kind"] for c in golden["cases"]}
    assert kinds == {"basic", "repeats"}
    for c in golden["cases"]:
        T, S, Cc = c["T"], min(c["k"] + 1, c["max_error"]), c["copy_columns"]
        assert len(c["eval_keys"]) <= 12
        for j in c["eval_keys"]:
            row = c["rows"][str(j)]
            assert len(row["E"]) == S and len(row["C"]) == Cc
            assert abs(sum(row["E"]) - 1) <= 4 * EPS * S, (c["name"], j)
            assert abs(sum(row["C"]) - 1) <= 4 * EPS * Cc, (c["name"], j)
            assert all(v == 0.0 for v in row["C"][T - 1:]), (c["name"], j)  # columns beyond T - 1
            assert 1 - 4 * EPS <= row["M"] <= (T - 1) * (1 + 4 * EPS)
        if "wide_of" in c:  # the lumped column of the narrow case = the sum of the wide case's columns from there on
            narrow = by_name[c["wide_of"]]
            n_cc = narrow["copy_columns"]
            assert n_cc < Cc and narrow["point"] == c["point"] and narrow["keys"] == c["keys"]
            for j in c["eval_keys"]:
                w, n = c["rows"][str(j)], narrow["rows"][str(j)]
                assert n["C"][:n_cc - 1] == w["C"][:n_cc - 1]
                assert abs(math.fsum(w["C"][n_cc - 1:]) - n["C"][n_cc - 1]) <= T * EPS * n["C"][n_cc - 1]
                assert n["M"] == w["M"] and n["ln_p"] == w["ln_p"]
    assert any("wide_of" in c for c in golden["cases"])


def _classes(erroneous, counts=None, keys=None, copy=None):
    K = len(erroneous)
    err = np.zeros((K, 3))
    err[:, 1] = np.asarray(erroneous) * 0.75
    err[:, 2] = np.asarray(erroneous) * 0.25
    err[:, 0] = 1 - np.asarray(erroneous)
    copy = np.tile([0.5, 0.25, 0.25], (K, 1)) if copy is None else np.asarray(copy, dtype=float)
    return PosteriorClasses(np.arange(1, K + 1) if keys is None else keys, np.ones(K) if counts is None else counts,
                            np.zeros(K), err, copy, np.ones(K))


def test_erroneous_is_summed_not_complemented():
    err = np.array([[1.0, 1e-30, 2e-30], [0.25, 0.5, 0.25]])
    pc = PosteriorClasses([1, 2], [1, 1], [0, 0], err, np.ones((2, 1)), np.ones(2))
    assert pc.erroneous.tolist() == [1e-30 + 2e-30, 0.75]  # 1 - E_0 would give 0 in the first row
    assert pc.error_free.tolist() == [1.0, 0.25]


def test_error_cutoff_is_not_the_first_crossing():
    # below 0.5 at key 2, above again at key 3: the first crossing is 2, the cutoff 4
    pc = _classes([0.9, 0.4, 0.6, 0.3, 0.1])
    assert pc.error_cutoff() == 4
    assert pc.error_cutoff(level=0.95) == 1
    assert pc.error_cutoff(level=0.35) == 4
    assert pc.error_cutoff(level=0.2) == 5
    assert pc.error_cutoff(level=0.05) is None
    # keys in dict order, not ascending: the rule is over ascending keys
    assert _classes([0.1, 0.9, 0.3], keys=[30, 1, 7]).error_cutoff() == 7
    # the last key fails: None, whatever came before
    assert _classes([0.1, 0.1, 0.7]).error_cutoff() is None


def test_nan_rows():
    pc = _classes([0.9, float("nan"), 0.2, 0.1], counts=[10, 5, 4, 2])
    assert pc.error_cutoff() == 3  # NaN counts as not below
    pc2 = _classes([0.9, 0.2, float("nan")])
    assert pc2.error_cutoff() is None
    got = pc.expected_kmers()
    assert got["undefined"] == 5.0
    assert got["erroneous"] == pytest.approx(10 * 0.9 + 4 * 0.2 + 2 * 0.1, rel=1e-15)
    assert got["error_free"] == pytest.approx(10 * 0.1 + 4 * 0.8 + 2 * 0.9, rel=1e-15)


def test_expected_kmers_by_hand():
    copy = [[1.0, 0.0, 0.0], [0.5, 0.25, 0.25], [0.0, 0.5, 0.5]]
    pc = _classes([0.5, 0.25, 0.0], counts=[8, 4, 2], copy=copy)
    got = pc.expected_kmers()
    assert set(got) == {"erroneous", "error_free", "copies_1", "copies_2", "copies_ge_3", "undefined"}
    assert got == {"erroneous": 5.0, "error_free": 9.0, "copies_1": 10.0, "copies_2": 2.0, "copies_ge_3": 2.0,
                   "undefined": 0.0}
    one = PosteriorClasses([1], [3], [0], [[1.0]], [[1.0]], [1.0]).expected_kmers()
    assert one == {"erroneous": 0.0, "error_free": 3.0, "copies_ge_1": 3.0, "undefined": 0.0}


class _StandIn:
    """What print_output touches of a model, without a device."""
    params = ("coverage", "error_rate")
    hist = {1: 8, 2: 4, 3: 2}

    def short_name(self):
        return "basic"

    def correct_c(self, c):
        return c * 0.8

    def compute_loglikelihood(self, *args):
        return -123.5


def test_print_output_with_and_without_posterior():
    hist = dict(_StandIn.hist)
    base = print_output(hist, _StandIn(), True, 2, estimated=(10.0, 0.05), silent=True)
    same = print_output(hist, _StandIn(), True, 2, estimated=(10.0, 0.05), silent=True, posterior=None)
    assert same == base and list(same) == list(base)
    assert not any(k.startswith("posterior") for k in base)
    pc = _classes([0.5, 0.25, 0.0], counts=[8, 4, 2], copy=[[1.0, 0.0, 0.0], [0.5, 0.25, 0.25], [0.0, 0.5, 0.5]])
    rec = print_output(hist, _StandIn(), True, 2, estimated=(10.0, 0.05), silent=True, posterior=pc)
    assert {k: v for k, v in rec.items() if not k.startswith("posterior")} == base
    assert {k: v for k, v in rec.items() if k.startswith("posterior")} == {
        "posterior_error_cutoff": 2, "posterior_erroneous_kmers": 5.0, "posterior_error_free_kmers": 9.0,
        "posterior_copies_1": 10.0, "posterior_copies_2": 2.0, "posterior_copies_ge_3": 2.0,
        "posterior_undefined_kmers": 0.0, "posterior_sample_factor": 2}  # not scaled back: the fitted histogram's numbers


def test_value_errors_before_the_library_is_asked():
    b = BasicModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)
    r = RepeatsModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            posterior_classes(b, (10.0, 0.05), copy_columns=bad)
        with pytest.raises(ValueError):
            b.posterior_classes_points([[10.0, 0.05]], copy_columns=bad)
    with pytest.raises(ValueError):
        posterior_classes(b, (10.0, 0.05, 0.5))
    with pytest.raises(ValueError):
        posterior_classes(r, (10.0, 0.05))
    with pytest.raises(ValueError):
        r.posterior_classes_points([[10.0, 0.05]])
    assert b._handle is None and r._handle is None  # nothing reached the library
