"""The read bootstrap without a device: the thirteen thresholds of the Poisson(1) multiplicity
derived exactly, the restatement's frequencies (tests/bootstrap_weights_reference.py), summarize_read_bootstrap on
hand-made arrays, and tests/read_weights_check.cpp -- where a launch of a weighted add starts in the weights, beyond the
launch cuts no GPU test reaches -- built with the host compiler under the address and undefined-behaviour sanitizers, and
run."""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bootstrap_weights_reference as bw
from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")


def exact_thresholds():
    """floor(2^32 P(Poisson(1) <= i)), i = 0 .. 12, in exact arithmetic: 1 / e from its alternating series, cut where
    the next term is below 2^-200, so that the truncation is far below the distance of any 2^32 cdf_i from an integer
    (checked: the floor is the same at both ends of the enclosure)."""
    terms, n, term = [], 0, Fraction(1)
    while term > Fraction(1, 1 << 200):
        terms.append(term if n % 2 == 0 else -term)
        n += 1
        term /= n
    lo, hi = sorted((sum(terms), sum(terms) + (term if n % 2 == 0 else -term)))  # an alternating series encloses its limit
    out = []
    for i in range(13):
        partial = sum(Fraction(1, math.factorial(j)) for j in range(i + 1))
        a, b = math.floor((1 << 32) * lo * partial), math.floor((1 << 32) * hi * partial)
        assert a == b, i
        out.append(a)
    tail = 1 - hi * sum(Fraction(1, math.factorial(j)) for j in range(13))
    return out, tail


def test_the_thirteen_constants_are_the_floor_of_the_distribution_function():
    want, tail = exact_thresholds()
    assert list(bw.THRESHOLDS) == want
    assert want[-1] == (1 << 32) - 1 and 0 < tail * (1 << 32) < 0.3    # the mass beyond 12 is 0.27 * 2^-32
    # the header and the kernels' table carry the same thirteen numbers, in order
    for path in (os.path.join(REPO, "include", "covest_amd.h"), os.path.join(CSRC, "sim_philox.h")):
        text = open(path).read()
        at = text.index("1580030168")
        found = [int(v) for v in re.findall(r"\d{10}", text[at:at + 600])][:13]
        assert found == want, path
    philox = open(os.path.join(CSRC, "sim_philox.h")).read()
    assert "kStreamBootstrap = 9" in philox and re.search(r"//\s+bootstrap\s+read r\s+replicate b", philox)
    header = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    assert "(lo32(r), hi32(r), b, 9)" in header and "9 bootstrap" in header
    from covest_amd import _capi
    assert {"covest_bootstrap_weights", "covest_bootstrap_weights_device", "covest_kmer_add_weighted",
            "covest_kmer_add_weighted_device"} <= set(_capi.EXPORTS)


def test_the_restatement_has_the_poisson_frequencies():
    n = 1_000_000
    m = bw.weights(n, 3, seed=(5 << 32) | 77, first_read=(1 << 32) - 1000)
    assert m.dtype == np.uint32 and m.shape == (n,) and int(m.max()) <= 13
    counts = np.bincount(m, minlength=14)
    for i in range(14):
        p = math.exp(-1.0) / math.factorial(i) if i < 13 else 1e-12
        sd = math.sqrt(n * p * (1.0 - p))
        assert abs(counts[i] - n * p) <= 5.0 * sd + 1e-9, (i, int(counts[i]), n * p, sd)
    # the steps themselves, and rows of a run against the whole
    assert bw.multiplicity([0, bw.THRESHOLDS[0] - 1, bw.THRESHOLDS[0], bw.THRESHOLDS[12] - 1, bw.THRESHOLDS[12]]).tolist() \
        == [0, 0, 1, 12, 13]
    whole = bw.weights(1000, 1, seed=9, first_read=(1 << 32) - 3)
    assert np.array_equal(bw.weights(401, 1, seed=9, first_read=(1 << 32) - 3 + 300), whole[300:701])
    assert not np.array_equal(bw.weights(1000, 2, seed=9, first_read=(1 << 32) - 3), whole)
    assert bw.expand(["a", "b", "c", "d"], [0, 2, 1, 0]) == ["b", "b", "c"]


def test_summarize_read_bootstrap_on_hand_made_arrays():
    from covest_amd.bootstrap import _percentiles
    from covest_amd.read_bootstrap import summarize_read_bootstrap
    names = ["coverage", "error_rate"]
    est = np.array([[10.0, 0.010], [12.0, 0.012], [99.0, 0.5], [9.0, 0.011], [11.0, 0.013]])
    ok = np.array([True, True, False, True, True])
    occ = np.array([1000.0, 1250.0, 7.0, 800.0, 1100.0])
    full, occ_full = [10.5, 0.0115], 1000.0
    bound = np.array([[False, False], [False, True], [True, True], [False, False], [False, True]])

    def correct_c(c):
        return 0.8 * c

    out = summarize_read_bootstrap(est, ok, full, occ, occ_full, names, None, 0.9, correct_c, at_bound=bound)
    assert out["used"] == 4 and out["failed"] == 1
    good = [0, 1, 3, 4]
    columns = {
        "coverage": np.array([est[b, 0] * occ_full / occ[b] for b in good]),          # the rescaling to the full set
        "error_rate": est[good, 1],
        "genome_size": np.array([occ[b] / correct_c(est[b, 0]) for b in good]),
    }
    assert columns["coverage"].tolist() == [10.0, 9.6, 11.25, 10.0]                    # (the failed replicate is not there)
    at_full = {"coverage": 10.5, "error_rate": 0.0115, "genome_size": occ_full / correct_c(10.5)}
    for name, v in columns.items():
        mean = v.mean()
        assert out["mean"][name] == pytest.approx(mean, rel=1e-15)
        assert out["standard_errors"][name] == pytest.approx(math.sqrt(((v - mean) ** 2).sum() / (len(v) - 1)), rel=1e-14)  # ddof 1
        assert out["bias"][name] == pytest.approx(mean - at_full[name], abs=1e-15 * abs(mean))
        lo, hi = _percentiles(v, 0.9)
        # (the test forms c * full / occ, the code c * (full / occ): a few units in the last place of a double apart)
        assert out["intervals"][name] == pytest.approx([float(lo), float(hi)], rel=1e-14)
        assert out["intervals"][name][0] <= np.median(v) <= out["intervals"][name][1]
    assert out["bound_share"] == {"coverage": 0.0, "error_rate": 0.5, "genome_size": 0.0}
    # a fixed parameter: None everywhere; the genome size goes with the coverage
    fixed = summarize_read_bootstrap(est, ok, full, occ, occ_full, names, [None, 0.0115], 0.9, correct_c)
    assert fixed["standard_errors"]["error_rate"] is None and fixed["intervals"]["error_rate"] is None
    assert fixed["mean"]["error_rate"] is None and fixed["bias"]["error_rate"] is None
    assert fixed["standard_errors"]["coverage"] == out["standard_errors"]["coverage"]
    assert fixed["bound_share"]["coverage"] is None                                     # (no at_bound given)
    no_c = summarize_read_bootstrap(est, ok, full, occ, occ_full, names, [10.5, None], 0.9, correct_c)
    assert no_c["standard_errors"]["coverage"] is None and no_c["standard_errors"]["genome_size"] is None
    assert no_c["standard_errors"]["error_rate"] == out["standard_errors"]["error_rate"]
    # fewer than two successful refits: nothing can be said
    one = summarize_read_bootstrap(est, [True, False, False, False, False], full, occ, occ_full, names, None, 0.9, correct_c)
    assert one["used"] == 1 and one["failed"] == 4
    assert all(v is None for key in ("mean", "standard_errors", "bias", "intervals", "bound_share") for v in one[key].values())
    assert set(one["mean"]) == {"coverage", "error_rate", "genome_size"}
    with pytest.raises(ValueError):
        summarize_read_bootstrap(est, ok, full, occ, occ_full, names, None, 1.0, correct_c)
    with pytest.raises(ValueError):
        summarize_read_bootstrap(est, ok[:3], full, occ, occ_full, names, None, 0.9, correct_c)


def test_arguments_are_checked_before_the_library_is_asked():
    from covest_amd import read_bootstrap as rb_function
    from covest_amd.kmer_hist import _read_weights
    from covest_amd.read_bootstrap import bootstrap_histograms, bootstrap_weights, read_bootstrap
    assert rb_function is read_bootstrap
    for bad in (dict(n_reads=-1, replicate=0), dict(n_reads=1, replicate=-1), dict(n_reads=1, replicate=1 << 32),
                dict(n_reads=1, replicate=0, seed=1 << 64), dict(n_reads=1, replicate=0, first_read=-1)):
        with pytest.raises(ValueError):
            bootstrap_weights(**bad)
    reads = np.frombuffer(b"ACGTACGTAC" * 4, dtype=np.uint8).reshape(4, 10)
    for bad in (dict(replicates=1), dict(replicates=2.0), dict(replicates=True), dict(replicates=4, seed=-1)):
        with pytest.raises(ValueError):
            bootstrap_histograms(reads, 5, **bad)
    with pytest.raises(ValueError):
        bootstrap_histograms(reads, 0, 4)
    assert _read_weights([0, 1, 70000], 3).dtype == np.uint32
    for bad in ([0, 1], [0, -1, 2], [0, 1 << 32, 2], [0.5, 1.0, 2.0], [[0, 1, 2]]):
        with pytest.raises(ValueError):
            _read_weights(bad, 3)

    class Model:
        params, k, device, sample_factor = ("coverage", "error_rate"), 21, 0, 1
    for bad in (dict(replicates=1), dict(level=1.0), dict(refit="each"), dict(sample_factor=2), dict(fix=[None]),
                dict(trim=0), dict(refit="lockstep", gradient="analytic"), dict(gradient="fd")):
        with pytest.raises(ValueError):
            read_bootstrap(Model(), [10.0, 0.01], reads, **bad)
    with pytest.raises(ValueError):
        read_bootstrap(Model(), [10.0], reads)


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = shutil.which(name) if name else None
        if exe:
            return exe
    return None


def test_read_weights_under_sanitizers(tmp_path):
    """As tests/test_kmer_plan_cpu.py builds its programs: the host compiler, -fsanitize=address,undefined, a main of its
    own, no preloaded runtime."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "read_weights_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "read_weights_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "read_weights ok" in run.stdout, run.stdout + run.stderr
