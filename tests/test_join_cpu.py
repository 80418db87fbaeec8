"""The join of two k-mer tables without a device: the restatement (tests/join_reference.py)
against a loop over every possible key of hand-made dicts, every CopySpectrum method on hand-made matrices, and
tests/join_cells_check.cpp -- the cell arithmetic the kernel compiles (csrc/kmer_join.h) -- built with the host compiler
under the address and undefined-behaviour sanitizers, and run."""
import math
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import join_reference as jr
from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")


# ---- the restatement ------------------------------------------------------------------------------------------------
def brute_force(counts_a, counts_b, rows, cols, universe):
    """The definition, key by key over `universe` (every key that could be held), cell by cell."""
    out = [[0] * cols for _ in range(rows)]
    for i in range(rows):
        for j in range(cols):
            for x in universe:
                a, b = counts_a.get(x, 0), counts_b.get(x, 0)
                if (a > 0 or b > 0) and min(a, rows - 1) == i and min(b, cols - 1) == j:
                    out[i][j] += 1
    return out


UNIVERSE = range(40)
HAND_MADE = {
    "disjoint": (Counter({1: 1, 2: 2, 3: 7}), Counter({10: 1, 11: 3, 12: 3})),
    "identical": (Counter({4: 1, 5: 2, 6: 2, 7: 9}), Counter({4: 1, 5: 2, 6: 2, 7: 9})),
    "b empty": (Counter({0: 3, 39: 1}), Counter()),
    "a empty": (Counter(), Counter({0: 3, 39: 1, 20: 1})),
    "both empty": (Counter(), Counter()),
    # counts at, below and above the clips of (4, 3): rows clip at 3, columns at 2
    "around the clips": (Counter({1: 2, 2: 3, 3: 4, 4: 1, 5: 3, 6: 100, 8: 2}),
                         Counter({1: 1, 2: 2, 3: 3, 4: 2, 5: 50, 7: 2, 9: 1, 6: 1})),
    "overlapping": (Counter({x: x % 5 + 1 for x in range(0, 30)}), Counter({x: x % 3 + 1 for x in range(20, 40)})),
}
SHAPES = [(1, 1), (1, 4), (4, 1), (2, 2), (4, 3), (3, 4), (8, 8), (120, 60)]


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_reference_is_the_definition(name):
    a, b = HAND_MADE[name]
    for rows, cols in SHAPES:
        got = jr.join(a, b, rows, cols)
        assert got.dtype == np.int64 and got.shape == (rows, cols)
        assert got.tolist() == brute_force(a, b, rows, cols, UNIVERSE), (name, rows, cols)
        assert got.sum() == len(set(a) | set(b)) and (got[0, 0] == 0 or rows == 1 or cols == 1)
    rows, cols = jr.unclipped_shape(a, b)
    full = jr.join(a, b, rows, cols)
    assert full.tolist() == brute_force(a, b, rows, cols, UNIVERSE)
    assert full[1:].sum(axis=1).tolist() == [sum(1 for v in a.values() if v == i) for i in range(1, rows)]
    assert full[:, 1:].sum(axis=0).tolist() == [sum(1 for v in b.values() if v == j) for j in range(1, cols)]


def test_reference_details():
    a, b = HAND_MADE["identical"]
    full = jr.join(a, b, *jr.unclipped_shape(a, b))
    assert full.sum() == np.trace(full) == 4                     # A = B: nothing off the diagonal
    a, b = HAND_MADE["disjoint"]
    full = jr.join(a, b, *jr.unclipped_shape(a, b))
    assert full[1:, 1:].sum() == 0 and full[0].sum() == 3 and full[:, 0].sum() == 3
    assert jr.join(Counter({1: 0, 2: 1}), Counter({1: 0}), 3, 3).sum() == 1   # a count of 0 is a key not held
    assert jr.join(Counter(), Counter(), 1, 1).tolist() == [[0]]
    with pytest.raises(ValueError):
        jr.join(a, b, 0, 1)
    with pytest.raises(ValueError):
        jr.join(a, b, 1, 0)
    assert len(jr.genome(0)) == len(jr.genome(1)) == jr.GENOME_LEN and jr.genome(0) != jr.genome(1)
    reads = jr.noisy_reads(1, n=50)
    assert reads == jr.noisy_reads(1, n=50) and len(reads) == 50 and all(60 <= len(r) <= 100 for r in reads)
    assert any(r.islower() for r in reads) and any(r.isupper() for r in reads)


# ---- CopySpectrum on hand-made matrices ----------------------------------------------------------------------------------
#            o = 0   1   2   3   4   5
MATRIX = [[0,  2,  1,  0,  0,  1],    # a = 0: genomic k-mers no read holds
          [90, 10, 0,  0,  0,  0],    # a = 1
          [6,  3,  1,  0,  0,  0],    # a = 2
          [0,  0,  0,  0,  0,  0],    # a = 3: no k-mer at all
          [1,  30, 6,  2,  1,  1],    # a = 4
          [4,  0,  0,  0,  0,  0],    # a = 5: erroneous only -- the error curve is not monotone
          [0,  5,  10, 5,  0,  0]]    # a = 6


def spectrum():
    from covest_amd.copy_spectrum import CopySpectrum
    return CopySpectrum(MATRIX)


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(
        got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-15, atol=0)


def test_copy_spectrum_sums():
    s = spectrum()
    assert s.matrix.dtype == np.int64 and s.matrix.shape == (7, 6)
    assert s.abundance_histogram().tolist() == [0, 100, 10, 0, 41, 4, 20]
    assert s.genome_spectrum() == {1: 50, 2: 18, 3: 7, 4: 1, 5: 2}
    assert s.unseen().tolist() == [0, 2, 1, 0, 0, 1]
    assert s.observed_kmers(3) == {"erroneous": 101, "error_free": 74, "copies_1": 48, "copies_2": 17, "copies_ge_3": 9,
                                   "undefined": 0}
    assert s.observed_kmers() == {"erroneous": 101, "error_free": 74, "copies_1": 48, "copies_2": 17, "copies_3": 7,
                                  "copies_ge_4": 2, "undefined": 0}
    assert s.observed_kmers(1) == {"erroneous": 101, "error_free": 74, "copies_ge_1": 74, "undefined": 0}
    assert s.observed_kmers(3, keys=[1, 2, 9]) == {"erroneous": 96, "error_free": 14, "copies_1": 13, "copies_2": 1,
                                                   "copies_ge_3": 0, "undefined": 0}
    for bad in ([], [[]], [1, 2], np.zeros((0, 3))):
        with pytest.raises(ValueError):
            from covest_amd.copy_spectrum import CopySpectrum
            CopySpectrum(bad)


def test_copy_spectrum_shares():
    s = spectrum()
    nan = math.nan
    assert same(s.error_share(), [nan, 0.9, 0.6, nan, 1 / 41, 1.0, 0.0])
    assert same(s.copy_share(3), [[0.5, 0.25, 0.25], [1, 0, 0], [0.75, 0.25, 0], [nan] * 3, [30 / 40, 6 / 40, 4 / 40],
                                  [nan] * 3, [0.25, 0.5, 0.25]])
    assert same(s.copy_share(1), [[1], [1], [1], [nan], [1], [nan], [1]])
    wide = s.copy_share(8)                                       # more columns than the matrix has copy numbers
    assert wide.shape == (7, 8) and same(wide[4], [30 / 40, 6 / 40, 2 / 40, 1 / 40, 1 / 40, 0, 0, 0])
    assert same(s.copy_share(), s.copy_share(4)) and same(s.copy_share(4)[4], [30 / 40, 6 / 40, 2 / 40, 2 / 40])
    assert same(s.mean_copies(), [(2 + 2 + 5) / 4, 1.0, 5 / 4, nan, (30 + 12 + 6 + 4 + 5) / 40, nan, 2.0])
    with pytest.raises(ValueError):
        s.copy_share(0)
    from covest_amd.copy_spectrum import CopySpectrum
    no_genome = CopySpectrum([[0], [5], [2]])                    # one column: nothing is genomic
    assert same(no_genome.error_share(), [nan, 1, 1]) and same(no_genome.mean_copies(), [nan] * 3)
    assert same(no_genome.copy_share(2), [[nan, nan]] * 3) and no_genome.genome_spectrum() == {}
    assert no_genome.error_cutoff() is None


def test_copy_spectrum_error_cutoff():
    """The rule of PosteriorClasses.error_cutoff: below the level at EVERY abundance from the cutoff on that has k-mers --
    not the first crossing (a = 4 is below 0.5, a = 5 is not), abundances without k-mers passed over (a = 3)."""
    from covest_amd.copy_spectrum import CopySpectrum
    s = spectrum()
    assert s.error_cutoff() == 6 and s.error_cutoff(0.5) == 6
    assert s.error_cutoff(1.5) == 1                              # every abundance passes: the smallest with k-mers
    assert s.error_cutoff(0.0) is None                           # the largest fails (0.0 is not below 0.0)
    monotone = CopySpectrum([[0, 1], [9, 1], [5, 5], [0, 0], [1, 9], [0, 4]])
    assert monotone.error_cutoff() == 4 and monotone.error_cutoff(0.6) == 2 and monotone.error_cutoff(0.05) == 5
    assert CopySpectrum([[0, 1], [9, 1], [1, 9], [7, 3]]).error_cutoff() is None      # the largest abundance fails
    assert CopySpectrum([[0, 3]]).error_cutoff() is None and CopySpectrum([[0]]).error_cutoff() is None
    # the same rule, the same answer, from the posterior's own implementation
    from covest_amd.posterior import PosteriorClasses
    share = s.error_share()
    keys = [a for a in range(1, 7) if not math.isnan(share[a])]
    post = PosteriorClasses(keys, [1] * len(keys), [0.0] * len(keys), [[1 - share[a], share[a]] for a in keys],
                            [[1.0]] * len(keys), [1.0] * len(keys))
    for level in (0.0, 0.01, 0.3, 0.5, 0.61, 0.95, 1.5):
        assert post.error_cutoff(level) == s.error_cutoff(level), level


def test_copy_spectrum_compare():
    from covest_amd.posterior import PosteriorClasses
    s = spectrum()
    keys = [2, 1, 4, 6, 3, 9]                                    # the posterior's own order; 3: no k-mers; 9: beyond the matrix
    counts = [10, 100, 41, 20, 0, 1]
    err = [[0.5, 0.4, 0.1], [0.05, 0.9, 0.05], [0.995, 0.005, 0.0], [1.0, 0.0, 0.0], [0.99, 0.01, 0.0], [1.0, 0.0, 0.0]]
    cop = [[0.7, 0.2, 0.1], [0.9, 0.1, 0.0], [0.8, 0.15, 0.05], [0.2, 0.5, 0.3], [0.9, 0.1, 0.0], [0.0, 0.1, 0.9]]
    post = PosteriorClasses(keys, counts, [0.0] * 6, err, cop, [1.0] * 6)
    got = s.compare(post)
    nan = math.nan
    assert got["keys"].tolist() == keys
    model, measured = got["erroneous"]
    assert same(model, [0.5, 0.95, 0.005, 0.0, 0.01, 0.0]) and same(measured, [0.6, 0.9, 1 / 41, 0.0, nan, nan])
    assert got["copy_keys"].tolist() == [4, 6, 3, 9]             # E_0 >= 0.99
    model, measured = got["copy_share"]
    assert same(model, [cop[2], cop[3], cop[4], cop[5]])
    assert same(measured, [[30 / 40, 6 / 40, 4 / 40], [0.25, 0.5, 0.25], [nan] * 3, [nan] * 3])
    assert got["copy_observed"] == {"copies_1": 35, "copies_2": 16, "copies_ge_3": 9}      # abundances 3, 4 and 6
    assert list(got["copy_expected"]) == ["copies_1", "copies_2", "copies_ge_3"]
    assert same(list(got["copy_expected"].values()), [41 * 0.8 + 20 * 0.2, 41 * 0.15 + 20 * 0.5 + 0.1, 41 * 0.05 + 20 * 0.3 + 0.9])
    assert got["error_cutoff"] == (3, 6)                       # the model's: key 2 is at 0.5, not below; key 3 passes
    assert got["expected"] == post.expected_kmers()
    assert got["observed"] == s.observed_kmers(3, keys=keys)
    assert got["observed"]["erroneous"] == 97 and got["observed"]["copies_1"] == 48
    strict = s.compare(post, min_error_free=1.0)
    assert strict["copy_keys"].tolist() == [6, 9] and strict["copy_share"][0].shape == (2, 3)
    none = s.compare(post, min_error_free=2.0)
    assert none["copy_keys"].size == 0 and none["copy_share"][1].shape == (0, 3)


def test_copy_spectrum_sizes_are_checked_before_the_device():
    """copy_spectrum sizes the matrix from the clips or from stats(); 2^22 cells at most, and the message names the
    clip to pass."""
    from covest_amd.copy_spectrum import copy_spectrum

    class Fake:
        def __init__(self, need):
            self.need = need
            self.joined = None

        def stats(self):
            return self.need, 0

        def join_histogram(self, other, rows, cols):
            self.joined = (rows, cols)
            return np.zeros((rows, cols), dtype=np.int64)

    reads, genome = Fake(301), Fake(12)
    assert copy_spectrum(reads, genome).matrix.shape == (301, 12) and reads.joined == (301, 12)
    assert copy_spectrum(reads, genome, max_abundance=9).matrix.shape == (10, 12)
    assert copy_spectrum(reads, genome, max_copies=0).matrix.shape == (301, 1)
    assert copy_spectrum(reads, genome, 0, 0).matrix.shape == (1, 1)
    assert copy_spectrum(Fake(1 << 20), Fake(4)).matrix.shape == (1 << 20, 4)
    with pytest.raises(ValueError, match="max_abundance"):
        copy_spectrum(Fake((1 << 20) + 1), Fake(4))
    with pytest.raises(ValueError, match="max_copies"):
        copy_spectrum(Fake(4), Fake((1 << 20) + 1))
    with pytest.raises(ValueError, match="max_copies"):
        copy_spectrum(Fake(4), Fake(100), max_abundance=1 << 20)
    with pytest.raises(ValueError, match="max_abundance"):
        copy_spectrum(Fake(1 << 22), Fake(100), max_copies=1)
    with pytest.raises(ValueError):
        copy_spectrum(reads, genome, max_abundance=-1)


def test_print_output_records_the_copy_spectrum():
    """print_output(copy_spectrum=): the totals, the measured cutoff and spectrum_to_q of the genome's spectrum; the
    record is unchanged without it."""
    from covest_amd import BasicModel, print_output, spectrum_to_q
    model = BasicModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)
    plain = print_output({1: 10, 2: 5}, model, True, 1, silent=True)
    with_it = print_output({1: 10, 2: 5}, model, True, 1, silent=True, copy_spectrum=spectrum())
    assert {k: v for k, v in with_it.items() if not k.startswith("copy_spectrum_")} == plain
    q1, q2, q = spectrum_to_q({1: 50, 2: 18, 3: 7, 4: 1, 5: 2})
    assert {k: v for k, v in with_it.items() if k.startswith("copy_spectrum_")} == {
        "copy_spectrum_erroneous_kmers": 101, "copy_spectrum_error_free_kmers": 74, "copy_spectrum_copies_1": 48,
        "copy_spectrum_copies_2": 17, "copy_spectrum_copies_3": 7, "copy_spectrum_copies_ge_4": 2,
        "copy_spectrum_undefined_kmers": 0, "copy_spectrum_error_cutoff": 6, "copy_spectrum_q1": q1,
        "copy_spectrum_q2": q2, "copy_spectrum_q": q}


def test_the_binding_declares_the_join():
    from covest_amd import _capi
    assert {"covest_kmer_join_histogram", "covest_kmer_join_histogram_device"} <= set(_capi.EXPORTS)
    import covest_amd
    assert callable(covest_amd.copy_spectrum) and callable(covest_amd.genome_counts) and covest_amd.CopySpectrum
    from covest_amd import build
    assert {"kmer_join.hip", "abi_join.cpp"} <= {s[0] for s in build.SOURCES}


# ---- the cell arithmetic under the sanitizers ----------------------------------------------------------------------------
def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = shutil.which(name) if name else None
        if exe:
            return exe
    return None


def test_join_cells_under_sanitizers(tmp_path):
    """As tests/test_read_bootstrap_cpu.py builds its program: the host compiler, -fsanitize=address,undefined, a main of
    its own, no preloaded runtime."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "join_cells_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "join_cells_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "join_cells ok" in run.stdout, run.stdout + run.stderr
