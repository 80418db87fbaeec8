"""The duplicate remover without a device: the two symbols in the header and in _capi.EXPORTS,
the Python argument rules, the restatement (tests/dedup_reference.py) against a dictionary of byte strings on the shapes
the GPU tests use, and tests/read_fingerprint_check.cpp -- csrc/read_fingerprint.h built with the host compiler under the
address and undefined-behaviour sanitizers, and run as a program; its keys are held against the restatement's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dedup_reference as dr
from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "covest_amd", "csrc")
SYMBOLS = ("covest_dedup_reads", "covest_dedup_reads_device")


def test_header_and_exports_name_both_symbols():
    from covest_amd import _capi
    header = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _capi.EXPORTS, name
    # the fingerprint is stated where the ABI is: the finaliser's constants, as csrc/read_fingerprint.h has them
    fingerprint = open(os.path.join(CSRC, "read_fingerprint.h")).read()
    for constant in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15"):
        assert constant in header and constant in fingerprint, constant
    build = open(os.path.join(REPO, "covest_amd", "build.py")).read()
    assert '"abi_dedup.cpp"' in build and '"dedup_reads.hip"' in build


def test_package_exports():
    import covest_amd
    from covest_amd.dedup import DedupReads, dedup_reads
    assert covest_amd.dedup_reads is dedup_reads and covest_amd.DedupReads is DedupReads


def test_argument_rules_raise_before_the_library_is_asked(monkeypatch):
    from covest_amd import _capi
    from covest_amd.dedup import dedup_reads, dedup_reads_device

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_capi, "lib", no_library)
    reads = np.frombuffer(b"acgtacgt", dtype=np.uint8).reshape(2, 4)
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(first_read=-1), dict(first_read=1.5)):
        with pytest.raises(ValueError):
            dedup_reads(reads, **bad)
    for bad in (np.zeros((2, 4), dtype=np.int32), np.zeros(4, dtype=np.uint8),
                (np.zeros(4, dtype=np.uint8), np.array([0, 5])), (np.zeros(4, dtype=np.uint8), np.array([2, 1]))):
        with pytest.raises(ValueError):
            dedup_reads(bad)
    good = dict(bases_ptr=256, n_reads=2, out_bases_ptr=512, counts_ptr=1024, read_len=4)
    for bad in (dict(fp_bits=0), dict(fp_bits=64), dict(fp_bits=True), dict(fp_bits=7.5), dict(n_reads=-1), dict(read_len=-1),
                dict(counts_ptr=0), dict(offsets_ptr=2048), dict(seed=-1), dict(first_read=-1)):
        with pytest.raises(ValueError):
            dedup_reads_device(**dict(good, **bad))


def shapes():
    """The read sets of tests/test_gpu_dedup.py that have no device in them: (name, reads)."""
    yield "none", []
    yield "one", dr.random_reads(1, 100, 1)
    yield "1000 copies", dr.random_reads(1, 100, 2) * 1000
    yield "no two equal", dr.random_reads(500, 100, 3)
    yield "30 % copies", dr.with_copies(3000, 100, 0.3, 4)
    yield "30 % copies, half reversed", dr.with_copies(3000, 100, 0.3, 5, rc_copies=True)
    yield "ragged", dr.ragged(6)
    yield "ragged, other bytes", dr.ragged(7, alphabet=np.frombuffer(b"acgtnACGTN", dtype=np.uint8))
    for length in dr.LENGTHS:
        yield "length %d" % length, dr.with_copies(40, length, 0.3, 8 + length, rc_copies=True)


@pytest.mark.parametrize("reverse_complement", (False, True))
def test_restatement_agrees_with_a_dictionary_of_byte_strings(reverse_complement):
    for name, reads in shapes():
        kept, copies, collided = dr.dedup(reads, 63, seed=11, reverse_complement=reverse_complement)
        want_kept, want_copies = dr.dictionary(reads, reverse_complement)
        assert collided == 0, name
        assert np.array_equal(kept, want_kept) and np.array_equal(copies, want_copies), name
        assert int(copies.sum()) == len(reads), name


def test_restatement_collision_route():
    """With few bits different reads share keys: they are kept and counted, every dropped read still has an equal before
    it, and a duplicate survives only where its first copy lost the key to another read."""
    reads = dr.with_copies(3000, 100, 0.3, 4)
    want_kept, _ = dr.dictionary(reads)
    for bits in (1, 4, 8):
        kept, copies, collided = dr.dedup(reads, bits, seed=3)
        assert collided > 0 and int(copies.sum()) == len(reads)
        assert set(want_kept) <= set(kept) and len(kept) <= len(want_kept) + collided
        held = set(kept)
        for i in set(range(len(reads))) - held:
            assert any(reads[j] == reads[i] for j in kept[kept < i])


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = shutil.which(name) if name else None
        if exe:
            return exe
    return None


def test_read_fingerprint_under_sanitizers(tmp_path):
    """As tests/test_read_bootstrap_cpu.py builds its program: the host compiler, -fsanitize=address,undefined, a main
    of its own, no preloaded runtime.  Then the header's keys against the restatement's, on reads passed as arguments."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "read_fingerprint_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "read_fingerprint_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "read_fingerprint ok" in run.stdout, run.stdout + run.stderr
    alphabet = np.frombuffer(b"acgtnACGTN", dtype=np.uint8)
    reads = [dr.random_reads(1, length, 20 + length, alphabet)[0] for length in (0, 1, 2, 63, 64, 65, 300, 1000)]
    for seed, rc, bits in ((0, 0, 63), (0, 1, 63), ((0x57e4 << 32) | 0x0badf00d, 1, 63), ((1 << 64) - 1, 0, 8), (5, 1, 1)):
        run = subprocess.run([exe, str(seed), str(rc), str(bits)] + [r.decode() or "-" for r in reads],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        assert [int(line) for line in run.stdout.split()] == [dr.key(r, seed, bool(rc), bits) for r in reads], (seed, rc, bits)
