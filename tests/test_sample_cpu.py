"""The read sampler without a device: the selection word against the stream spelled out in plain integers, the
threshold, the restatement's own statistics and chunk invariance (the device is required to be bit-identical to it,
tests/test_gpu_sample.py), the argument rules of covest_amd.sample and of the C entry points, and that nothing is
computed where there is no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import sample_reference as ref
import sim_reference as sr
from conftest import REPO


def test_selection_word_by_hand():
    for seed, r in ((0, 0), (7, 1), ((0x5eed << 32) | 0x1234abcd, (1 << 32) - 1), (99, 1 << 32), (1 << 63, (1 << 40) + 5)):
        want = sr.philox_scalar((r & 0xffffffff, r >> 32, 0, 2), (seed & 0xffffffff, seed >> 32))[0]
        assert int(ref.words(r, 1, seed)[0]) == want
        assert ref.counter(r) == (r & 0xffffffff, r >> 32, 0, 2)
        for factor in (1, 2, 3, 1e9):
            assert bool(ref.keep_mask(r, 1, factor, seed)[0]) == (want < ref.threshold(factor))


def test_threshold():
    from covest_amd import sample
    want = {1: 1 << 32, 2: 1 << 31, 3: 1431655765, 2.5: 1717986918, 1e9: 4,
            float(np.nextafter(1.0, 2.0)): (1 << 32) - 1}
    for factor, thr in want.items():
        assert ref.threshold(factor) == thr, factor
        assert sample.threshold(factor) == thr, factor
    assert ref.keep_mask(0, 100_000, 1, 12345).all()


def test_kept_count_statistics():
    n, seed, factor = 300_000, 7, 3
    p = ref.threshold(factor) / 2.0 ** 32
    kept = int(ref.keep_mask(0, n, factor, seed).sum())
    assert abs(kept - n * p) <= 6 * math.sqrt(n * p * (1 - p)), kept


def test_chunk_invariance_of_the_restatement():
    rng = np.random.default_rng(3)
    lens = rng.choice([0, 1, 2, 5, 100], size=2000)
    offsets = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bases = rng.integers(65, 85, size=int(offsets[-1]), dtype=np.uint8)
    first, seed = (1 << 32) - 700, 11
    whole = ref.sample(bases, offsets, first, 2, seed)
    for cut in (1, 255, 256, 1999):
        a = ref.sample(bases[:offsets[cut]], offsets[:cut + 1], first, 2, seed)
        b = ref.sample(bases[offsets[cut]:], offsets[cut:] - offsets[cut], first + cut, 2, seed)
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])
        assert np.array_equal(np.concatenate([a[1], b[1][1:] + a[1][-1]]), whole[1])
        assert np.array_equal(np.concatenate([a[2], b[2]]), whole[2])
    # fixed length: the same through a read length
    fixed = rng.integers(65, 85, size=(500, 7), dtype=np.uint8)
    out, out_offsets, kept = ref.sample(fixed, 7, 5, 2, seed)
    assert np.array_equal(out.reshape(-1, 7), fixed[kept - 5]) and np.array_equal(out_offsets, np.arange(kept.size + 1) * 7)


def test_stream_is_disjoint_from_the_simulator():
    """The sampler's counters end in 2; the simulator's in 1 (genome) and 0 (read headers and bases)."""
    for r in (0, 5, (1 << 32) + 1):
        assert ref.counter(r)[3] == 2 and ref.counter(r)[2] == 0
    text = open(os.path.join(REPO, "tests", "sim_reference.py")).read()
    assert "0, 1, *_key(seed)" in text and "0, 0, *_key(seed)" in text  # the restated simulator's last counter words
    w_sim = sr.philox(np.array([3], dtype=np.uint64), np.array([0], dtype=np.uint64), 0, 0, 9, 0)[0]
    assert int(w_sim[0]) != int(ref.words(3, 1, 9)[0])


def test_argument_validation(tmp_path):
    from covest_amd import sample
    reads = np.full((4, 5), 65, dtype=np.uint8)
    for bad in (0.5, 0, -2, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            sample.sample_reads(reads, bad)
        with pytest.raises(ValueError):
            sample.sample_reads_device(1, 4, 1, 1, bad, read_len=5)
        with pytest.raises(ValueError):
            sample.sampled_histogram(str(tmp_path / "none.fa"), 21, bad)
        with pytest.raises(ValueError):
            sample.sample_reads_file(str(tmp_path / "none.fa"), str(tmp_path / "out.fa"), bad)
    with pytest.raises(ValueError):
        sample.sample_reads(reads, 2, seed=1 << 64)
    with pytest.raises(ValueError):
        sample.sample_reads(reads, 2, seed=-1)
    with pytest.raises(ValueError):
        sample.sample_reads(reads, 2, first_read=-1)
    with pytest.raises(ValueError):
        sample.sample_reads(reads.astype(np.int32), 2)
    with pytest.raises(ValueError):
        sample.sample_reads(reads.reshape(-1), 2)                                  # neither (n, L) nor a pair
    with pytest.raises(ValueError):
        sample.sample_reads((reads.reshape(-1), np.array([0, 5, 3])), 2)           # offsets descend
    with pytest.raises(ValueError):
        sample.sample_reads((reads.reshape(-1), np.array([0, 5, 30])), 2)          # beyond the bases
    with pytest.raises(ValueError):
        sample.sample_reads_device(1, -1, 1, 1, 2, read_len=5)
    with pytest.raises(ValueError):
        sample.sample_reads_device(1, 4, 1, 1, 2, read_len=-1)
    with pytest.raises(ValueError):
        sample.sample_reads_device(1, 4, 1, 1, 2, offsets_ptr=8)                   # offsets without out_offsets
    with pytest.raises(ValueError):
        sample.sample_reads_device(1, 4, 1, 0, 2, read_len=5)                      # no counts
    assert not (tmp_path / "out.fa").exists()


def test_header_and_exports_name_the_symbols():
    from covest_amd import _capi
    text = open(os.path.join(REPO, "include", "covest_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("covest_sample_reads", "covest_sample_reads_device"):
        assert re.search(r"\bint %s\s*\(" % name, text) and name in _capi.EXPORTS


def test_c_entry_points_refuse_bad_arguments(hip_lib):
    """COVEST_E_INVALID before any device is looked for; the host form answers n_reads == 0 without one."""
    bases = np.full(64, 65, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    offsets = np.arange(9, dtype=np.int64) * 8
    out_offsets = np.full(9, -1, dtype=np.int64)
    counts = np.full(2, -1, dtype=np.int64)
    n_kept, n_bases = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def host(n=8, L=8, first=0, factor=2.0, offs=None, out_offs=None, nk=ctypes.byref(n_kept)):
        return hip_lib.covest_sample_reads(-1, bases.ctypes.data, offs, n, L, first, factor, 1, out.ctypes.data, out_offs, None,
                                           nk, ctypes.byref(n_bases))

    def device(n=8, L=8, first=0, factor=2.0, offs=None, out_offs=None, cnt=counts.ctypes.data):
        return hip_lib.covest_sample_reads_device(-1, bases.ctypes.data, offs, n, L, first, factor, 1, out.ctypes.data, out_offs,
                                                  None, cnt, None)

    for fn in (host, device):
        for bad in (0.999, 0.0, -3.0, float("nan"), float("inf")):
            assert fn(factor=bad) == -1, bad
        assert fn(n=-1) == -1 and fn(first=-1) == -1
        assert fn(L=-1) == -1
        assert fn(n=1 << 62, L=100) == -1 and fn(n=8, first=(1 << 63) - 4) == -1
        assert fn(offs=offsets.ctypes.data) == -1                       # offsets without out_offsets
    assert b"out" in hip_lib.covest_last_error()
    assert device(cnt=None) == -1 and host(nk=None) == -1
    bad_offsets = offsets.copy()
    bad_offsets[3] = 5
    assert host(offs=bad_offsets.ctypes.data, out_offs=out_offsets.ctypes.data) == -1
    assert b"descend" in hip_lib.covest_last_error()
    assert host(n=0, out_offs=out_offsets.ctypes.data) == 0
    assert (n_kept.value, n_bases.value, out_offsets[0]) == (0, 0, 0) and (out_offsets[1:] == -1).all()
    assert host(n=0, L=-1, offs=offsets.ctypes.data, out_offs=out_offsets.ctypes.data) == 0
    assert not out.any() and (counts == -1).all()


def test_the_shared_checks_word_their_messages_as_before(hip_lib):
    """The texts of the checks covest_sample_reads*, covest_split_reads* and covest_simulate_reads* share
    (csrc/reads_args.h), byte for byte as each entry point worded them on its own; the factor is looked at first."""
    bases = np.full(64, 65, dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    offsets = np.arange(9, dtype=np.int64) * 8
    out_offsets = np.full(9, -1, dtype=np.int64)
    counts = np.full(2, -1, dtype=np.int64)
    n_kept, n_bases = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def host(n=8, L=8, first=0, factor=2.0, offs=None, out_offs=None):
        return hip_lib.covest_sample_reads(-1, bases.ctypes.data, offs, n, L, first, factor, 1, out.ctypes.data, out_offs, None,
                                           ctypes.byref(n_kept), ctypes.byref(n_bases))

    def device(n=8, L=8, first=0, factor=2.0, offs=None, out_offs=None):
        return hip_lib.covest_sample_reads_device(-1, bases.ctypes.data, offs, n, L, first, factor, 1, out.ctypes.data, out_offs,
                                                  None, counts.ctypes.data, None)

    def said(status):
        assert status == -1
        return hip_lib.covest_last_error().decode()

    for fn, name in ((host, "covest_sample_reads"), (device, "covest_sample_reads_device")):
        assert said(fn(n=-1, factor=0.5)) == name + ": factor must be a finite number, at least 1"
        assert said(fn(n=-1, L=-1)) == name + ": n_reads and first_read must not be negative"
        assert said(fn(first=-1)) == name + ": n_reads and first_read must not be negative"
        assert said(fn(L=-1, first=(1 << 63) - 4)) == name + ": without offsets read_len must not be negative"
        assert said(fn(first=(1 << 63) - 8)) == name + ": more reads than 64-bit offsets reach"
        assert said(fn(n=1 << 62, L=100)) == name + ": more reads than 64-bit offsets reach"
        assert said(fn(offs=offsets.ctypes.data)) == name + ": reads of their own lengths need an array for the output offsets"
    bad = offsets.copy()
    bad[3] = 5
    assert said(host(offs=bad.ctypes.data, out_offs=out_offsets.ctypes.data)) == "covest_sample_reads: offsets descend at read 2"
    bad = offsets - 1
    assert said(host(offs=bad.ctypes.data, out_offs=out_offsets.ctypes.data)) == "covest_sample_reads: negative offset"
    genome = np.full(64, ord("A"), dtype=np.uint8)
    assert hip_lib.covest_simulate_reads(-1, genome.ctypes.data, 64, 8, (1 << 63) - 4, 8, 0.0, 1, 0, out.ctypes.data, None) == -1
    assert hip_lib.covest_last_error().decode() == "covest_simulate_reads: more reads than 64-bit offsets reach"
    assert hip_lib.covest_simulate_reads(-1, genome.ctypes.data, 64, 8, 0, 1 << 61, 0.0, 1, 0, out.ctypes.data, None) == -1
    assert hip_lib.covest_last_error().decode() == "covest_simulate_reads: more reads than 64-bit offsets reach"


def test_no_cpu_path(hip_lib, tmp_path):
    from covest_amd import _capi, sample
    if hip_lib.covest_device_count() > 0:
        pytest.skip("a HIP device is present")
    reads = np.full((4, 5), 65, dtype=np.uint8)
    with pytest.raises(_capi.CovestHipError):
        sample.sample_reads(reads, 2)
    with pytest.raises(_capi.CovestHipError):
        sample.sample_reads((reads.reshape(-1), np.array([0, 5, 20])), 2)
    fasta = tmp_path / "reads.fa"
    fasta.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    with pytest.raises(_capi.CovestHipError):
        sample.sampled_histogram(str(fasta), 5, 2)
    with pytest.raises(_capi.CovestHipError):
        sample.sample_reads_file(str(fasta), str(tmp_path / "out.fa"), 2)
    with pytest.raises(_capi.CovestHipError):
        sample.sample_reads_device(256, 4, 256, 256, 2, read_len=5)
