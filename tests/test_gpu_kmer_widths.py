"""The two table counters (kmer_count.hip, k <= 31; kmer_wide.hip, keys of 2, 4 and 8 words) at every key width and
on both sides of every change of code path, k = 1 .. 255, against tests/kmer_reference.py -- a restatement that
shares no code with the oracle and is held against it, and against the reference's own vectors, by
tests/test_kmer_reference_cpu.py.  Exact integer equality throughout: histogram and distinct count.

  (a) test_width_sweep            reads of every length that changes the lane loop's rounds or window_codes' switch
                                  to bytes, through the host entry, into a table that has to grow; counted twice;
                                  cleared and counted again
  (b) test_key_position_probes    k-mers that differ in ONE base, at the ends and around every word boundary of
                                  the key, alone and embedded: a word dropped or garbled merges them, a mask
                                  missing or misplaced splits a k-mer from its embedded copies
  (c) test_one_key_in_every_lane  low-complexity reads: 64 lanes insert the same new key at once
  (d) test_histogram_bins_and_rehash  counts 4095, 4096, 4097 (the histogram kernel's LDS bins end at 4096), and
                                  covest_kmer_reserve carrying them into a larger table
  (e) test_device_resident_entries    covest_kmer_add_device with a read length and with offsets, wide k included
  (f) test_file_front_end_beyond_31   kmer_hist.main on a FASTA file with Ns and wrapped lines, k = 40 and 150
"""
import pytest

import kmer_reference as kr

pytestmark = pytest.mark.gpu

K_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9,
           12, 13, 14,            # has_first_slot turns on at 13
           15, 16, 17,
           20, 21, 24, 25,
           28, 29, 30, 31, 32, 33,  # one word | two words
           47, 48, 49,
           62, 63, 64, 65,        # two words | four
           95, 96, 97,
           126, 127, 128, 129,    # four words | eight
           159, 160, 161,
           191, 192, 193,
           223, 224, 225,
           254, 255)              # 255 leaves two bits of the top word


def _check(counts, reads, what):
    want, distinct = kr.histogram(reads, counts.k, counts.canonical)
    assert counts.histogram() == want, what
    assert len(counts) == distinct, what
    return want, distinct


def test_width_sweep(hip_lib):
    from covest_amd import kmer_hist as kh
    ran = 0
    for k in K_SWEEP:
        batches = kr.sweep_batches(k)
        reads = list(kr.sweep_reads(k))
        for canonical in (False, True):
            what = ("sweep", k, canonical)
            counts = kh.KmerCounts(k, canonical, min_slots=1024)
            for batch in batches:
                counts.add_reads(batch)
            h, distinct = _check(counts, reads, what)
            if distinct > 512:  # (decided by the reference, not by the device) the table had to grow
                assert counts.slots > 1024, what
            counts.add_reads(reads)  # everything a second time: every count doubles, no key is new
            h2 = counts.histogram()
            assert h2[0::2] == h and not any(h2[1::2]) and len(counts) == distinct, what
            counts.clear()
            assert counts.histogram() == [0] and len(counts) == 0, what
            counts.add_reads(reads)
            assert counts.histogram() == h and len(counts) == distinct, what
            counts.close()
            ran += 1
    print("width sweep: %d (k, strand) combinations" % ran)
    assert ran == len(K_SWEEP) * 2


def test_key_position_probes(hip_lib):
    from covest_amd import kmer_hist as kh
    ran = 0
    for k in K_SWEEP:  # (k = 1 has the one position 0)
        reads = list(kr.probe_reads(k))
        for canonical in (False, True):
            counts = kh.KmerCounts(k, canonical, min_slots=1024)
            counts.add_reads(reads)
            _check(counts, reads, ("probes", k, canonical))
            counts.close()
            ran += 1
    print("key-position probes: %d (k, strand) combinations" % ran)
    assert ran == len(K_SWEEP) * 2


@pytest.mark.parametrize("canonical", [False, True])
def test_one_key_in_every_lane(hip_lib, canonical):
    """A failure here is COVEST_E_NOMEM (the spin of wide_add is bounded) or a wrong histogram, never a hang."""
    from covest_amd import kmer_hist as kh
    for k in kr.LANES_K:
        reads = list(kr.lanes_reads(k))
        counts = kh.KmerCounts(k, canonical, min_slots=1024)
        counts.add_reads(reads)
        _check(counts, reads, ("lanes", k, canonical))
        counts.close()


@pytest.mark.parametrize("k", kr.BINS_K)
def test_histogram_bins_and_rehash(hip_lib, k):
    from covest_amd import _capi, kmer_hist as kh
    reads = list(kr.bins_reads(k))
    counts = kh.KmerCounts(k, min_slots=1024)
    counts.add_reads(reads)
    h, distinct = _check(counts, reads, ("bins", k))
    assert len(h) == 4098
    want, _ = kr.histogram(reads, k)
    assert [h[n] for n in kr.BINS_COUNTS] == [want[n] for n in kr.BINS_COUNTS] == [1, 1, 1]
    # the rehash into a larger table carries every key and its count, the large ones too
    slots = counts.slots
    _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 8 * slots), "covest_kmer_reserve")
    assert counts.slots >= 8 * slots
    assert counts.histogram() == h and len(counts) == distinct
    counts.add_reads(reads)
    h2, _ = _check(counts, reads + reads, ("bins twice", k))
    assert len(h2) == 2 * 4097 + 1 and [h2[2 * n] for n in kr.BINS_COUNTS] == [1, 1, 1]
    counts.close()


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md 8)
sys.path[:0] = [os.environ["COVEST_REPO"], os.path.join(os.environ["COVEST_REPO"], "tests")]
import numpy as np
import kmer_reference as kr
from covest_amd import kmer_hist as kh
dev = torch.device("cuda", 0)

def resident(reads, front=""):
    # the reads back to back behind `front`, and their offsets (offsets[0] = len(front)), both in HBM
    blob = np.frombuffer((front + "".join(reads)).encode(), dtype=np.uint8)
    offs = np.full(len(reads) + 1, len(front), dtype=np.int64)
    offs[1:] += np.cumsum([len(r) for r in reads], dtype=np.int64)
    d_bases = torch.from_numpy(blob.copy()).to(dev) if blob.size else torch.zeros(1, dtype=torch.uint8, device=dev)
    return d_bases, torch.from_numpy(offs).to(dev)

def check(c, want, what):
    torch.cuda.synchronize()
    assert c.histogram() == want[0], what
    assert len(c) == want[1], what
    c.close()

ran = 0
for k in kr.DEVICE_K:
    for L in kr.device_lengths(k):
        reads = kr.device_fixed_reads(k, L)
        d_bases, d_offs = resident(reads)
        for canonical in (False, True):
            want = kr.histogram(reads, k, canonical)
            c = kh.KmerCounts(k, canonical, min_slots=1024)
            c.add_device(d_bases.data_ptr(), len(reads), L)
            check(c, want, ("read_len", k, L, canonical))
            c = kh.KmerCounts(k, canonical, min_slots=1024)
            c.add_device(d_bases.data_ptr(), len(reads), L, d_offsets_ptr=d_offs.data_ptr())
            check(c, want, ("offsets", k, L, canonical))
            ran += 1
    # reads of every length from none to k + 130 bases behind a 10-byte run the offsets skip: offsets[0] = 10, and the
    # reads start at every byte alignment.  (read_len beside offsets only bounds what the wrapper reserves.)
    ragged = kr.device_ragged_reads(k)
    d_bases, d_offs = resident(ragged, front="ACGTACGTAC")
    short = [r[:k - 1] for r in kr.device_fixed_reads(k, k)]   # every read one base short of k: the hash of what there is
    d_short, _ = resident(short)
    for canonical in (False, True):
        c = kh.KmerCounts(k, canonical, min_slots=1024)
        c.add_device(d_bases.data_ptr(), len(ragged), k + 130, d_offsets_ptr=d_offs.data_ptr())
        check(c, kr.histogram(ragged, k, canonical), ("ragged", k, canonical))
        c = kh.KmerCounts(k, canonical, min_slots=1024)
        c.add_device(d_short.data_ptr(), len(short), k - 1)
        check(c, kr.histogram(short, k, canonical), ("k - 1 bases", k, canonical))
assert ran == len(kr.DEVICE_K) * 4 * 2
print("device entries ok", ran)
"""


def test_device_resident_entries(hip_lib):
    """One child process that imports torch first (one HIP runtime per process); nothing is exec'd in place."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "device entries ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


@pytest.mark.parametrize("k", kr.FILE_K)
def test_file_front_end_beyond_31(hip_lib, tmp_path, k):
    from covest_amd import kmer_hist as kh
    fa = tmp_path / "reads.fa"
    fa.write_text(kr.fasta_text())
    for strategy, own in ((kh.NS_IGNORE, kr.NS_IGNORE), (kh.NS_SINGLE, kr.NS_SINGLE)):
        reads = [kr.preprocess(seq, own) for _, seq in kr.fasta_records()]
        assert kh.main(str(fa), None, k, strategy) == kr.histogram(reads, k)[0], (k, strategy)
