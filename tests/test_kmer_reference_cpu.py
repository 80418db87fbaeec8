"""The second k-mer reference (tests/kmer_reference.py) against the oracle (oracle/kmer_oracle.py) on every input
tests/test_gpu_kmer_widths.py counts, and against the golden vectors generated from the reference's own
bin/kmer_hist.py.  The two restatements share no code: where they agree, the device is compared with either.
CPU only; exact integer equality."""
import pytest

import kmer_reference as kr
from conftest import load_golden
from test_gpu_kmer_widths import K_SWEEP


def _agree(reads, k, what, histograms=False):
    """The same keys with the same counts, both strand modes (the oracle's per-window loop is the slow side: it is
    run once per mode); with `histograms` also the two count-of-counts functions."""
    from oracle import kmer_oracle as ko
    reads = list(reads)
    for canonical in (False, True):
        keys, occurrences = ko.count_kmers(reads, k, canonical=canonical)
        assert kr.count(reads, k, canonical) == {int(a): int(b) for a, b in zip(keys, occurrences)}, (what, k, canonical)
        if histograms:
            assert kr.histogram(reads, k, canonical) == (ko.histogram(reads, k, canonical=canonical), len(keys)), (what, k)


def test_golden_vectors():
    g = load_golden("kmer_hist.json")
    for c in g["cases"]:
        reads = [kr.preprocess(r, c["nstrategy"]) for r in c["reads"]]
        assert kr.histogram(reads, c["k"]) == (c["hist"], c["distinct"]), c["name"]
    for h in g["helpers"]:
        k = len(h["kmer"])
        assert list(kr.count([h["kmer"]], k)) == [h["hash"]]
        for b, name in (("a", "rehash_a"), ("t", "rehash_t")):
            assert sorted(kr.count([h["kmer"] + b], k)) == sorted({h["hash"], h[name]})
    with pytest.raises(KeyError):
        kr.histogram(["acgtx"], 3)


def test_k_sweep_is_the_issue_list():
    want = set()
    for part in ("1 2 3 4 5 7 8 9", "12 13 14", "15 16 17", "20 21 24 25", "28 29 30 31 32 33", "47 48 49",
                 "62 63 64 65", "95 96 97", "126 127 128 129", "159 160 161", "191 192 193", "223 224 225", "254 255"):
        want.update(int(v) for v in part.split())
    assert sorted(want) == list(K_SWEEP) and len(K_SWEEP) == 49


def test_sweep_inputs():
    """(a): every length of the list is there six times, and the batches are the reads."""
    for k in K_SWEEP:
        reads = kr.sweep_reads(k)
        lens = sorted(len(r) for r in reads)
        assert all(lens.count(n) >= 6 for n in kr.sweep_lengths(k)), k
        assert any(r.islower() for r in reads if r) and any(r.isupper() for r in reads if r)
        assert sum(kr.sweep_batches(k), []) == list(reads) and all(kr.sweep_batches(k))
        _agree(reads, k, "sweep")


def test_probe_inputs():
    """(b): the positions hold both sides of every word boundary from either end, B and B' differ in one base."""
    for k in K_SWEEP:
        ps = kr.probe_positions(k)
        assert {p for p in (0, 1, k - 2, k - 1) if 0 <= p < k} <= set(ps) and ps == sorted(set(ps)) and 0 <= ps[0] and ps[-1] < k
        for m in range(1, 8):
            for p in (32 * m - 1, 32 * m, 32 * m + 1):
                if p < k:
                    assert p in ps and k - 1 - p in ps, (k, p)
        reads = kr.probe_reads(k)
        assert len(reads) == 6 * len(ps) + (3 if k in kr.PALINDROME_K else 0)
        for i, p in enumerate(ps):
            b, b2 = reads[6 * i], reads[6 * i + 3]
            assert [j for j in range(k) if b[j] != b2[j]] == [p]
            assert reads[6 * i + 1].endswith(b) and reads[6 * i + 2].startswith(b)
        if k in kr.PALINDROME_K:
            assert kr.revcomp(reads[-3]) == reads[-3] and kr.revcomp(reads[-2]) == reads[-1]
        _agree(reads, k, "probe")
    assert set(kr.PALINDROME_K) <= set(K_SWEEP)


def test_lane_bin_device_and_file_inputs():
    for k in kr.LANES_K:
        _agree(kr.lanes_reads(k), k, "lanes", histograms=True)
        hist, distinct = kr.histogram(kr.lanes_reads(k)[:3], k, canonical=True)
        assert distinct == 3 and hist[201 + 71] == 1          # poly-A and poly-T are one canonical key, AC gives two
    for k in kr.BINS_K:
        reads = kr.bins_reads(k)
        _agree(reads, k, "bins")
        hist, _ = kr.histogram(reads, k)
        assert len(hist) == 4098 and [hist[n] for n in kr.BINS_COUNTS] == [1, 1, 1]
        hist2, _ = kr.histogram(reads + reads, k)
        assert [hist2[2 * n] for n in kr.BINS_COUNTS] == [1, 1, 1] and len(hist2) == 2 * 4097 + 1
    for k in kr.DEVICE_K:
        for length in kr.device_lengths(k):
            _agree(kr.device_fixed_reads(k, length), k, "device fixed")
        ragged = kr.device_ragged_reads(k)
        assert len(ragged) == 300 and "" in ragged and any(len(r) == k - 1 for r in ragged)
        assert max(map(len, ragged)) <= k + 130
        _agree(ragged, k, "device ragged")
        _agree([r[:k - 1] for r in kr.device_fixed_reads(k, k)], k, "one base short")
    text = kr.fasta_text()
    assert max(map(len, text.splitlines())) <= kr.FASTA_LINE and "N" in text and "n" in text
    for k in kr.FILE_K:
        for strategy in (kr.NS_IGNORE, kr.NS_SINGLE):
            reads = [kr.preprocess(seq, strategy) for _, seq in kr.fasta_records()]
            assert any(len(r) < k for r in reads) and "" in [kr.preprocess(s, kr.NS_IGNORE) for _, s in kr.fasta_records()]
            _agree(reads, k, "fasta")


def test_fasta_records_through_the_reader(tmp_path):
    """(f): the library's reader hands the counter the reads the reference is given."""
    from covest_amd import kmer_hist as kh
    fa = tmp_path / "reads.fa"
    fa.write_text(kr.fasta_text())
    for strategy, own in ((kh.NS_IGNORE, kr.NS_IGNORE), (kh.NS_SINGLE, kr.NS_SINGLE)):
        assert list(kh.load_reads(str(fa), strategy)) == [kr.preprocess(seq, own) for _, seq in kr.fasta_records()]


def test_short_reads_and_strands_by_hand():
    """Small cases worked out by hand (a=0 c=1 g=2 t=3)."""
    assert kr.count(["", "ac", "ACGTA"], 5) == {0: 1, 1: 1, 0b0001101100: 1}
    # "ac" zero-extended to aaaac; its reverse complement gtttt = 2 3 3 3 3
    assert kr.count(["ac"], 5, canonical=True) == {1: 1}
    assert kr.count(["tt"], 3, canonical=True) == {0b000011: 1}  # att -> aat, both 3 digits: min(15, 3)
    assert kr.count([""], 3, canonical=True) == {0: 1}
    assert kr.count(["acg", "cgt"], 3, canonical=True) == {0b000110: 2}  # cgt is acg's reverse complement
    assert kr.histogram([], 4) == ([0], 0)
    assert kr.histogram(["aaaaaa", "AAAA"], 4) == ([0, 0, 0, 0, 1], 1)
