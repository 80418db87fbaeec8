"""Every k the partitioned k-mer counter takes, k = 19 .. 31, in both strand modes, against the oracle (DESIGN.md section
6ad): the other tests pin exact histograms at k = 19 .. 26, 28, 30 and 31 only, and k = 30 -- the one k with the
239-window tile -- only ragged and forward.  Two small seeded inputs made on the host, chosen so that at every k runs
cross wave and tile boundaries (reads of 600, 300 and 100 bases over tiles of 238 to 240 windows), a run is longer than a
record holds ("A" * 300, "AC" * 150, "ACG" * 100: one minimizer throughout), the windows' halo is read, and reads
shorter than k go through their own kernel (k - 1 bases, and none); the reads of one length are counted through both
layouts.  One child process, torch imported first."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md 8)
sys.path.insert(0, os.environ["COVEST_REPO"])
import numpy as np
from covest_amd import kmer_hist as kh
from oracle import kmer_oracle as ko
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1931)
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)

def text(codes):
    return LUT[codes].tobytes().decode()

def random_read(n):
    return text(rng.integers(0, 4, size=n, dtype=np.uint8))

genome = rng.integers(0, 4, size=2000, dtype=np.uint8)
def genome_reads(n, L):
    return [text(genome[s:s + L]) for s in rng.integers(0, genome.size - L, size=n)]

def revcomp(read):
    return read[::-1].translate(str.maketrans("ACGT", "TGCA"))

def count(name, reads, k, canonical, fixed_len):
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    offs = np.zeros(len(reads) + 1, dtype=np.int64); np.cumsum(lens, out=offs[1:])
    d_bases, d_offs = torch.from_numpy(blob.copy()).to(dev), torch.from_numpy(offs).to(dev)
    want = ko.histogram(reads, k, canonical=canonical)
    want_distinct = len(ko.count_kmers(reads, k, canonical=canonical)[0])
    windows = int(np.maximum(lens - k + 1, 1).sum())
    for layout in (("fixed",) if fixed_len else ()) + ("offsets",):
        c = kh.KmerCounts(k, canonical=canonical, min_slots=1 << 12)
        if layout == "fixed":
            path = c.count_reads_device(d_bases.data_ptr(), len(reads), fixed_len)
        else:
            path = c.count_reads_device(d_bases.data_ptr(), len(reads), 0, d_offsets_ptr=d_offs.data_ptr(), n_bases=int(offs[-1]))
        where = (name, layout, k, canonical)
        assert path == "partitioned", (where, path, getattr(c, "why_not_partitioned", ""))
        got = c.histogram()
        assert got == want, (where, got[:8], want[:8])
        assert len(c) == want_distinct, (where, len(c), want_distinct)
        assert sum(i * v for i, v in enumerate(got)) == windows, (where, "windows lost or counted twice")
        c.close()

one = random_read(600)
fixed = [random_read(300) for _ in range(20)] + ["A" * 300, "AC" * 150, "ACG" * 100] + genome_reads(30, 300)
n_counts = 0
for k in range(19, 32):
    ragged = ([one, revcomp(one), "A" * 300, "AC" * 150, random_read(k - 1), random_read(k), random_read(k + 1), ""]
              + genome_reads(40, 100))
    for canonical in (False, True):
        count("ragged", ragged, k, canonical, None)
        count("fixed", fixed, k, canonical, 300)
        n_counts += 3
print("every k ok:", n_counts, "counts")
"""


def test_every_k_both_strand_modes_both_layouts(hip_lib):
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "every k ok: 78 counts" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
