"""The plan of covest_kmer_count_reads_device as the device reports it: the smallest inputs that
take both branches of the planner -- everything looked at and 2^10 buckets, a sample and more buckets --, the one-length
probe of reads that come with offsets, and the 238-window tile of k = 31.  tests/kmer_plan_check.cpp pins the same plans
without a device; here they are what partition_info() says after a real count, and every count conserves the windows."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md 8)
sys.path.insert(0, os.environ["COVEST_REPO"])
from covest_amd import kmer_hist as kh
dev = torch.device("cuda", 0)
L = 100
gen = torch.Generator(device=dev); gen.manual_seed(41)
lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
genome = lut[torch.randint(0, 4, (200_000,), device=dev, generator=gen)]

def reads(n):
    starts = torch.randint(0, genome.numel() - L, (n,), device=dev, generator=gen)
    return genome[starts[:, None] + torch.arange(L, device=dev)[None, :]].reshape(-1).contiguous()

def count(name, bases, n, k, offsets=None):
    torch.cuda.synchronize()
    c = kh.KmerCounts(k, canonical=True, min_slots=1 << 12)
    if offsets is None:
        path = c.count_reads_device(bases.data_ptr(), n, L)
    else:
        path = c.count_reads_device(bases.data_ptr(), n, 0, d_offsets_ptr=offsets.data_ptr(), n_bases=n * L)
    assert path == "partitioned", (name, path, getattr(c, "why_not_partitioned", ""))
    h, info, distinct = c.histogram(), c.partition_info(), len(c)
    print(name, {key: info[key] for key in ("buckets", "minimizer", "sampled_1_in", "records")}, "distinct", distinct)
    assert sum(i * v for i, v in enumerate(h)) == n * (L - k + 1), (name, "windows lost or counted twice")
    assert sum(h) == distinct, name
    c.close()
    return h, info

def plan_of(info):
    return info["buckets"], info["minimizer"], info["sampled_1_in"]

small = reads(20_000)
h_a, info_a = count("(a) 20 000 reads", small, 20_000, 21)
assert plan_of(info_a) == (1024, 13, 1), info_a
h_b, info_b = count("(b) 100 000 reads", reads(100_000), 100_000, 21)
assert plan_of(info_b) == (4096, 13, 16), info_b
offsets = torch.arange(20_001, dtype=torch.int64, device=dev) * L
h_c, info_c = count("(c) (a) with offsets", small, 20_000, 21, offsets=offsets)
assert plan_of(info_c) == plan_of(info_a) and info_c["records"] == info_a["records"], (info_a, info_c)
assert h_c == h_a, "(c): the histogram of the same bytes differs"
count("(d) k = 31", small, 20_000, 31)
print("plan ok")
"""


def test_plans_as_the_device_reports_them(hip_lib):
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and "plan ok" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
