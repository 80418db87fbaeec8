"""The stable G-way split of the packed reads on the device (split_reads.hip through covest_amd.sample and the C ABI)
against its numpy restatement (tests/split_reference.py): bases, offsets, read indices and group starts equal byte for
byte, whatever the number of reads and of groups, the read lengths, the alignment of either buffer or the chunk of the
run; nothing written outside the stated ranges; the error codes as include/covest_amd.h states them.

Host forms run in this process (numpy buffers).  What needs device buffers of a chosen alignment runs in ONE fresh child
process with torch imported first (one HIP runtime a process), as tests/test_gpu_sample.py does.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import split_reference as ref

pytestmark = pytest.mark.gpu

SEED = (0x5a3d << 32) | 0x0badcafe   # both key words in use
GROUPS = (1, 2, 3, 64, 65, 255, 256)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def ragged(n, seed=20241019):
    """(bases, offsets) of n reads: lengths 0 .. 300 with a run of 300 empty reads and one read longer than a tile."""
    rng = np.random.default_rng(seed)
    lens = rng.choice((0, 1, 2, 5, 16, 17, 100, 300), size=n)
    if n > 700:
        lens[200:500] = 0
        lens[600] = 5000
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return rng.choice(ACGT, size=int(offsets[-1])), offsets


def check_host(reads, layout, groups, seed, first_read=0):
    """split_reads against the restatement; returns the SplitReads."""
    from covest_amd import sample
    got = sample.split_reads(reads, groups, seed=seed, first_read=first_read)
    blob = reads[0] if isinstance(reads, tuple) else reads
    want = ref.split(blob, layout, first_read, groups, seed)
    assert np.array_equal(np.ascontiguousarray(got.bases).reshape(-1), want[0]), (groups, "bases")
    assert np.array_equal(got.offsets, want[1]), (groups, "offsets")
    assert np.array_equal(got.read_index, want[2]), (groups, "read_index")
    assert np.array_equal(got.group_first, want[3]), (groups, "group_first")
    return got


@pytest.mark.parametrize("groups", GROUPS)
def test_host_form_ragged_and_fixed(hip_lib, groups):
    from covest_amd import sample
    bases, offsets = ragged(1500)
    got = check_host((bases, offsets), offsets, groups, SEED, first_read=(1 << 32) - 3)
    if groups == 1:  # one group: the output is the input
        assert np.array_equal(got.bases, bases) and np.array_equal(got.offsets, offsets)
    for g in range(groups):  # group(g): the group's reads, offsets from 0
        b, o = got.group(g)
        lo, hi = got.group_first[g], got.group_first[g + 1]
        assert o[0] == 0 and o.size == hi - lo + 1 and np.array_equal(b, got.bases[got.offsets[lo]:got.offsets[hi]])
    reads = np.random.default_rng(2).choice(ACGT, size=(sample.SPLIT_SHARE + 1, 7))
    got = check_host(reads, 7, groups, SEED)
    assert got.bases.shape == reads.shape and np.array_equal(got.bases, reads[got.read_index])
    assert sum(len(got.group(g)) for g in range(groups)) == len(reads)
    # fewer reads than groups: empty groups are legal
    few = check_host(reads[:3], 7, groups, SEED)
    assert (np.diff(few.group_first) >= 0).all() and few.group_first[-1] == 3


def test_read_groups_chunks_and_no_reads(hip_lib):
    from covest_amd import sample
    first = (1 << 32) - 3
    n = 2 * sample.SPLIT_SHARE + 1
    for groups in (2, 32, 256):
        whole = sample.read_groups(n, groups, seed=SEED, first_read=first)
        assert np.array_equal(whole, ref.groups_of(first, n, groups, SEED)), groups
        for a, m in ((0, 1), (1, 1024), (1023, 1026), (n - 1, 1)):  # a chunk [a, a + m) with first_read = a
            assert np.array_equal(sample.read_groups(m, groups, seed=SEED, first_read=first + a), whole[a:a + m]), (groups, a)
    assert not np.array_equal(sample.read_groups(n, 32, seed=SEED + 1), sample.read_groups(n, 32, seed=SEED))
    assert sample.read_groups(0, 5).size == 0
    got = sample.split_reads(np.zeros((0, 9), dtype=np.uint8), 5)
    assert got.group_first.tolist() == [0] * 6 and got.offsets.tolist() == [0] and got.bases.shape == (0, 9)
    got = sample.split_reads((np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)), 256)
    assert got.group_first.tolist() == [0] * 257 and got.offsets.tolist() == [0]
    empties = check_host((np.zeros(0, dtype=np.uint8), np.zeros(1001, dtype=np.int64)), np.zeros(1001, dtype=np.int64), 3, SEED)
    assert empties.n_reads == 1000 and empties.offsets.tolist() == [0] * 1001


def test_simulated_reads_in(hip_lib):
    from covest_amd import sample, simulate as sim
    g = sim.random_genome(20_000, 3)
    reads = sim.simulate_reads(g, 100, n_reads=3000, error_rate=0.05, seed=3, first_read=77)
    got = sample.split_reads(reads, 4, seed=3)          # numbered from the reads' own first_read
    want = ref.split(reads.bases, 100, 77, 4, 3)
    assert np.array_equal(got.read_index, want[2]) and np.array_equal(got.bases.reshape(-1), want[0])
    assert np.array_equal(got.group_first, want[3])


def test_error_codes(hip_lib):
    """COVEST_E_INVALID as the header states it, from the C ABI itself (the Python layer raises ValueError earlier)."""
    from covest_amd import _capi
    L = _capi.lib()
    bases = np.full(64, ord("A"), dtype=np.uint8)
    out = np.zeros(64, dtype=np.uint8)
    offsets = np.arange(9, dtype=np.int64) * 8
    index, out_off = np.zeros(8, dtype=np.int64), np.zeros(9, dtype=np.int64)
    first = np.full(260, -7, dtype=np.int64)

    def host(groups=4, n=8, read_len=8, first_read=0, offs=None, out_offs=out_off.ctypes.data, gf=first.ctypes.data):
        return L.covest_split_reads(-1, bases.ctypes.data, offs, n, read_len, first_read, groups, 1, out.ctypes.data, out_offs,
                                    index.ctypes.data, gf)

    def device(groups=4, n=8, read_len=8, first_read=0, offs=None, out_offs=None, gf=16):
        # (refused before any pointer is looked at: the addresses are never used)
        return L.covest_split_reads_device(-1, 16, offs, n, read_len, first_read, groups, 1, 16, out_offs, None, gf, None)

    assert host() == 0 and first[:5].tolist()[-1] == 8 and (first[5:] == -7).all()
    for call in (host, device):
        assert call(groups=0) == _capi.COVEST_E_INVALID and "groups" in _capi.last_error()
        assert call(groups=257) == _capi.COVEST_E_INVALID
        assert call(groups=-1) == _capi.COVEST_E_INVALID
        assert call(n=-1) == _capi.COVEST_E_INVALID
        assert call(first_read=-1) == _capi.COVEST_E_INVALID
        assert call(read_len=-1) == _capi.COVEST_E_INVALID
        assert call(offs=offsets.ctypes.data, out_offs=None) == _capi.COVEST_E_INVALID and "offsets" in _capi.last_error()
        assert call(gf=None) == _capi.COVEST_E_INVALID and "group_first" in _capi.last_error()
    bad = offsets.copy()
    bad[3] = 5                                            # the host form looks at the offsets
    assert host(offs=bad.ctypes.data) == _capi.COVEST_E_INVALID and "descend" in _capi.last_error()
    assert host(offs=offsets.ctypes.data) == 0 and np.array_equal(out_off, offsets)
    with pytest.raises(_capi.CovestHipError):
        _capi.check(host(groups=0), "covest_split_reads")


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import numpy as np
import split_reference as ref
from covest_amd import sample
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
SEED = (0x5a3d << 32) | 0x0badcafe
PAT, WPAT = 0xA5, -0x0123456789abcdef
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GROUPS = (1, 2, 3, 64, 65, 255, 256)
S, PASS = sample.SPLIT_SHARE, sample.SPLIT_SCAN_PASS
rng = np.random.default_rng(99)


def run(blob, offsets, L, n, first, G, seed, s_shift, d_shift, where, with_index=True, with_out_off=True):
    # one device call between sentinels, every output against the restatement
    total = blob.size
    src = torch.full((64 + s_shift + total + 64,), PAT, dtype=torch.uint8, device=dev)
    if total:
        src[64 + s_shift:64 + s_shift + total] = torch.from_numpy(blob).to(dev)
    dst = torch.full((64 + d_shift + total + 64,), PAT, dtype=torch.uint8, device=dev)
    d_out_off = torch.full((n + 3,), WPAT, dtype=torch.int64, device=dev)
    d_index = torch.full((n + 2,), WPAT, dtype=torch.int64, device=dev)
    d_first = torch.full((G + 3,), WPAT, dtype=torch.int64, device=dev)
    d_off = torch.from_numpy(offsets).to(dev) if offsets is not None else None
    sample.split_reads_device(src.data_ptr() + 64 + s_shift, n, dst.data_ptr() + 64 + d_shift, d_first.data_ptr() + 8, G,
                              seed=seed, first_read=first, read_len=L, offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                              out_offsets_ptr=d_out_off.data_ptr() + 8 if with_out_off else None,
                              read_index_ptr=d_index.data_ptr() + 8 if with_index else None, stream=stream)
    torch.cuda.synchronize()
    layout = offsets if offsets is not None else L if L > 0 else np.zeros(n + 1, dtype=np.int64)
    want_bases, want_off, want_index, want_first = ref.split(blob, layout, first, G, seed)
    f, o, i, b, s = d_first.cpu().numpy(), d_out_off.cpu().numpy(), d_index.cpu().numpy(), dst.cpu().numpy(), src.cpu().numpy()
    assert np.array_equal(f[1:G + 2], want_first) and f[0] == WPAT and f[G + 2] == WPAT, ("group_first", where)
    if with_out_off:
        assert np.array_equal(o[1:n + 2], want_off) and o[0] == WPAT and o[n + 2] == WPAT, ("offsets", where)
    else:
        assert (o == WPAT).all(), ("offsets written", where)
    if with_index:
        assert np.array_equal(i[1:n + 1], want_index) and i[0] == WPAT and i[n + 1] == WPAT, ("read_index", where)
    else:
        assert (i == WPAT).all(), ("read_index written", where)
    at, nb = 64 + d_shift, want_bases.size
    assert np.array_equal(b[at:at + nb], want_bases), ("bases", where)
    assert (b[:at] == PAT).all() and (b[at + nb:] == PAT).all(), ("stray byte", where)
    assert (s[:64 + s_shift] == PAT).all() and (s[64 + s_shift + total:] == PAT).all(), ("source", where)


# reads of one length: every read count round the share of a workgroup at every number of groups (G > n: empty groups);
# source and destination 0 .. 3 bytes off a 16-byte boundary, never the same for both
SHIFTS = ((0, 1), (1, 2), (2, 3), (3, 0), (1, 3), (3, 1), (2, 0), (0, 3))
case = 0
for L in (1, 7, 100):
    for n in (1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1):
        for G in GROUPS:
            s_shift, d_shift = SHIFTS[case % len(SHIFTS)]
            run(rng.choice(ACGT, size=n * L), None, L, n, 3, G, SEED, s_shift, d_shift, (L, n, G, s_shift, d_shift),
                with_index=case % 3 != 0, with_out_off=case % 2 == 0)
            case += 1
run(np.zeros(0, np.uint8), None, 0, 300, 3, 5, SEED, 1, 3, "fixed length 0")
print("fixed ok")

# more workgroups than one pass of a group's scan holds
n = S * PASS + S + 1
run(rng.choice(ACGT, size=n), None, 1, n, 5, 255, SEED, 3, 1, "rows of more than one pass")
print("long rows ok")

# ragged reads with empty reads, a run of 300 empty ones and one read longer than a tile, read indices across 2^32
lens = rng.choice((0, 1, 2, 5, 16, 17, 100, 300), size=2 * S + 77)
lens[900:1200] = 0
lens[1500] = 5000
offsets = np.zeros(lens.size + 1, dtype=np.int64); np.cumsum(lens, out=offsets[1:])
blob = rng.choice(ACGT, size=int(offsets[-1]))
case = 0
for G in GROUPS:
    for s_shift, d_shift in (SHIFTS if G == 65 else (SHIFTS[case % len(SHIFTS)], SHIFTS[(case + 3) % len(SHIFTS)])):
        run(blob, offsets, 0, lens.size, (1 << 32) - 3, G, SEED, s_shift, d_shift, ("ragged", G, s_shift, d_shift),
            with_index=case % 2 == 0)
        case += 1
# a source that does not start at offset 0 of its buffer
run(np.concatenate([np.full(37, 0x58, np.uint8), blob]), offsets + 37, 0, lens.size, 0, 7, SEED, 3, 2, "offsets from 37")
print("ragged ok")

# n_reads == 0: group_first[0 .. G] = 0, out_offsets[0] = 0, nothing else
d_first = torch.full((8,), WPAT, dtype=torch.int64, device=dev)
d_o = torch.full((3,), WPAT, dtype=torch.int64, device=dev)
sample.split_reads_device(0, 0, 0, d_first.data_ptr() + 8, 5, read_len=5, out_offsets_ptr=d_o.data_ptr() + 8, stream=stream)
torch.cuda.synchronize()
assert d_first.cpu().tolist() == [WPAT, 0, 0, 0, 0, 0, 0, WPAT] and d_o.cpu().tolist() == [WPAT, 0, WPAT], "n_reads == 0"
print("device forms ok")
"""


def test_device_forms(hip_lib):
    """Raw device pointers (torch tensors): reads of length 1, 7 and 100 at every read count round a workgroup's share
    and every number of groups, rows longer than one pass of the scan, ragged reads at misalignments 0 .. 3 with read
    indices across 2^32, NULL read_index / out_offsets, n_reads == 0; guard bytes round every output unchanged."""
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "device forms ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]
