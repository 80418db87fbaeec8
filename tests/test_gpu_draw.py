"""Replicate histograms drawn on the device (draw_hist.hip) against the numpy restatement of the
definition (tests/draw_reference.py): exact integers, every row summing to n -- over the cell counts either side of each
boundary between the kernel's paths, the draw counts either side of a workgroup's chunk, replicate windows, seeds and
degenerate weights; the device form on a stream of its own; one distributional check."""
import os
import subprocess
import sys

import numpy as np
import pytest

import draw_reference as ref
from conftest import load_hist

pytestmark = pytest.mark.gpu

SEED = (0x5eed << 32) | 0x0d12a3


def _weights(m, seed=1):
    """m weights over six decades, a tenth of them zero, one cell a tenth of the total (the modal cell of a model
    histogram) -- never all zero."""
    rng = np.random.default_rng(1000 * seed + m)
    w = 10.0 ** rng.uniform(-6, 0, m)
    w[rng.random(m) < 0.1] = 0.0
    w[m // 3] = max(w.sum() / 9.0, 1.0)
    return w


def _check(w, n, reps=1, seed=SEED, first=0):
    from covest_amd import draw_histograms
    got = draw_histograms(w, n, reps, seed=seed, first_replicate=first)
    want = ref.draw_histograms(w, n, reps, seed=seed, first_replicate=first)
    assert got.dtype == np.int64 and got.shape == (reps, len(w))
    assert (got.sum(axis=1) == n).all()
    assert np.array_equal(got, want), (len(w), n, reps, seed, first, np.flatnonzero((got != want).any(axis=0))[:8])
    return got


def _boundary_cells():
    from covest_amd import bootstrap as bs
    cells = [1, 2, 3, 64, 65, 257]
    for edge in (bs.GUIDE_SIZE, bs.LDS_BOTH_CELLS, bs.LDS_THRESHOLD_CELLS):
        cells += [edge - 1, edge, edge + 1]
    cells += [bs.GUIDE_SIZE + 2, bs.MAX_CELLS - 1, bs.MAX_CELLS]  # (m - 1 thresholds are searched: one more past the guide)
    return cells


@pytest.mark.parametrize("m", _boundary_cells())
def test_cell_counts_either_side_of_every_path_boundary(hip_lib, m):
    _check(_weights(m), 5001, reps=2)


def _draw_counts():
    from covest_amd.bootstrap import CHUNK_DRAWS as C
    return [0, 1, 2, 3, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1]


@pytest.mark.parametrize("n", _draw_counts())
def test_draw_counts_either_side_of_a_chunk(hip_lib, n):
    _check(_weights(257), n)
    if n in (3, 257) or n > 1000:
        _check(_weights(13000, seed=2), n)  # (counters in HBM: the other accumulation path)


def test_replicate_windows_prefixes_and_seeds(hip_lib):
    from covest_amd import draw_histograms
    w = _weights(65)
    whole = _check(w, 3000, reps=8)
    for reps in (1, 3):
        assert np.array_equal(_check(w, 3000, reps=reps, first=5), whole[5:5 + reps])
        assert np.array_equal(_check(w, 3000, reps=reps), whole[:reps])
    assert not np.array_equal(whole[0], whole[1])
    _check(w, 500, reps=3, first=(1 << 32) - 3)  # first_rep + n_rep = 2^32 is accepted
    # the prefix property: the row for n = 1000 is the row for n = 1001 less its last draw
    a, b = draw_histograms(w, 1000, 1, seed=SEED), draw_histograms(w, 1001, 1, seed=SEED)
    last = np.searchsorted(ref.thresholds(w)[:-1], ref.draws(1001, 0, SEED)[-1:], side="right")[0]
    step = np.zeros(len(w), dtype=np.int64)
    step[last] = 1
    assert np.array_equal(b[0] - a[0], step)
    for seed in (0, (1 << 63) + 5):
        _check(w, 3000, reps=2, seed=seed)
    assert not np.array_equal(draw_histograms(w, 3000, 1, seed=0), draw_histograms(w, 3000, 1, seed=(1 << 63) + 5))


def test_degenerate_weights(hip_lib):
    assert _check([1.0, 0.0], 1000)[0].tolist() == [1000, 0]
    assert _check([0.0, 1.0], 1000)[0].tolist() == [0, 1000]
    got = _check([1.0, 0.0, 0.0, 2.0, 0.0, 1.0, 0.0], 4001, reps=2)
    assert not got[:, [1, 2, 4, 6]].any() and got[:, [0, 3, 5]].all()
    rare = np.ones(9)
    rare[4] = 1e-18
    assert not _check(rare, 100_000)[:, 4].any()  # 1e-18 / 8 of 2^63 is less than one step: the cell is never hit
    assert _check([3.0], 777)[0].tolist() == [777]


def test_output_is_overwritten_not_added_to(hip_lib):
    from covest_amd import _capi
    w = _weights(300)
    want = ref.draw_histograms(w, 4000, 2, seed=SEED)
    out = np.full((2, 300), 12345, dtype=np.int64)
    for _ in range(2):  # twice into the same buffer: the same counts, not doubled
        _capi.check(hip_lib.covest_draw_histograms(-1, 300, w.ctypes.data, 4000, 0, 2, SEED, out.ctypes.data), "draw")
        assert np.array_equal(out, want)


_DEVICE_SCRIPT = r"""
import os, sys
import torch                      # first: ONE HIP runtime per process (INTEGRATION.md)
sys.path.insert(0, os.environ["COVEST_REPO"])
sys.path.insert(0, os.path.join(os.environ["COVEST_REPO"], "tests"))
import numpy as np
from covest_amd import bootstrap as bs
dev = torch.device("cuda", 0)
side = torch.cuda.Stream()
rng = np.random.default_rng(5)
for m, n, reps, first in ((300, 70_001, 3, 2), (13_000, 9_001, 2, 0), (17_000, 9_001, 2, 0)):
    w = rng.random(m) + 1e-3
    want = bs.draw_histograms(w, n, reps, seed=77, first_replicate=first)          # the host form
    t = bs.draw_thresholds(w)
    d_t = torch.from_numpy(t.view(np.int64)).to(dev)
    buf = torch.full((reps * m + 16,), -7, dtype=torch.int64, device=dev)          # eight guard words either side
    torch.cuda.synchronize()
    for _ in range(2):                                                             # the second call overwrites the first
        bs.draw_histograms_device(d_t.data_ptr(), m, n, reps, buf.data_ptr() + 64, seed=77, first_replicate=first,
                                  stream=side.cuda_stream)
    side.synchronize()
    got = buf.cpu().numpy()
    assert (got[:8] == -7).all() and (got[-8:] == -7).all(), ("stray write", m)
    assert np.array_equal(got[8:-8].reshape(reps, m), want), ("device form", m)
print("device form ok")
"""


def test_device_form_on_a_stream_of_its_own(hip_lib):
    env = dict(os.environ, COVEST_REPO=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _DEVICE_SCRIPT], env=env, capture_output=True,
                          text=True)
    assert proc.returncode == 0 and "device form ok" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]


# Seeds for which the numpy restatement itself passes the check below, with the probabilities of the CPU oracle in
# place of the device's (they agree to 1e-9 relative): run on a machine without a device before this test first ran,
# the ten cells with n p >= 25 lie at most 1.31 (seed 11) and 1.42 (seed 12) standard deviations from n p.
DISTRIBUTION_SEEDS = (11, 12)


def test_counts_follow_the_binomial_law(hip_lib):
    """n = 10^6 draws over the cells of sim_c10_e0.05.hist at (10, 0.05): every cell with n p >= 25 lies within 5
    binomial standard deviations of n p -- and the counts are the restatement's."""
    from covest_amd import BasicModel, model_cells
    model = BasicModel(21, 100, load_hist("sim_c10_e0.05"), 0, max_error=8)
    keys, w, has_tail = model_cells(model, (10.0, 0.05))
    model.close()
    assert len(w) == 15 and not has_tail
    n, p = 10 ** 6, w / np.cumsum(w)[-1]
    checked = 0
    for seed in DISTRIBUTION_SEEDS:
        got = _check(w, n, seed=seed)[0]
        for i in np.flatnonzero(n * p >= 25):
            sd = np.sqrt(n * p[i] * (1 - p[i]))
            print("seed %d cell %d: %d draws, expected %.1f, %.2f sd" % (seed, keys[i], got[i], n * p[i], (got[i] - n * p[i]) / sd))
            assert abs(got[i] - n * p[i]) <= 5 * sd, (seed, int(keys[i]))
            checked += 1
    assert checked == 2 * 10
