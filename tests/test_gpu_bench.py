"""bench.py's plain run on the GPU: `--steps` is the number of timed steps, the line carries the headline alone
(what only `--full` measures stays out of it), and `--dump-outputs` writes what the last timed step computed --
the grid's finite log-likelihoods with their flat indices and the arg-min the step returned, which must be the first
minimum of -LL; every dumped number is finite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_plain_run_steps_and_dumped_outputs(tmp_path, oracle):
    out_dir = tmp_path / "outputs"
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                           "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["roofline"]["launches"] == 3
    assert line["ms_per_step"] > 0 and line["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in line
    assert "variants" not in line and "cpu_baseline" not in line

    vals = np.load(out_dir / "loglikelihoods.npy")
    index = np.load(out_dir / "loglikelihood_index.npy")
    arg = np.load(out_dir / "argmin.npy")
    for a in (vals, index, arg):
        assert a.dtype == np.float64 and np.isfinite(a).all()
    assert arg.shape == (2,) and vals.shape == index.shape and 0 < len(vals) <= line["config"]["grid_points"]
    assert np.all(np.diff(index) > 0) and index[-1] < line["config"]["grid_points"]
    ll = np.full(line["config"]["grid_points"], -np.inf)  # the points left out have LL -inf (or NaN)
    ll[index.astype(np.int64)] = vals
    want_idx, want_min = oracle.first_min(-ll)
    assert int(arg[1]) == want_idx == line["argmin"]["flat_index"]
    assert arg[0] == want_min == line["argmin"]["min_negll"]
