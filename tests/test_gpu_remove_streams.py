"""covest_kmer_remove_device and covest_kmer_remove_weighted_device on a stream that is not the null stream
(tests/stream_order.py, scheme A; tests/test_gpu_streams.py's helpers are used here).

The calls say "asynchronous on `stream`" and must see the adds issued there before them.  Here a counter is filled on a
side stream S from bases that arrive late behind a bounded busy-wait; the removals are issued on S behind the adds with
NO synchronisation in between; the weights of the weighted removal are written late on S as well (until then they hold
other valid weights); and only S is waited for.  A removal issued on the null stream would walk an empty table with the
poison bases and underflow; one that read its weights early would take out the wrong amounts.  Expected values:
tests/remove_reference.py, exact, and no underflow.

ONE fresh child process with torch imported first (one HIP runtime a process): this file run as a
program.  Two streams, no environment variable, nothing that could fault: poison is valid input.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = (0x6b02 << 32) | 0x0badf00d
N, L = 300, 100


def case_remove():
    """Adds on S from late bases, then an unweighted removal of ranks 40 .. 179 and a weighted one of all reads with
    late weights, all on S: keys of 21 bases (a first slot) and of 12 (none)."""
    import torch
    import remove_reference as rr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from test_gpu_streams import run_a, simulated
    S = so.side_stream()
    reads, strings = simulated(2000, N, L, 0.02, SEED)
    blob = reads.reshape(-1)
    d_true = so.to_device(blob)
    w_add = np.array([(0, 1, 13, 70000)[(3 * i) % 4] for i in range(N)], dtype=np.uint32)
    w_sub = np.minimum(w_add, np.array([(13, 0, 70000, 1)[(i // 2) % 4] for i in range(N)], dtype=np.uint32))
    w_early = np.where(w_sub > 0, 0, 5).astype(np.uint32)   # valid weights, and wrong ones: read too early they show
    d_w_add, d_w_true = so.to_device(w_add), so.to_device(w_sub)
    for k in (21, 12):
        name = "remove: k = %d" % k
        ref = rr.Table(k, True).add(strings).add(strings, w_add).remove(strings[40:180]).remove(strings, w_sub)
        want_hist, want_distinct = ref.histogram()
        d_in, d_w = so.to_device(so.other_bases(blob)), so.to_device(w_early)
        counts = KmerCounts(k, canonical=True, min_slots=1 << 17)

        def fill_and_remove(st):
            counts.add_device(d_in.data_ptr(), N, L, stream=st, reserve=False)
            counts.add_weighted_device(d_in.data_ptr(), N, L, d_w_add.data_ptr(), stream=st, reserve=False)
            counts.remove_device(d_in.data_ptr() + 40 * L, 140, L, stream=st)
            counts.remove_weighted_device(d_in.data_ptr(), N, L, d_w.data_ptr(), stream=st)

        def warm():
            c = KmerCounts(k, canonical=True, min_slots=1 << 17)
            c.add_device(d_true.data_ptr(), N, L, reserve=False)
            c.add_weighted_device(d_true.data_ptr(), N, L, d_w_add.data_ptr(), reserve=False)
            c.remove_device(d_true.data_ptr() + 40 * L, 140, L)
            c.remove_weighted_device(d_true.data_ptr(), N, L, d_w_true.data_ptr())
            torch.cuda.synchronize()
            assert c.histogram() == want_hist, name + " (warm)"
            c.close()
        run_a(name, S, [(d_in, d_true), (d_w, d_w_true)], fill_and_remove, warm=warm)
        assert counts.histogram() == want_hist and len(counts) == want_distinct, name   # (raises on an underflow)
        assert counts.occupancy() == ref.occupancy(), name
        counts.close()
    torch.cuda.synchronize()


CASES = {f.__name__[5:]: f for f in (case_remove,)}


def _child(case):
    """One fresh child process: this file as a program, under a time limit of its own."""
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and ("%s ok" % case) in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
    return proc.stdout


def test_remove_on_a_side_stream(hip_lib):
    _child("remove")


test_remove_on_a_side_stream.__doc__ = case_remove.__doc__


if __name__ == "__main__":
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    CASES[sys.argv[1]]()
    print("%s ok" % sys.argv[1])
