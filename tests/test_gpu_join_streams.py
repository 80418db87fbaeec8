"""covest_kmer_join_histogram_device on a stream that is not the null stream (tests/stream_order.py, scheme A;
tests/test_gpu_streams.py does the same for its neighbours, and its helpers are used here).

The call says "asynchronous on `stream`", zeroes its output on that stream and must see the adds issued there before
it.  Here both counters are filled on a side stream S from bases that arrive late behind a bounded busy-wait, the join
is issued on S with NO synchronisation in between, its output lies under a guard pattern that is copied over it again
behind the delay, and only S is waited for.  A memset issued on the null stream is lost under the late pattern (the
counts are then added onto the pattern); a sweep issued there walks two empty tables and what it wrote is lost as well.
Expected values: tests/join_reference.py over tests/kmer_reference.py, exact.

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
SEED = (0x6a01 << 32) | 0x0badf00d
PAT64 = 0x25A5A5A5A5A5A5A5
N, L = 300, 100


def case_join():
    """Two counters filled on S from late bases, then the join on S: keys of 21 bases (a first slot) and of 12 (none),
    a matrix inside the LDS rectangle and one beyond it on both sides."""
    import torch
    import join_reference as jr
    import kmer_reference as kr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    import sim_reference as sr
    from test_gpu_streams import Out, run_a
    S = so.side_stream()
    genome = sr.random_genome(2000, SEED)
    reads_a = np.ascontiguousarray(sr.reads_and_origin(genome, L, 0, N, 0.02, SEED)[0], dtype=np.uint8)
    reads_b = np.ascontiguousarray(sr.reads_and_origin(genome, L, N, N, 0.02, SEED)[0], dtype=np.uint8)  # the next N reads
    strings_a, strings_b = ([bytes(r).decode("ascii") for r in reads] for reads in (reads_a, reads_b))
    blob_a, blob_b = reads_a.reshape(-1), reads_b.reshape(-1)
    d_true_a, d_true_b = so.to_device(blob_a), so.to_device(blob_b)
    for k, (rows, cols) in ((21, (40, 12)), (12, (300, 20)), (21, (1, 1))):
        name = "join: k = %d, %d x %d" % (k, rows, cols)
        want = jr.join(kr.count(strings_a, k, True), kr.count(strings_b, k, True), rows, cols)
        assert rows == 1 or (want[1:, 1:].sum() > 0 and want[0].sum() > 0 and want[1:, 0].sum() > 0), name
        d_in_a, d_in_b = so.to_device(so.other_bases(blob_a)), so.to_device(so.other_bases(blob_b))
        a, b = KmerCounts(k, canonical=True, min_slots=1 << 17), KmerCounts(k, canonical=True, min_slots=1 << 16)
        out = Out(rows * cols, torch.int64, PAT64)

        def fill_and_join(st):
            a.add_device(d_in_a.data_ptr(), N, L, stream=st, reserve=False)
            b.add_device(d_in_b.data_ptr(), N, L, stream=st, reserve=False)
            a.join_histogram_device(b, rows, cols, out.ptr, stream=st)

        def warm():
            c, d = KmerCounts(k, canonical=True, min_slots=1 << 17), KmerCounts(k, canonical=True, min_slots=1 << 16)
            scratch = Out(rows * cols, torch.int64, PAT64)
            c.add_device(d_true_a.data_ptr(), N, L, reserve=False)
            d.add_device(d_true_b.data_ptr(), N, L, reserve=False)
            c.join_histogram_device(d, rows, cols, scratch.ptr)
            torch.cuda.synchronize()
            c.close()
            d.close()
        run_a(name, S, [(d_in_a, d_true_a), (d_in_b, d_true_b), out.late()], fill_and_join, warm=warm)
        got = out.read(name).reshape(rows, cols)
        assert np.array_equal(got, want), (name, got[:4, :4], want[:4, :4])
        a.close()
        b.close()
    torch.cuda.synchronize()


CASES = {f.__name__[5:]: f for f in (case_join,)}


def _child(case):
    """One fresh child process: this file as a program, under a time limit of its own."""
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and ("%s ok" % case) in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
    return proc.stdout


def test_join_on_a_side_stream(hip_lib):
    _child("join")


test_join_on_a_side_stream.__doc__ = case_join.__doc__


if __name__ == "__main__":
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    CASES[sys.argv[1]]()
    print("%s ok" % sys.argv[1])
