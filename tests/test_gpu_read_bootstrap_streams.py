"""The read bootstrap's two asynchronous entry points on a stream that is not the null stream (tests/stream_order.py,
scheme A; tests/test_gpu_streams.py does the same for their neighbours, and its helpers are used here).

bootstrap_weights_device and KmerCounts.add_weighted_device say "asynchronous on `stream`".  On the null stream a launch
that lost its `stream` argument gives the right answer; here the true inputs -- the bases, the weights -- arrive late on
a side stream S behind a bounded busy-wait, the draw's output lies under a guard pattern that is copied over it again
behind the delay, and only S is waited for: work on another stream computes on the poison (other bases, other weights:
valid inputs of the same sizes) or is lost under the pattern.  The draw is followed by the weighted add with NO
synchronisation between them: the add reads on S what the draw wrote on S.  Expected values are the restatements'
(bootstrap_weights_reference, kmer_reference over the expanded reads), exact.

Each test is ONE fresh child process with torch imported first (one HIP runtime a process): this file run
as a program with the name of the case.  One GPU process at a time, two streams, no environment variable, nothing that
could fault: poison is valid input.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = (0x57e4 << 32) | 0x0badf00d   # both key words in use
PAT32 = 0x25A5A5A5
N, L = 300, 100


def as_list(reads):
    return [bytes(r).decode("ascii") for r in reads]


def case_draw():
    """bootstrap_weights_device on S: it has no input that could arrive late, so the late guard pattern is what a launch
    on the wrong stream is lost under."""
    import torch
    import bootstrap_weights_reference as bw
    import stream_order as so
    from covest_amd.read_bootstrap import bootstrap_weights_device
    from test_gpu_streams import Out, run_a
    S = so.side_stream()
    for n, first, rep in ((1000, (1 << 32) - 3, 2), (257, 0, (1 << 32) - 1)):
        out = Out(n, torch.int32, PAT32)
        run_a("read bootstrap: draw, n = %d" % n, S, [out.late()],
              lambda st: bootstrap_weights_device(out.ptr, n, rep, seed=SEED, first_read=first, stream=st),
              warm=lambda: bootstrap_weights_device(out.ptr, n, rep, seed=SEED ^ 1, first_read=first))
        assert np.array_equal(out.read("weights").view(np.uint32), bw.weights(n, rep, seed=SEED, first_read=first)), n
    torch.cuda.synchronize()


def case_weighted_add():
    """add_weighted_device on S (reserve=False: nothing waits): the bases AND the weights arrive late; keys of one word
    (both layouts: the kernel that numbers the windows through, the wave a read) and of two (k = 40)."""
    import torch
    import bootstrap_weights_reference as bw
    import kmer_reference as kr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from test_gpu_streams import run_a, simulated
    S = so.side_stream()
    reads, strings = simulated(2000, N, L, 0.02, SEED)
    blob = reads.reshape(-1)
    weights = bw.weights(N, 5, seed=SEED)
    poison = bw.weights(N, 6, seed=SEED)
    assert not np.array_equal(weights, poison) and (weights == 0).any() and (weights > 1).any()
    d_true, d_w_true = so.to_device(blob), so.to_device(weights)
    d_off = so.to_device(np.arange(N + 1, dtype=np.int64) * L)
    for k, with_offsets in ((21, False), (21, True), (40, False)):
        name = "read bootstrap: weighted add, k = %d%s" % (k, " with offsets" if with_offsets else "")
        d_in, d_w = so.to_device(so.other_bases(blob)), so.to_device(poison)
        read_len, off_ptr = (0, d_off.data_ptr()) if with_offsets else (L, None)

        def add(st, counts):
            counts.add_weighted_device(d_in.data_ptr(), N, read_len, d_w.data_ptr(), d_offsets_ptr=off_ptr, stream=st,
                                       reserve=False)

        def warm():
            c = KmerCounts(k, canonical=True, min_slots=1 << 17)
            add(None, c)
            c.close()
        counts = KmerCounts(k, canonical=True, min_slots=1 << 17)
        run_a(name, S, [(d_in, d_true), (d_w, d_w_true)], lambda st: add(st, counts), warm=warm)
        want_hist, want_distinct = kr.histogram(bw.expand(strings, weights), k, True)
        assert counts.histogram() == want_hist and len(counts) == want_distinct, name  # (waits for the device: S is done)
        counts.close()
    torch.cuda.synchronize()


def case_draw_then_add():
    """The replicate as bootstrap_histograms makes it, on S and with no synchronisation inside: clear(S), the draw on S
    into a buffer that holds other weights (and is overwritten with them again behind the delay), add_weighted_device
    on S.  A draw on another stream is lost under the late copy; an add on another stream reads the poison."""
    import torch
    import bootstrap_weights_reference as bw
    import kmer_reference as kr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from covest_amd.read_bootstrap import bootstrap_weights_device
    from test_gpu_streams import run_a, simulated
    S = so.side_stream()
    reads, strings = simulated(2000, N, L, 0.02, SEED ^ 9)
    blob = reads.reshape(-1)
    first, rep, k = (1 << 32) - 100, 4, 21
    weights = bw.weights(N, rep, seed=SEED, first_read=first)
    poison = bw.weights(N, rep + 1, seed=SEED, first_read=first)
    d_in, d_true, d_old = so.to_device(so.other_bases(blob)), so.to_device(blob), so.to_device(blob)
    d_w, d_w_poison = so.to_device(poison), so.to_device(poison)
    counts = KmerCounts(k, canonical=True, min_slots=1 << 17)

    def replicate(st):
        counts.add_device(d_old.data_ptr(), N, L, stream=st, reserve=False)   # (what the clear has to take away, on S too)
        counts.clear(st)
        bootstrap_weights_device(d_w.data_ptr(), N, rep, seed=SEED, first_read=first, stream=st)
        counts.add_weighted_device(d_in.data_ptr(), N, L, d_w.data_ptr(), stream=st, reserve=False)

    def warm():
        c = KmerCounts(k, canonical=True, min_slots=1 << 17)
        c.add_weighted_device(d_true.data_ptr(), N, L, d_w_poison.data_ptr(), reserve=False)
        c.clear()
        c.close()
        scratch = so.to_device(poison)
        bootstrap_weights_device(scratch.data_ptr(), N, rep + 2, seed=SEED)
    run_a("read bootstrap: clear, draw, weighted add", S, [(d_in, d_true), (d_w, d_w_poison)], replicate, warm=warm)
    want_hist, want_distinct = kr.histogram(bw.expand(strings, weights), k, True)
    assert counts.histogram() == want_hist and len(counts) == want_distinct
    assert np.array_equal(d_w.cpu().numpy().view(np.uint32), weights)
    counts.close()
    torch.cuda.synchronize()


CASES = {f.__name__[5:]: f for f in (case_draw, case_weighted_add, case_draw_then_add)}


def _child(case):
    """One fresh child process: this file as a program, under a time limit of its own."""
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and ("%s ok" % case) in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
    return proc.stdout


def test_draw_on_a_side_stream(hip_lib):
    _child("draw")


def test_weighted_add_on_a_side_stream(hip_lib):
    _child("weighted_add")


def test_draw_then_weighted_add_without_a_synchronisation(hip_lib):
    _child("draw_then_add")


test_draw_on_a_side_stream.__doc__ = case_draw.__doc__
test_weighted_add_on_a_side_stream.__doc__ = case_weighted_add.__doc__
test_draw_then_weighted_add_without_a_synchronisation.__doc__ = case_draw_then_add.__doc__


if __name__ == "__main__":
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    CASES[sys.argv[1]]()
    print("%s ok" % sys.argv[1])
