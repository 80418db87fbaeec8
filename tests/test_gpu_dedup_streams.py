"""dedup_reads_device on a stream that is not the null stream (tests/stream_order.py, scheme A; the helpers of
tests/test_gpu_streams.py; the arrangement of tests/test_gpu_read_bootstrap_streams.py).

dedup_reads_device says "asynchronous on `stream`": two memsets, five kernels and the gather.  On the null stream a
launch that lost its `stream` argument gives the right answer; here the true inputs -- the bases and the offsets --
arrive late on a side stream S behind a bounded busy-wait, every output lies under a guard pattern that is copied over
it again behind the delay, and only S is waited for.  The poison is valid input of the same sizes with ANOTHER duplicate
structure (other reads are copies of one another, and every base is another one), so a launch on another stream keeps
other reads, and a memset or a launch that ran too early is lost under the pattern.  Expected values are the
restatement's (tests/dedup_reference.py), exact.

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
SEED = (0x57e4 << 32) | 0x0badf00d
PAT8, PAT32, PAT64 = 0x5A, 0x25A5A5A5, 0x25A5A5A5A5A5A5A5
N, L = 3000, 100


def read_sets():
    """(the true reads, the poison): the same sizes, other duplicates."""
    import dedup_reference as dr
    import stream_order as so
    true = dr.with_copies(N, L, 0.3, 61)
    other = dr.with_copies(N, L, 0.2, 62, rc_copies=True)
    poison = [bytes(so.other_bases(np.frombuffer(r, dtype=np.uint8))) for r in other]
    assert not np.array_equal(dr.dictionary(true)[0], dr.dictionary(poison)[0])
    return true, poison


class Outputs:
    """The five outputs under their guard patterns (test_gpu_streams.Out), and the call on them."""

    def __init__(self, n, total):
        import torch
        from test_gpu_streams import Out
        self.counts, self.bases = Out(3, torch.int64, PAT64), Out(total, torch.uint8, PAT8)
        self.offsets, self.kept, self.copies = Out(n + 1, torch.int64, PAT64), Out(n, torch.int64, PAT64), Out(n, torch.int32, PAT32)

    def late(self):
        return [o.late() for o in (self.counts, self.bases, self.offsets, self.kept, self.copies)]

    def call(self, st, d_in, n, rc, first, read_len=0, d_off=None):
        from covest_amd.dedup import dedup_reads_device
        dedup_reads_device(d_in.data_ptr(), n, self.bases.ptr, self.counts.ptr, reverse_complement=rc, seed=SEED,
                           first_read=first, read_len=read_len, offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                           out_offsets_ptr=self.offsets.ptr, kept_ptr=self.kept.ptr, copies_ptr=self.copies.ptr, stream=st)

    def check(self, where, reads, rc, first):
        import dedup_reference as dr
        kept, copies, collided = dr.dedup(reads, 63, SEED, rc)
        assert collided == 0
        bases, offsets = dr.pack([reads[i] for i in kept])
        assert self.counts.read(where).tolist() == [kept.size, bases.size, 0], where
        assert np.array_equal(self.kept.read(where, kept.size, True), kept + first), where
        assert np.array_equal(self.copies.read(where, kept.size, True), copies), where
        assert np.array_equal(self.offsets.read(where, kept.size + 1, True), offsets), where
        assert np.array_equal(self.bases.read(where, bases.size, True), bases), where
        return kept, bases


def case_dedup():
    """dedup_reads_device on S, reads of one length and reads with offsets (which arrive late too), forward and with the
    reverse complement."""
    import torch
    import dedup_reference as dr
    import stream_order as so
    from test_gpu_streams import run_a
    S = so.side_stream()
    true, poison = read_sets()
    ragged_true, ragged_poison = dr.ragged(63, per_length=40), dr.ragged(64, per_length=40)
    ragged_poison = [bytes(so.other_bases(np.frombuffer(r, dtype=np.uint8))) for r in ragged_poison]
    for name, reads, bad, fixed, rc, first in (("one length", true, poison, L, False, (1 << 32) - 100),
                                               ("one length, reverse complement", true, poison, L, True, 0),
                                               ("offsets", ragged_true, ragged_poison, None, True, 5)):
        blob, offs = dr.pack(reads)
        bad_blob, bad_offs = dr.pack(bad)
        assert bad_blob.size == blob.size and len(bad) == len(reads)
        assert fixed is not None or not np.array_equal(offs, bad_offs)
        n = len(reads)
        d_in, d_true = so.to_device(bad_blob), so.to_device(blob)
        copies = [(d_in, d_true)]
        d_off = None
        if fixed is None:
            d_off, d_off_true = so.to_device(bad_offs), so.to_device(offs)
            copies.append((d_off, d_off_true))
        out = Outputs(n, blob.size)
        warm_out = Outputs(n, blob.size)
        run_a("dedup: " + name, S, copies + out.late(),
              lambda st: out.call(st, d_in, n, rc, first, fixed or 0, d_off),
              warm=lambda: warm_out.call(None, d_true, n, rc, first, fixed or 0, so.to_device(offs) if fixed is None else None))
        out.check(name, reads, rc, first)
    torch.cuda.synchronize()


def case_dedup_then_add():
    """The call followed by add_device on the same stream with NO synchronisation between the two: the counter reads on
    S what the gather wrote on S.  The number of kept reads is the restatement's (the host cannot know it yet)."""
    import torch
    import dedup_reference as dr
    import kmer_reference as kr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from test_gpu_streams import run_a
    S = so.side_stream()
    true, poison = read_sets()
    blob, bad_blob = dr.pack(true)[0], dr.pack(poison)[0]
    d_in, d_true = so.to_device(bad_blob), so.to_device(blob)
    want_kept = dr.dictionary(true)[0]
    k = 21
    out, warm_out = Outputs(N, blob.size), Outputs(N, blob.size)
    counts = KmerCounts(k, canonical=True, min_slots=1 << 19)

    def both(st, o, c, src):
        o.call(st, src, N, False, 0, L)
        c.add_device(o.bases.ptr, want_kept.size, L, stream=st, reserve=False)

    def warm():
        c = KmerCounts(k, canonical=True, min_slots=1 << 19)
        both(None, warm_out, c, d_true)
        c.close()
    run_a("dedup, then add_device", S, [(d_in, d_true)] + out.late(), lambda st: both(st, out, counts, d_in), warm=warm)
    kept, _ = out.check("dedup, then add_device", true, False, 0)
    assert np.array_equal(kept, want_kept)
    want_hist, want_distinct = kr.histogram([true[i].decode() for i in kept], k, True)
    assert counts.histogram() == want_hist and len(counts) == want_distinct  # (waits for the device: S is done)
    counts.close()
    torch.cuda.synchronize()


CASES = {f.__name__[5:]: f for f in (case_dedup, case_dedup_then_add)}


def _child(case):
    """One fresh child process: this file as a program, under a time limit of its own."""
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and ("%s ok" % case) in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
    return proc.stdout


def test_dedup_on_a_side_stream(hip_lib):
    _child("dedup")


def test_dedup_then_add_without_a_synchronisation(hip_lib):
    _child("dedup_then_add")


test_dedup_on_a_side_stream.__doc__ = case_dedup.__doc__
test_dedup_then_add_without_a_synchronisation.__doc__ = case_dedup_then_add.__doc__


if __name__ == "__main__":
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    CASES[sys.argv[1]]()
    print("%s ok" % sys.argv[1])
