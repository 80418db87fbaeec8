"""Every asynchronous entry point on a stream that is not the null stream (tests/stream_order.py: schemes A and B).

"Asynchronous on `stream`" is what the device forms of the library say of themselves; on the null stream -- what every
other GPU test passes -- a launch that lost its `stream` argument, a memset or copy issued on nullptr, a missing
hipStreamWaitEvent and a read-back that waits for the wrong stream all give the right answer.  Here the true inputs
arrive late on a side stream S behind a bounded busy-wait (the reads side, scheme A), or a grid handle's own staging
copies queue up behind one on the null stream (scheme B), and only S, or the handle's read-back, is waited for: a piece
of work on the wrong stream computes on poison -- valid inputs of the same sizes -- or on what the last configuration
left behind, and the comparison fails.  Expected values are the project's restatements (sim_reference, repeat_reference,
sample_reference, split_reference, lookup_reference, correct_reference, draw_reference, oracle.kmer_oracle), bit for
bit; a grid on S is held against a second handle evaluated on the null stream.

What scheme A cannot see, by construction: a launch that reads nothing that arrives late and writes only the call's own
scratch -- the flag kernels of the sampler and the split look at the offsets and the seed alone -- computes the right
thing however early it runs.  Holding the null stream back instead would show it, but the rest of the call would then
read what an earlier call left in the scratch, which is not provably in range, and no case here may be able to fault:
those launches are left to review.  The partitioned counter keeps its buffers from call to call, so there the second
side is tested too (a recount of the same reads with the null stream held back).

Every case asserts that it was not blind: the host time from the enqueue of the delay to the return of the last call
under test is below half the delay the events measured (stream_order.Delay.check_blind).  Calls that wait for their
stream themselves are exempt and say so.

Each test is ONE fresh child process with torch imported first (one HIP runtime a process), as
tests/test_gpu_split.py does: this file run as a program with the name of the case.  One GPU process at a time, three
streams at the most, no environment variable, nothing that could fault: poison and stale data are valid inputs.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = (0x57e4 << 32) | 0x0badf00d   # both key words in use
PAT8, PAT32, PAT64, PATF = 0xA5, 0x25A5A5A5, -0x0123456789abcdef, -1.2345e300
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K, CUTOFF = 21, 2


# ---- what the cases share (child process only: torch is imported there, never in the pytest process) -------------------
class Out:
    """An output of n elements between eight guard elements either side.  The guard pattern fills all of it, and is
    copied over all of it AGAIN on the side stream behind the delay (`late()`): a memset or a launch of the entry point
    that ran too early is overwritten."""

    def __init__(self, n, dtype, pat):
        import torch
        self.n, self.pat = int(n), pat
        self.buf = torch.full((self.n + 16,), pat, dtype=dtype, device=torch.device("cuda", 0))
        self.fresh = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 8 * self.buf.element_size()

    def late(self):
        return (self.buf, self.fresh)

    def read(self, where, count=None, rest_untouched=False):
        """The first `count` elements (default: all n); the guards either side must hold their pattern."""
        a = self.buf.cpu().numpy()
        count = self.n if count is None else int(count)
        assert (a[:8] == self.pat).all() and (a[8 + self.n:] == self.pat).all(), ("stray write", where)
        if rest_untouched:
            assert (a[8 + count:8 + self.n] == self.pat).all(), ("written beyond its end", where)
        return a[8:8 + count]


def run_a(name, S, copies, call, warm=None, exempt=None):
    """Scheme A.  `warm()`: the entry point once on the null stream, on valid inputs, so that no first launch (code
    object loading, the first scratch block) falls into the timed part.  Then the delay on S, `copies` on S behind it,
    `call(stream)` with S, and S.synchronize() -- and only that."""
    import torch
    import stream_order as so
    if warm is not None:
        warm()
        torch.cuda.synchronize()  # (before the delay is enqueued: nothing of the case is in flight yet)
    d = so.late(S, copies)
    out = call(S.cuda_stream)
    issued = d.host_ms()
    S.synchronize()
    d.check_blind(issued, name, exempt)
    return out


def ragged_reads(n, seed):
    """(bases, offsets) of n reads of lengths 0 .. 300 (tests/test_gpu_split.py's mix)."""
    rng = np.random.default_rng(seed)
    lens = rng.choice((0, 1, 2, 5, 16, 17, 100, 300), size=n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return rng.choice(ACGT, size=int(offsets[-1])), offsets


def simulated(genome_len, n_reads, read_len, error_rate, seed):
    """((n, L) uint8 reads, the same as strings) of the restatement's simulator on the restatement's genome."""
    import sim_reference as sr
    genome = sr.random_genome(genome_len, seed)
    reads, _ = sr.reads_and_origin(genome, read_len, 0, n_reads, error_rate, seed)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    return reads, [bytes(r).decode("ascii") for r in reads]


# ---- the self-check: the detector sees a mis-streamed operation on this machine -----------------------------------------
def case_self_check():
    """One case per scheme in which an ordinary torch copy -- no kernel of the library -- is deliberately issued on the
    wrong stream: the comparison must come out unequal (and equal with the copy on the right stream)."""
    import torch
    import stream_order as so
    dev = torch.device("cuda", 0)
    S = so.side_stream()
    true = torch.arange(1 << 16, dtype=torch.int64, device=dev)
    poison = -true - 1
    torch.cuda.synchronize()
    # scheme A: the stand-in for an entry point copies its input to its output, on the null stream (wrong) and on S
    for wrong in (True, False):
        buf, out = poison.clone(), torch.zeros_like(true)
        torch.cuda.synchronize()
        d = so.late(S, [(buf, true)])
        with torch.cuda.stream(so.null_stream() if wrong else S):
            out.copy_(buf, non_blocking=True)
        issued = d.host_ms()
        S.synchronize()
        d.check_blind(issued, "self-check A (%s stream)" % ("wrong" if wrong else "right"))
        equal = bool(torch.equal(out, true))
        print("self-check A, copy on the %s stream: %s" % ("wrong" if wrong else "right", "equal" if equal else "unequal"))
        assert equal != wrong, ("scheme A does not see a mis-streamed copy: side streams block here, or the delay is "
                                "too short" if wrong else "scheme A: a copy on the right stream gave a wrong answer")
        if wrong:
            assert bool(torch.equal(out, poison)), "the mis-streamed copy read neither the poison nor the truth"
    # scheme B: the stand-in for a handle stages on the null stream behind the delay and records an event; the consumer
    # on S does not wait for it (wrong), or does
    for wrong in (True, False):
        buf, out = poison.clone(), torch.zeros_like(true)
        event = torch.cuda.Event()
        torch.cuda.synchronize()
        d = so.delay(so.null_stream())
        with torch.cuda.stream(so.null_stream()):
            buf.copy_(true, non_blocking=True)
            event.record(so.null_stream())
        with torch.cuda.stream(S):
            if not wrong:
                S.wait_event(event)
            out.copy_(buf, non_blocking=True)
        issued = d.host_ms()
        S.synchronize()
        d.check_blind(issued, "self-check B (%s)" % ("no wait" if wrong else "wait"))
        equal = bool(torch.equal(out, true))
        print("self-check B, consumer %s the event: %s" % ("without" if wrong else "behind", "equal" if equal else "unequal"))
        assert equal != wrong, ("scheme B does not see a missing event wait: side streams block here, or the delay is "
                                "too short" if wrong else "scheme B: a consumer behind the event gave a wrong answer")
    torch.cuda.synchronize()


# ---- generators ----------------------------------------------------------------------------------------------------------
def case_generators():
    import torch
    import repeat_reference as rr
    import sim_reference as sr
    import stream_order as so
    from covest_amd import simulate as sim
    from test_gpu_repeat import hand_plan
    S = so.side_stream()
    # random_genome_device, n = 257: no input -- the late guard pattern is what a launch on the wrong stream is lost under
    n = 257
    out = Out(n, torch.uint8, PAT8)
    run_a("generators: random_genome_device", S, [out.late()],
          lambda st: sim.random_genome_device(out.ptr, n, SEED, stream=st),
          warm=lambda: sim.random_genome_device(out.ptr, n, SEED ^ 1))
    assert np.array_equal(out.read("random genome"), sr.random_genome(n, SEED)), "random_genome_device"

    # repeat_genome_device on a hand-made plan of tests/test_gpu_repeat.py: the plan arrives late
    unit_len, n, div = 101, 4097, 0.1
    n_units = -(-n // unit_len)
    plan, poison = hand_plan("mixed", n_units), hand_plan("all distinct", n_units)
    d_plan, d_true = so.to_device(poison), so.to_device(plan)
    out = Out(n, torch.uint8, PAT8)

    def repeat(st):
        sim.repeat_genome_device(d_plan.data_ptr(), n_units, unit_len, n, out.ptr, divergence=div, seed=SEED, stream=st)
    run_a("generators: repeat_genome_device", S, [(d_plan, d_true), out.late()], repeat, warm=lambda: repeat(None))
    want = rr.genome(plan, unit_len, n, div, SEED)
    assert not np.array_equal(want, rr.genome(poison, unit_len, n, div, SEED))
    assert np.array_equal(out.read("repeat genome"), want), "repeat_genome_device"

    # simulate_reads_device: a genome of 20 000, 300 reads of 100, e = 0.05; the genome arrives late; with origin_ptr and without
    n_g, L, n_reads, e, first = 20_000, 100, 300, 0.05, 7
    genome = sr.random_genome(n_g, 3)
    want, want_origin = sr.reads_and_origin(genome, L, first, n_reads, e, SEED)
    d_genome, d_true = so.to_device(so.other_bases(genome)), so.to_device(genome)
    for with_origin in (True, False):
        d_genome.copy_(so.to_device(so.other_bases(genome)))
        bases, origin = Out(n_reads * L, torch.uint8, PAT8), Out(n_reads, torch.int64, PAT64)

        def simulate(st):
            sim.simulate_reads_device(d_genome.data_ptr(), n_g, L, n_reads, bases.ptr, error_rate=e, seed=SEED,
                                      first_read=first, origin_ptr=origin.ptr if with_origin else None, stream=st)
        run_a("generators: simulate_reads_device%s" % (" with origin" if with_origin else ""), S,
              [(d_genome, d_true), bases.late(), origin.late()], simulate, warm=lambda: simulate(None))
        assert np.array_equal(bases.read("reads").reshape(n_reads, L), want), ("simulate_reads_device", with_origin)
        assert np.array_equal(origin.read("origin", n_reads if with_origin else 0, rest_untouched=True),
                              want_origin if with_origin else want_origin[:0]), ("origin", with_origin)
    torch.cuda.synchronize()


# ---- sampler and split -----------------------------------------------------------------------------------------------------
def sampler_on(S, name, blob, offsets, L, first, factor, warm=True):
    """sample_reads_device on S with the bases arriving late (the offsets in place: the poison shares them): every
    output against sample_reference."""
    import torch
    import sample_reference as ref
    import stream_order as so
    from covest_amd import sample
    n = offsets.size - 1 if offsets is not None else blob.size // L
    d_in, d_true = so.to_device(so.other_bases(blob)), so.to_device(blob)
    d_off = so.to_device(offsets) if offsets is not None else None
    bases, out_off = Out(blob.size, torch.uint8, PAT8), Out(n + 1, torch.int64, PAT64)
    kept, counts = Out(n, torch.int64, PAT64), Out(2, torch.int64, PAT64)

    def call(st):
        sample.sample_reads_device(d_in.data_ptr(), n, bases.ptr, counts.ptr, factor, seed=SEED, first_read=first,
                                   read_len=L, offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                                   out_offsets_ptr=out_off.ptr, kept_ptr=kept.ptr, stream=st)
    run_a(name, S, [(d_in, d_true), bases.late(), out_off.late(), kept.late(), counts.late()], call,
          warm=(lambda: call(None)) if warm else None)
    want_bases, want_off, want_kept = ref.sample(blob, offsets if offsets is not None else L, first, factor, SEED)
    assert 0 < want_kept.size < n, name
    assert counts.read(name).tolist() == [want_kept.size, want_bases.size], (name, "counts")
    assert np.array_equal(bases.read(name, want_bases.size), want_bases), (name, "bases")
    assert np.array_equal(out_off.read(name, want_kept.size + 1), want_off), (name, "offsets")
    assert np.array_equal(kept.read(name, want_kept.size), want_kept), (name, "kept")


def split_on(S, name, blob, offsets, L, first, G, warm=True):
    """split_reads_device on S with the bases arriving late: every output against split_reference."""
    import torch
    import split_reference as ref
    import stream_order as so
    from covest_amd import sample
    n = offsets.size - 1 if offsets is not None else blob.size // L
    d_in, d_true = so.to_device(so.other_bases(blob)), so.to_device(blob)
    d_off = so.to_device(offsets) if offsets is not None else None
    bases, out_off = Out(blob.size, torch.uint8, PAT8), Out(n + 1, torch.int64, PAT64)
    index, first_of = Out(n, torch.int64, PAT64), Out(G + 1, torch.int64, PAT64)

    def call(st):
        sample.split_reads_device(d_in.data_ptr(), n, bases.ptr, first_of.ptr, G, seed=SEED, first_read=first, read_len=L,
                                  offsets_ptr=d_off.data_ptr() if d_off is not None else None, out_offsets_ptr=out_off.ptr,
                                  read_index_ptr=index.ptr, stream=st)
    run_a(name, S, [(d_in, d_true), bases.late(), out_off.late(), index.late(), first_of.late()], call,
          warm=(lambda: call(None)) if warm else None)
    want_bases, want_off, want_index, want_first = ref.split(blob, offsets if offsets is not None else L, first, G, SEED)
    assert np.array_equal(first_of.read(name), want_first), (name, "group_first")
    assert np.array_equal(bases.read(name), want_bases), (name, "bases")
    assert np.array_equal(out_off.read(name), want_off), (name, "offsets")
    assert np.array_equal(index.read(name), want_index), (name, "read_index")


def case_sampler_and_split():
    import torch
    import stream_order as so
    from covest_amd import sample
    S = so.side_stream()
    share, scan_pass = sample.SPLIT_SHARE, sample.SPLIT_SCAN_PASS
    n = share + 1
    rng = np.random.default_rng(11)
    fixed = rng.choice(ACGT, size=n * 7)
    blob, offsets = ragged_reads(n, 20241019)
    sampler_on(S, "sampler: one length", fixed, None, 7, 3, 2.0)
    sampler_on(S, "sampler: ragged", blob, offsets, 0, (1 << 32) - 3, 3.0)
    for G in (3, 65):
        split_on(S, "split: one length, G = %d" % G, fixed, None, 7, 3, G)
        split_on(S, "split: ragged, G = %d" % G, blob, offsets, 0, (1 << 32) - 3, G)
    # rows of more than one pass of the scan: share * pass + share + 1 reads of length 1
    n = share * scan_pass + share + 1
    split_on(S, "split: two passes of the row scan", rng.choice(ACGT, size=n), None, 1, 5, 3)
    # n_reads == 0: nothing is launched, the outputs are memsets on the stream -- under the late guard pattern if they ran
    # on another one
    counts, out_off = Out(2, torch.int64, PAT64), Out(1, torch.int64, PAT64)
    run_a("sampler: no reads", S, [counts.late(), out_off.late()],
          lambda st: sample.sample_reads_device(0, 0, 0, counts.ptr, 2.0, read_len=5, out_offsets_ptr=out_off.ptr, stream=st))
    assert counts.read("no reads").tolist() == [0, 0] and out_off.read("no reads").tolist() == [0], "sampler: n_reads == 0"
    first_of, out_off = Out(6, torch.int64, PAT64), Out(1, torch.int64, PAT64)
    run_a("split: no reads", S, [first_of.late(), out_off.late()],
          lambda st: sample.split_reads_device(0, 0, 0, first_of.ptr, 5, read_len=5, out_offsets_ptr=out_off.ptr, stream=st))
    assert first_of.read("no reads").tolist() == [0] * 6 and out_off.read("no reads").tolist() == [0], "split: n_reads == 0"
    torch.cuda.synchronize()


# ---- the counter: add_device, lookup_device, correct_device, clear -------------------------------------------------------
def case_counter():
    import torch
    import correct_reference as cr
    import kmer_reference as kr
    import lookup_reference as lr
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from oracle import kmer_oracle
    S = so.side_stream()
    n, L = 300, 100
    reads, strings = simulated(2000, n, L, 0.02, SEED)          # (coverage 15: the correction has something to correct)
    table = kr.count(strings, K, True)
    weights = np.array([3.25, -1e-3, 0.1, 7.0e5, 2.0 ** -30, -0.7, 1.0 / 3.0])   # (tests/test_gpu_lookup.py's table)
    d_weights = so.to_device(weights)
    want_ab, _, want_sum, want_score = lr.lookup(strings, table, K, True, CUTOFF, weights)
    want_out, _, want_fix, _ = cr.correct(strings, table, K, True, CUTOFF)
    assert (want_fix[:, 1] > 0).any() and (want_sum[:, 1] > 0).any()
    blob = reads.reshape(-1)
    d_true = so.to_device(blob)
    d_off = so.to_device(np.arange(n + 1, dtype=np.int64) * L)

    def outputs():
        return (Out(n * L, torch.int32, PAT32), Out(4 * n, torch.int32, PAT32), Out(n * L, torch.uint8, PAT8),
                Out(4 * n, torch.int32, PAT32))

    def check(name, ab, summary, out, fix, score=None):
        assert np.array_equal(ab.read(name).view(np.uint32), want_ab), (name, "abundance")
        assert np.array_equal(summary.read(name).view(np.uint32).reshape(n, 4), want_sum), (name, "summary")
        if score is not None:
            assert np.array_equal(score.read(name).view(np.uint64), want_score.view(np.uint64)), (name, "score")
        if out is not None:
            assert np.array_equal(out.read(name), want_out), (name, "corrected bases")
            assert np.array_equal(fix.read(name).view(np.uint32).reshape(n, 4), want_fix), (name, "fix")

    for with_offsets in (False, True):
        name = "counter: add, lookup, correct%s" % (" with offsets" if with_offsets else "")
        d_in = so.to_device(so.other_bases(blob))
        ab, summary, out, fix = outputs()
        score = Out(n, torch.float64, PATF)
        read_len, off_ptr = (0, d_off.data_ptr()) if with_offsets else (L, None)

        def chain(st, counts):
            counts.add_device(d_in.data_ptr(), n, read_len, d_offsets_ptr=off_ptr, stream=st, reserve=False)
            counts.lookup_device(d_in.data_ptr(), n, read_len, d_offsets_ptr=off_ptr, cutoff=CUTOFF,
                                 d_weights_ptr=d_weights.data_ptr(), n_weights=len(weights), d_abundance_ptr=ab.ptr,
                                 d_summary_ptr=summary.ptr, d_score_ptr=score.ptr, stream=st)
            counts.correct_device(d_in.data_ptr(), n, read_len, out.ptr, d_offsets_ptr=off_ptr, cutoff=CUTOFF,
                                  d_fix_ptr=fix.ptr, stream=st)

        def warm():
            c = KmerCounts(K, canonical=True, min_slots=1 << 16)
            chain(None, c)
            c.close()
        counts = KmerCounts(K, canonical=True, min_slots=1 << 16)
        run_a(name, S, [(d_in, d_true), ab.late(), summary.late(), out.late(), fix.late(), score.late()],
              lambda st: chain(st, counts), warm=warm)
        check(name, ab, summary, out, fix, score)
        assert len(counts) == len(table), name  # (waits for the device itself: after the comparison)
        counts.close()

    # clear(S) followed by add_device on S, no synchronisation in between: the same reads counted before the clear, on S
    # too -- a clear that ran on another stream runs before them, and every abundance doubles
    name = "counter: clear, then add"
    d_in, d_old = so.to_device(so.other_bases(blob)), so.to_device(blob)
    ab, summary, _, _ = outputs()
    counts = KmerCounts(K, canonical=True, min_slots=1 << 16)

    def clear_and_add(st):
        counts.add_device(d_old.data_ptr(), n, L, stream=st, reserve=False)
        counts.clear(st)
        counts.add_device(d_in.data_ptr(), n, L, stream=st, reserve=False)
        counts.lookup_device(d_in.data_ptr(), n, L, cutoff=CUTOFF, d_abundance_ptr=ab.ptr, d_summary_ptr=summary.ptr, stream=st)
    run_a(name, S, [(d_in, d_true), ab.late(), summary.late()], clear_and_add)
    check(name, ab, summary, None, None)
    counts.close()

    # keys of more than one word (k = 40: kmer_wide.hip's clear and count): the same sequence, read through histogram()
    name = "counter: wide keys, clear, then add"
    d_in.copy_(so.to_device(so.other_bases(blob)))
    wide = KmerCounts(40, canonical=True, min_slots=1 << 16)

    def wide_clear_and_add(st):
        wide.add_device(d_old.data_ptr(), n, L, stream=st, reserve=False)
        wide.clear(st)
        wide.add_device(d_in.data_ptr(), n, L, stream=st, reserve=False)
    run_a(name, S, [(d_in, d_true)], wide_clear_and_add)
    assert wide.histogram() == kmer_oracle.histogram(strings, 40, canonical=True), name  # (waits for the device: S is done)
    wide.close()

    # Scheme B for the counter's own null-stream work: covest_kmer_create empties the table on the null stream and
    # covest_kmer_reserve re-inserts on it; an add on S must find the table ready.  Both wait for the device themselves
    # (exempt): what is pinned is the result, with the null stream held back while they are called.
    name = "counter: created and reserved behind a late null stream"
    d_in.copy_(d_true)
    ab, summary, _, _ = outputs()
    torch.cuda.synchronize()
    d = so.delay(so.null_stream())
    counts = KmerCounts(K, canonical=True, min_slots=1024)
    counts.add_device(d_in.data_ptr(), n, L, stream=S.cuda_stream)       # (reserve=True: the table of 1 024 slots grows)
    counts.lookup_device(d_in.data_ptr(), n, L, cutoff=CUTOFF, d_abundance_ptr=ab.ptr, d_summary_ptr=summary.ptr,
                         stream=S.cuda_stream)
    issued = d.host_ms()
    S.synchronize()
    d.check_blind(issued, name, exempt="creation and reserve wait for the device")
    assert counts.slots > 1024, name
    check(name, ab, summary, None, None)
    counts.close()
    torch.cuda.synchronize()


# ---- the partitioned counter ---------------------------------------------------------------------------------------------
def case_partitioned():
    """count_reads_device waits for its stream itself (the layout of ragged reads, the room of the buckets, what the
    passes reported): exempt from the blindness condition.  Scheme A covers its first stage -- whatever it issues before
    its first wait runs on the poison if it is on another stream -- and the result.  A recount of the same reads on S
    with the NULL stream held back covers the later stages (what they put on the null stream would run after its report
    was read), and asserts the blindness condition: the call waits for S alone."""
    import torch
    import stream_order as so
    from covest_amd.kmer_hist import KmerCounts
    from oracle import kmer_oracle
    S = so.side_stream()
    n, L = 300, 100
    reads, strings = simulated(2000, n, L, 0.02, SEED ^ 5)
    rng = np.random.default_rng(3)
    lens = rng.integers(K, L + 1, size=n)                       # no read shorter than k
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    cut = [s[:m] for s, m in zip(strings, lens.tolist())]
    cut_blob = np.frombuffer("".join(cut).encode(), dtype=np.uint8)
    for name, blob, offs, texts in (("partitioned: one length", reads.reshape(-1), None, strings),
                                    ("partitioned: ragged", cut_blob, offsets, cut)):
        want_hist = kmer_oracle.histogram(texts, K, canonical=True)
        want_len = len(kmer_oracle.count_kmers(texts, K, canonical=True)[0])
        d_in, d_true = so.to_device(so.other_bases(blob)), so.to_device(blob)
        d_off = so.to_device(offs) if offs is not None else None
        counts = KmerCounts(K, canonical=True)

        def call(st):
            return counts.count_reads_device(d_in.data_ptr(), n, 0 if offs is not None else L,
                                             d_offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                                             n_bases=blob.size, stream=st)
        path = run_a(name, S, [(d_in, d_true)], call, exempt="count_reads_device waits for its stream")
        assert path == "partitioned", (name, path, getattr(counts, "why_not_partitioned", None))
        assert counts.histogram() == want_hist and len(counts) == want_len, name  # (histogram waits for the device)
        counts.close()
        # The later stages, from the other side: the NULL stream is held back while the call runs on S, so a launch,
        # memset or copy that the call put on the null stream runs late, and what the passes report is read before it
        # ran.  The call waits for S only: here the blindness condition holds and is asserted.  The counter has counted
        # the same reads once before (on the null stream): every buffer it keeps from call to call holds what this count
        # leaves there, so a stage that ran late finds valid contents.
        held = name + ", null stream held back"
        again = KmerCounts(K, canonical=True)
        d_in.copy_(d_true)

        def recount(st):
            return again.count_reads_device(d_in.data_ptr(), n, 0 if offs is not None else L,
                                            d_offsets_ptr=d_off.data_ptr() if d_off is not None else None,
                                            n_bases=blob.size, stream=st)
        assert recount(None) == "partitioned" and again.histogram() == want_hist, held
        torch.cuda.synchronize()
        d = so.delay(so.null_stream())
        path = recount(S.cuda_stream)
        issued = d.host_ms()
        S.synchronize()
        d.check_blind(issued, held)
        assert path == "partitioned", (held, path)
        assert again.histogram() == want_hist and len(again) == want_len, held
        again.close()
    torch.cuda.synchronize()


# ---- bootstrap draws -------------------------------------------------------------------------------------------------------
def case_draws():
    import torch
    import draw_reference as ref
    import stream_order as so
    from covest_amd import bootstrap as bs
    S = so.side_stream()
    rng = np.random.default_rng(5)
    n, reps, first = 9001, 2, 2
    for m in (300, 13_000):          # counters in LDS, counters in HBM
        w, w_poison = rng.random(m) + 1e-3, rng.random(m) + 1e-3
        d_t, d_true = so.to_device(bs.draw_thresholds(w_poison)), so.to_device(bs.draw_thresholds(w))
        out = Out(reps * m, torch.int64, -7)

        def call(st):
            bs.draw_histograms_device(d_t.data_ptr(), m, n, reps, out.ptr, seed=77, first_replicate=first, stream=st)
        run_a("draws: m = %d" % m, S, [(d_t, d_true), out.late()], call, warm=lambda: call(None))
        want = ref.draw_histograms(w, n, reps, seed=77, first_replicate=first)
        assert np.array_equal(out.read(m).reshape(reps, m), want), ("draw_histograms_device", m)
    torch.cuda.synchronize()


# ---- a chain with no synchronisation inside ----------------------------------------------------------------------------
def case_chain():
    import torch
    import stream_order as so
    from covest_amd import sample, simulate as sim
    from covest_amd.kmer_hist import KmerCounts
    S = so.side_stream()
    n_g, L, n, e, G = 3000, 100, 300, 0.02, 4
    # the same chain made with the host forms (they wait for the device: all of it before the delay)
    h_genome = sim.random_genome(n_g, SEED)
    h_reads = sim.simulate_reads(h_genome, L, n_reads=n, error_rate=e, seed=SEED)
    h_split = sample.split_reads(h_reads, G, seed=SEED)
    host = KmerCounts(K, canonical=True)
    h_reads.add_to(host)
    h_found = host.lookup(h_split.bases, cutoff=CUTOFF)
    h_fixed = host.correct(h_split.bases, CUTOFF)
    host.close()
    torch.cuda.synchronize()
    genome, reads, origin = Out(n_g, torch.uint8, PAT8), Out(n * L, torch.uint8, PAT8), Out(n, torch.int64, PAT64)
    split, index, first_of = Out(n * L, torch.uint8, PAT8), Out(n, torch.int64, PAT64), Out(G + 1, torch.int64, PAT64)
    ab, summary = Out(n * L, torch.int32, PAT32), Out(4 * n, torch.int32, PAT32)
    fixed, fix = Out(n * L, torch.uint8, PAT8), Out(4 * n, torch.int32, PAT32)
    counts = KmerCounts(K, canonical=True, min_slots=1 << 16)

    def chain(st):
        sim.random_genome_device(genome.ptr, n_g, SEED, stream=st)
        sim.simulate_reads_device(genome.ptr, n_g, L, n, reads.ptr, error_rate=e, seed=SEED, origin_ptr=origin.ptr, stream=st)
        sample.split_reads_device(reads.ptr, n, split.ptr, first_of.ptr, G, seed=SEED, read_len=L, read_index_ptr=index.ptr,
                                  stream=st)
        counts.add_device(split.ptr, n, L, stream=st, reserve=False)
        counts.lookup_device(split.ptr, n, L, cutoff=CUTOFF, d_abundance_ptr=ab.ptr, d_summary_ptr=summary.ptr, stream=st)
        counts.correct_device(split.ptr, n, L, fixed.ptr, cutoff=CUTOFF, d_fix_ptr=fix.ptr, stream=st)
    outs = (genome, reads, origin, split, index, first_of, ab, summary, fixed, fix)
    run_a("chain: genome, reads, split, add, lookup, correct", S, [o.late() for o in outs], chain)
    assert np.array_equal(genome.read("genome"), h_genome), "chain: genome"
    assert np.array_equal(reads.read("reads").reshape(n, L), h_reads.bases), "chain: reads"
    assert np.array_equal(origin.read("origin"), h_reads.positions << 1 | h_reads.forward.astype(np.int64)), "chain: origin"
    assert np.array_equal(split.read("split").reshape(n, L), h_split.bases), "chain: split bases"
    assert np.array_equal(index.read("index"), h_split.read_index), "chain: read_index"
    assert np.array_equal(first_of.read("group_first"), h_split.group_first), "chain: group_first"
    assert np.array_equal(ab.read("abundance").view(np.uint32), h_found.abundance), "chain: abundance"
    assert np.array_equal(summary.read("summary").view(np.uint32).reshape(n, 4), h_found.summary), "chain: summary"
    assert np.array_equal(fixed.read("corrected"), h_fixed.bases), "chain: corrected bases"
    assert np.array_equal(fix.read("fix").view(np.uint32).reshape(n, 4), h_fixed.fix), "chain: fix"
    assert h_fixed.corrected.sum() > 0 and h_found.weak.sum() > 0
    counts.close()
    torch.cuda.synchronize()


# ---- two streams at once -----------------------------------------------------------------------------------------------
def case_two_streams():
    """A split pending behind a delay on S1 while a sampler call and a split call run on S2: they complete after
    S2.synchronize() alone, the host has not waited for S1, and S1's outputs are right afterwards.  Then 8 rounds of a
    sampler call on S1 and a split call on S2 behind equal delays, sizes falling from round to round so that no
    scratch block grows.  A scratch block shared between overlapping calls (call_scratch.h hands a block to one call at a
    time) makes these rounds LIKELY to fail, not certain: no arrangement of two whole calls can force their kernels to
    interleave."""
    import torch
    import sample_reference as sref
    import split_reference as pref
    import stream_order as so
    from covest_amd import sample
    S1, S2 = so.side_stream(), so.side_stream()
    rng = np.random.default_rng(17)
    L = 7
    # (the host forms first: every kernel has been launched once before anything is timed)
    sample.sample_reads(rng.choice(ACGT, size=(64, L)), 2.0, seed=SEED)
    sample.split_reads(rng.choice(ACGT, size=(64, L)), 3, seed=SEED)
    torch.cuda.synchronize()

    class Split:
        def __init__(self, n, G):
            self.n, self.G = n, G
            self.blob = rng.choice(ACGT, size=n * L)
            self.d_in, self.d_true = so.to_device(so.other_bases(self.blob)), so.to_device(self.blob)
            self.bases, self.index = Out(n * L, torch.uint8, PAT8), Out(n, torch.int64, PAT64)
            self.first_of = Out(G + 1, torch.int64, PAT64)

        def late(self):
            return [(self.d_in, self.d_true), self.bases.late(), self.index.late(), self.first_of.late()]

        def call(self, st):
            sample.split_reads_device(self.d_in.data_ptr(), self.n, self.bases.ptr, self.first_of.ptr, self.G, seed=SEED,
                                      read_len=L, read_index_ptr=self.index.ptr, stream=st)

        def check(self, name):
            want_bases, _, want_index, want_first = pref.split(self.blob, L, 0, self.G, SEED)
            assert np.array_equal(self.first_of.read(name), want_first), (name, "group_first")
            assert np.array_equal(self.bases.read(name), want_bases), (name, "bases")
            assert np.array_equal(self.index.read(name), want_index), (name, "read_index")

    class Sampler:
        def __init__(self, n):
            self.n = n
            self.blob = rng.choice(ACGT, size=n * L)
            self.d_in, self.d_true = so.to_device(so.other_bases(self.blob)), so.to_device(self.blob)
            self.bases, self.kept = Out(n * L, torch.uint8, PAT8), Out(n, torch.int64, PAT64)
            self.counts = Out(2, torch.int64, PAT64)

        def late(self):
            return [(self.d_in, self.d_true), self.bases.late(), self.kept.late(), self.counts.late()]

        def call(self, st):
            sample.sample_reads_device(self.d_in.data_ptr(), self.n, self.bases.ptr, self.counts.ptr, 2.0, seed=SEED,
                                       read_len=L, kept_ptr=self.kept.ptr, stream=st)

        def check(self, name):
            want_bases, _, want_kept = sref.sample(self.blob, L, 0, 2.0, SEED)
            assert self.counts.read(name).tolist() == [want_kept.size, want_bases.size], (name, "counts")
            assert np.array_equal(self.bases.read(name, want_bases.size), want_bases), (name, "bases")
            assert np.array_equal(self.kept.read(name, want_kept.size), want_kept), (name, "kept")

    pending, small_sampler, small_split = Split(2 * sample.SPLIT_SHARE + 1, 5), Sampler(1500), Split(1200, 3)
    for job in (small_sampler, small_split):  # S2's inputs are in place: nothing delays S2
        job.d_in.copy_(job.d_true)
    torch.cuda.synchronize()
    d = so.late(S1, pending.late())
    pending.call(S1.cuda_stream)
    small_sampler.call(S2.cuda_stream)
    small_split.call(S2.cuda_stream)
    S2.synchronize()                      # and only S2
    issued = d.host_ms()
    small_sampler.check("two streams: sampler on S2")
    small_split.check("two streams: split on S2")
    d.check_blind(issued, "two streams: S2 complete while S1 is pending")  # (the host has not waited for S1)
    S1.synchronize()
    pending.check("two streams: split on S1")
    worst = 0.0
    for r in range(8):
        n = 1100 - 100 * r
        a, b = Sampler(n), Split(n, 3)
        torch.cuda.synchronize()
        da = so.late(S1, a.late(), ms=30.0)
        db = so.late(S2, b.late(), ms=30.0)
        a.call(S1.cuda_stream)
        b.call(S2.cuda_stream)
        issued = da.host_ms()
        S1.synchronize()
        S2.synchronize()
        worst = max(worst, issued)
        assert issued < 0.5 * min(da.ms(), db.ms()), ("round %d has tested nothing: host %.1f ms" % (r, issued))
        a.check("two streams: round %d, sampler on S1" % r)
        b.check("two streams: round %d, split on S2" % r)
    print("stream-order: two streams: 8 rounds behind 30 ms delays, largest host issue %.2f ms" % worst)
    torch.cuda.synchronize()


# ---- the grid side: scheme B -----------------------------------------------------------------------------------------------
def null_reference(model, axes, kernel, scan_start=None):
    """(values, arg-min, scan records) of a second handle configured with `axes` and evaluated on the null stream."""
    from covest_amd import DenseGrid
    g = DenseGrid(model, axes)
    g.evaluate(kernel=kernel, scan_start=scan_start)
    out = g.loglikelihoods(), g.argmin(), g.scan_records() if scan_start is not None else None
    g.close()
    return out


def same_as(name, got, want):
    ll, best, scan = got
    rll, rbest, rscan = want
    assert np.array_equal(ll, rll, equal_nan=True), (name, "values", int((ll != rll).sum()))
    assert best == rbest, (name, "arg-min", best, rbest)
    if rscan is not None:
        assert scan is not None and list(scan[0]) == list(rscan[0]) and list(scan[1]) == list(rscan[1]), (name, "scan records")


def grid_b(name, S, model, axes1, axes2, kernel, scan_start=None, exempt=None, want_owed=None):
    """Scheme B.  The handle is created with axes1 and evaluated once -- on S, so that the reset's wait for the stream of
    the last evaluation is not a wait for the null stream; the first configuration went up by blocking copies, the
    asynchronous ones start with the first reset.  Then the delay on the null stream, reset(axes2), evaluate(stream=S),
    and the handle's own read-back.  Returns (values, arg-min, scan records) after comparing them with the null-stream
    handle's."""
    import stream_order as so
    from covest_amd import DenseGrid
    want = null_reference(model, axes2, kernel, scan_start)
    stale = null_reference(model, axes1, kernel, scan_start)
    assert not np.array_equal(stale[0], want[0], equal_nan=True), (name, "the two configurations give the same values")
    g = DenseGrid(model, axes1)
    g.evaluate(kernel=kernel, stream=S.cuda_stream, scan_start=scan_start)
    same_as(name + " (first configuration)", (g.loglikelihoods(), g.argmin(), None), (stale[0], stale[1], None))
    d = so.delay(so.null_stream())
    g.reset(axes2)
    g.evaluate(kernel=kernel, stream=S.cuda_stream, scan_start=scan_start)
    issued = d.host_ms()
    if want_owed is not None:  # (a read of the provisional values: it succeeds exactly while the strict pass is owed)
        prov = g.provisional_loglikelihoods()
    got = g.loglikelihoods(), g.argmin(), g.scan_records() if scan_start is not None else None
    d.check_blind(issued, name, exempt)
    same_as(name, got, want)
    if want_owed is not None:
        moved = int((prov.view(np.int64) != got[0].view(np.int64)).sum())
        print("%s: %d values moved by the strict pass on the stream of the evaluation" % (name, moved))
        assert moved > 0, (name, "no point was handed back")
    g.close()
    return got


def shifted(axes, dc, de):
    """axes2 of a case: the same lengths and the same q axes, other values of c and e."""
    return [axes[0] + dc, axes[1] + de] + [a.copy() for a in axes[2:]]


def case_grid_repeats():
    import torch
    import stream_order as so
    from covest_amd import RepeatsModel
    from oracle import covest_oracle
    from test_gpu_factored_band import HIST
    from test_gpu_factored_colskip import GRIDS
    from test_gpu_variants import _against_direct, _points
    covest_oracle.build()
    S = so.side_stream()
    skip = GRIDS["skip"]                                                         # 432 points: read in place
    # the smallest grid of whole (c, e) pairs above kArgminSmall = 16 384 points: 19 x 18 pairs of 48 weight vectors
    large = [np.linspace(12.0, 30.0, 19), np.linspace(0.005, 0.08, 18)] + [a.copy() for a in skip[2:]]
    assert 16384 < math.prod(len(a) for a in large) <= 16384 + 48 and math.prod(len(a) for a in skip) == 432
    for tail in (0, 7):
        m = RepeatsModel(21, 100, HIST, tail, max_error=8)
        om = covest_oracle.OracleModel("repeats", 21, 100, HIST, tail, max_error=8)
        t = " tail" if tail else ""
        got = {}
        for kernel in ("factored", "direct"):
            got[kernel] = grid_b("grid: repeats%s, 432 points in place, %s" % (t, kernel), S, m, skip, shifted(skip, 1.0, 0.002), kernel)
            grid_b("grid: repeats%s, 16 416 points copied, %s" % (t, kernel), S, m, large, shifted(large, 0.5, 0.001), kernel)
        # the values themselves (they equal the null stream's): K-factored against K-direct and the oracle, at the project's 1e-10
        axes2 = shifted(skip, 1.0, 0.002)
        _against_direct(om, got["factored"][0], got["direct"][0], tail, "streams: skip%s" % t, lambda idx: _points(axes2, idx))
        if not tail:  # the selection scan on the device: its records are read back through the handle too
            grid_b("grid: repeats, 432 points in place, factored with scan", S, m, skip, axes2, "factored", scan_start=math.inf)
        m.close()
    torch.cuda.synchronize()


def case_grid_basic():
    import torch
    import stream_order as so
    from covest_amd import BasicModel
    from test_gpu_lazy_fix import BASIC_8X8, BASIC_TWO_STAGE, H280
    S = so.side_stream()
    m = BasicModel(21, 100, H280, 0, max_error=8)
    # A reset on the in-place path that issues the 8-byte memset of the queue counter on the null stream.  stage_inputs
    # issues it where the counter is not known to be clean where it lies, and on the in-place path that is a reset whose
    # arena grew: 64 points, then 128 x 128 = 16 384, the largest grid read in place (the process's buffer cache hands
    # buffers out by best fit: the handle of 64 points does not get a block fit for 16 384).  Growing the arena waits for
    # the device, so the case cannot be blind: what it pins is that the evaluation on S finds a cleared counter (kernel
    # "recur" hands points back through it).
    grown = [np.linspace(13.0, 18.0, 128), np.linspace(0.01, 0.04, 128)]
    grid_b("grid: basic, 64 -> 16 384 points in place, counter memset", S, m, BASIC_8X8, grown, "recur",
           exempt="the arena grows: the reset waits for the device", want_owed=True)
    # the smallest grid above kArgminSmall: 16 385 = 145 x 113 points, axes only
    large = [np.linspace(13.0, 18.0, 145), np.linspace(0.01, 0.04, 113)]
    for kernel in ("recur", "direct"):
        grid_b("grid: basic, 16 385 points copied, %s" % kernel, S, m, large, shifted(large, 0.01, 0.0001), kernel)
    # grids whose evaluation hands points back (tests/test_gpu_lazy_fix.py): the strict pass is owed, and runs on the
    # stream of the evaluation when the values are read
    grid_b("grid: basic, 8 x 8 in place, strict pass owed", S, m, BASIC_8X8, shifted(BASIC_8X8, 0.01, 0.0001), "recur",
           want_owed=True)
    grid_b("grid: basic, 160 x 110 copied, strict pass owed", S, m, BASIC_TWO_STAGE, shifted(BASIC_TWO_STAGE, 0.01, 0.0001),
           "recur", want_owed=True)
    # a reset that changes an axis length: the last axis loses a value (the arena does not grow; what the old
    # configuration left where the new axes go are valid numbers)
    longer = [np.linspace(13.0, 18.0, 146), np.linspace(0.01, 0.04, 114)]
    shorter = [longer[0] + 0.01, np.linspace(0.0101, 0.0401, 113)]
    grid_b("grid: basic, 146 x 114 -> 146 x 113 copied", S, m, longer, shorter, "recur")
    m.close()
    torch.cuda.synchronize()


def case_grid_read_back():
    """Read-back order: evaluate(stream=S) behind a delay ON S, followed at once by argmin() and loglikelihoods() -- a
    read-back that waited for another stream would return what the evaluation before left; argmin_pair_tensor consumed
    on S; axis_minima; and two resets in a row with no read in between."""
    import torch
    import stream_order as so
    from covest_amd import BasicModel, DenseGrid
    from test_gpu_lazy_fix import BASIC_8X8, BASIC_TWO_STAGE
    from test_gpu_lazy_fix import H280
    S = so.side_stream()
    m = BasicModel(21, 100, H280, 0, max_error=8)

    def settle(g, axes):
        # other axes on the handle, and nothing of it in flight: the case that follows begins with idle streams
        g.reset(axes)
        S.synchronize()
        so.null_stream().synchronize()

    for axes, size in ((BASIC_8X8, "8 x 8"), (BASIC_TWO_STAGE, "160 x 110")):
        axes2, axes3 = shifted(axes, 0.01, 0.0001), shifted(axes, 0.02, 0.0002)
        want2, want3 = null_reference(m, axes2, "recur"), null_reference(m, axes3, "recur")
        r = DenseGrid(m, axes2)
        r.evaluate(kernel="recur")
        axis2 = r.axis_minima((0,))
        r.close()
        g = DenseGrid(m, axes)
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        first = g.loglikelihoods()
        assert not np.array_equal(first, want2[0], equal_nan=True)
        settle(g, axes2)
        # (the strict pass is owed after the evaluation: argmin() and loglikelihoods() launch it on S, behind the delay)
        name = "grid: read-back at once, %s" % size
        d = so.delay(S)
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        issued = d.host_ms()
        best = g.argmin()
        ll = g.loglikelihoods()
        d.check_blind(issued, name)
        same_as(name, (ll, best, None), want2)
        # the pair where the arg-min kernel left it, consumed on S (other axes first: what the handle holds must differ)
        name = "grid: argmin_pair_tensor on S, %s" % size
        settle(g, axes3)
        d = so.delay(S)
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        pair = g.argmin_pair_tensor(0)
        with torch.cuda.stream(S):
            taken = pair.clone()
        issued = d.host_ms()
        S.synchronize()
        d.check_blind(issued, name)
        value, index = taken.cpu().tolist()
        assert want3[1] != want2[1], name
        assert (value, int(index)) == g.argmin() == want3[1], (name, value, index, g.argmin(), want3[1])
        g.fix_eager(False)
        # the per-axis minima: reduced on the stream of the evaluation, behind it
        name = "grid: axis_minima at once, %s" % size
        settle(g, axes2)
        d = so.delay(S)
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        issued = d.host_ms()
        val, idx = g.axis_minima((0,))
        d.check_blind(issued, name)
        assert np.array_equal(val, axis2[0]) and np.array_equal(idx, axis2[1]), name
        # two resets in a row: reset, evaluate(S) -- pending behind a delay on S --, reset, evaluate(S), no read in
        # between; the second reset behind a longer delay on the null stream.  The reset itself must have waited for S
        # (it stages over what the pending evaluation reads): S is idle when it returns.
        name = "grid: two resets in a row, %s" % size
        g.reset(axes2)
        ds = so.delay(S, 50.0)
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        d = so.delay(so.null_stream(), 300.0)
        g.reset(axes3)
        assert S.query(), (name, "the reset returned while the evaluation on S was still in flight")
        waited = d.host_ms()
        g.evaluate(kernel="recur", stream=S.cuda_stream)
        issued = d.host_ms()
        got = g.loglikelihoods(), g.argmin(), None
        print("stream-order: %s: the second reset returned %.1f ms after the null-stream delay began (S held %.1f ms)"
              % (name, waited, ds.ms()))
        d.check_blind(issued, name)
        same_as(name, got, want3)
        g.close()
    m.close()
    torch.cuda.synchronize()


CASES = {f.__name__[5:]: f for f in (case_self_check, case_generators, case_sampler_and_split, case_counter, case_partitioned,
                                     case_draws, case_chain, case_two_streams, case_grid_repeats, case_grid_basic,
                                     case_grid_read_back)}


def _child(case):
    """One fresh child process: this file as a program, under a time limit of its own."""
    proc = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), case],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and ("%s ok" % case) in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
    return proc.stdout


def test_self_check_both_schemes_see_a_mis_streamed_copy(hip_lib):
    """A torch copy on the wrong stream (scheme A) and a consumer that skips the event wait (scheme B) must come out
    UNEQUAL: side streams do not block against the null stream here, and the delay is long enough.  Fails, never
    skips."""
    out = _child("self_check")
    assert "self-check A, copy on the wrong stream: unequal" in out
    assert "self-check B, consumer without the event: unequal" in out


def test_generators_on_a_side_stream(hip_lib):
    """random_genome_device (n = 257), repeat_genome_device (a hand-made plan that arrives late), simulate_reads_device
    (a genome of 20 000 that arrives late, 300 reads of 100, e = 0.05, with origin_ptr and without)."""
    _child("generators")


def test_sampler_and_split_on_a_side_stream(hip_lib):
    """sample_reads_device and split_reads_device with reads of one length (7) and ragged reads at SPLIT_SHARE + 1 reads,
    the split at G = 3 and 65 and with a row scan of two passes, and the n_reads == 0 forms whose memsets go onto the
    stream; the bases arrive late."""
    _child("sampler_and_split")


def test_counter_on_a_side_stream(hip_lib):
    """KmerCounts.add_device(reserve=False), lookup_device and correct_device on S (k = 21, 300 reads of 100, both offsets
    layouts, cutoff 2, with a score; the reads arrive late), clear(S) followed by add_device on S -- keys of one word
    and of several --, and a counter created and grown while the null stream is held back (covest_kmer_create and
    covest_kmer_reserve wait for the device: exempt, the result is what is pinned)."""
    _child("counter")


def test_partitioned_counter_on_a_side_stream(hip_lib):
    """count_reads_device(stream=S), reads of one length and ragged, against the oracle's histogram and len(); the path
    is "partitioned".  count_reads_device waits for its stream itself, histogram() and len() wait for the device: exempt
    from the blindness condition -- the scheme covers only the first stage of the call and its result.  Then a recount
    on S while the null stream is held back: not exempt (the call waits for S alone), and the later stages' turn."""
    _child("partitioned")


def test_draws_on_a_side_stream(hip_lib):
    """draw_histograms_device with the thresholds arriving late and the output under a late guard pattern (its memset
    is on the stream), counters in LDS and in HBM."""
    _child("draws")


def test_chain_without_a_synchronisation_inside(hip_lib):
    """One delay at the head of S, then random_genome_device, simulate_reads_device, split_reads_device (G = 4),
    add_device(reserve=False), lookup_device, correct_device; S.synchronize(); every buffer of every stage equals the
    same chain made with the host forms."""
    _child("chain")


def test_two_streams_at_once(hip_lib):
    _child("two_streams")


test_two_streams_at_once.__doc__ = case_two_streams.__doc__


def test_grid_repeats_behind_a_late_null_stream(hip_lib):
    """Scheme B on RepeatsModel(21, 100, HIST, tail, max_error=8), tail 0 and 7, kernels "factored" and "direct":
    GRIDS["skip"] (432 points, read in place) and the smallest grid above kArgminSmall (axes, table and plan copied);
    loglikelihoods(), argmin() and scan_records() against a handle evaluated on the null stream, whose values are held
    against K-direct and the oracle by _against_direct (1e-10)."""
    _child("grid_repeats")


def test_grid_basic_behind_a_late_null_stream(hip_lib):
    """Scheme B on a BasicModel: the smallest grid above kArgminSmall (axes only), grids whose evaluation hands points
    back (the strict pass runs on the evaluation's stream when the values are read), a reset that changes an axis
    length, and the reset that issues the memset of the queue counter on the in-place path.  That reset grows the
    arena, which waits for the device: it is exempt from the blindness condition, and pins only the result."""
    _child("grid_basic")


def test_grid_read_back_order_and_two_resets(hip_lib):
    _child("grid_read_back")


test_grid_read_back_order_and_two_resets.__doc__ = case_grid_read_back.__doc__


if __name__ == "__main__":
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    CASES[sys.argv[1]]()
    print("%s ok" % sys.argv[1])
