"""Stream order made visible (TEST INFRASTRUCTURE ONLY; not collected): what tests/test_gpu_streams.py builds its cases
from.  Used inside a child process that imported torch first (one HIP runtime a process).

On the null stream a launch that lost its `stream` argument, a memset issued on nullptr or a missing hipStreamWaitEvent
all give the right answer.  Two schemes make them give a wrong one:

  A, "late inputs": the buffers hold poison -- valid inputs of the same sizes -- and a side stream S holds a bounded
     busy-wait (`delay`), then device-to-device copies of the true inputs (and of the guard pattern into the outputs),
     then the entry point under test.  Only S is waited for.  Whatever the entry point issued on another stream than S
     ran at once, on the poison or under the guard pattern, and the outputs differ.
  B, "late null stream": the delay sits on the null stream, where a grid handle stages what it uploads; an evaluation
     on S that does not wait for the handle's event reads what the previous configuration left behind.

A case tests something only while the host runs ahead of the delay: `Delay.check_blind` asserts that the host time from
the enqueue of the delay to the return of the last call under test is below half the delay the events measured.

Every figure is printed as a line that begins with "stream-order:" (profiles/stream_order.txt is made of them).
"""
import time

import numpy as np
import torch

DELAY_MS = 100.0   # a delay of bounded length, not a hang: nothing waits on anything that cannot finish
_rate = None       # torch.cuda._sleep cycles per millisecond on this device, measured once per process

# the poison of a buffer of bases: every base another base (A -> C -> G -> T -> A, in either case), every other byte kept
_ROTATE = np.arange(256, dtype=np.uint8)
for _a, _b in zip("ACGTacgt", "CGTAcgta"):
    _ROTATE[ord(_a)] = ord(_b)


def other_bases(bases):
    """`bases` (uint8, any shape) with every base replaced by another one: the same lengths, valid input, and no read,
    k-mer or genome slice equal to the true one."""
    return _ROTATE[np.asarray(bases, dtype=np.uint8)]


def side_stream():
    """A stream of torch's own making.  PyTorch creates these non-blocking with respect to the null stream; nothing here
    relies on it: the self-check of tests/test_gpu_streams.py proves it."""
    return torch.cuda.Stream()


def null_stream():
    return torch.cuda.default_stream()


def _cycles_per_ms():
    global _rate
    if _rate is None:
        torch.cuda._sleep(1000)  # (the kernel's first launch is not timed)
        torch.cuda.synchronize()
        cycles, ms = 1 << 20, 0.0
        for _ in range(8):  # a sleep long enough for the events' resolution: 2 ms and more
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            torch.cuda._sleep(cycles)
            end.record()
            end.synchronize()
            ms = begin.elapsed_time(end)
            if ms >= 2.0:
                break
            cycles *= 8
        if not ms > 0.0:
            raise RuntimeError("torch.cuda._sleep(%d) took no measurable time" % cycles)
        _rate = cycles / ms
        print("stream-order: calibration %d cycles in %.3f ms" % (cycles, ms))
    return _rate


class Delay:
    """A busy-wait of about `ms` milliseconds enqueued on `stream`, between two timed events.  `ms()`: what the events
    measured (waits for the delay's end); `host_ms()`: host time since the enqueue; `check_blind(issued_ms, what)`: the
    blindness condition, `issued_ms` = host_ms() taken at the return of the last call under test."""

    def __init__(self, stream, ms=DELAY_MS):
        cycles = int(ms * _cycles_per_ms())
        self.begin, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            self.begin.record(stream)
            torch.cuda._sleep(cycles)
            self.end.record(stream)

    def ms(self):
        self.end.synchronize()
        return self.begin.elapsed_time(self.end)

    def host_ms(self):
        return (time.perf_counter() - self.t0) * 1e3

    def check_blind(self, issued_ms, what, exempt=None):
        measured = self.ms()
        print("stream-order: %s: delay %.1f ms, host issue %.2f ms%s" % (what, measured, issued_ms,
                                                                         " (exempt: %s)" % exempt if exempt else ""))
        if exempt:
            return measured
        assert issued_ms < 0.5 * measured, (
            "%s has tested nothing: the host took %.1f ms from the enqueue of the delay to the return of the last call, "
            "and the delay lasted %.1f ms -- a call waited for the device, or the delay is too short" % (what, issued_ms, measured))
        return measured


def delay(stream, ms=DELAY_MS):
    """Enqueue the busy-wait on `stream`; the Delay's ms() is the length the events measured."""
    return Delay(stream, ms)


def late(stream, copies, ms=DELAY_MS):
    """Scheme A, steps 2 and 3: the delay on `stream`, then `copies` -- (destination, source) pairs of device tensors --
    on `stream` behind it.  The true inputs arrive late; so does the guard pattern of an output (a memset of the entry
    point that ran too early is then overwritten).  Returns the Delay."""
    d = delay(stream, ms)
    with torch.cuda.stream(stream):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
    return d


def to_device(array):
    """A host array as a device tensor of the same bytes (uint64 / uint32 as their signed twins: torch has no others)."""
    a = np.ascontiguousarray(array)
    twins = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    if a.dtype in twins:
        a = a.view(twins[a.dtype])
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
