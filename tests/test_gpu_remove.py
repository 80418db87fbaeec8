"""Counts taken back out of the k-mer table (kmer_remove.hip through KmerCounts.remove* and the C ABI; DESIGN.md section
6an) against the restatement of the definition (tests/remove_reference.py over tests/kmer_reference.py): exact equality
of the histogram, the distinct count, the occupancy and the looked-up abundance of every window, on reads of a 2 000-base
genome with 2 % substitutions (tests/join_reference.py's).

The smallest table covest_kmer_create makes has 2^10 slots (kmer_plan::log2_slots_for), so has_first_slot's condition on
the table's size holds for every table there is: the 2^7 and 2^8 slots its other half would need cannot be made, and the
boundary that can be reached is k = 12 | 13.

Device forms take their buffers from covest_amd.sample._DeviceArena (the runtime the library is bound to).
"""
import ctypes
import functools

import numpy as np
import pytest

import join_reference as jr
import kmer_reference as kr
import remove_reference as rr
from test_gpu_join import add_without_reserve

pytestmark = pytest.mark.gpu

WEIGHTS = (0, 1, 13, 70000)
COVEST_OK = 0   # include/covest_amd.h


class Device:
    def __init__(self):
        from covest_amd.sample import _DeviceArena
        self.arena = _DeviceArena("test_gpu_remove")
        self.n = 0

    def up(self, array):
        a = np.ascontiguousarray(array)
        self.n += 1
        return self.arena.upload("b%d" % self.n, a.ctypes.data, max(a.nbytes, 1))

    def close(self):
        self.arena.close()


@pytest.fixture
def dev(hip_lib):
    d = Device()
    yield d
    d.close()


def seeded_half(n, seed):
    """Which of n reads go: a seeded half."""
    return np.random.default_rng(seed).random(n) < 0.5


def same_state(counts, ref, reads, where):
    """The counter against the restatement: histogram, needed length, distinct, occupancy, and the abundance of every
    window of `reads`."""
    want_hist, want_distinct = ref.histogram()
    assert counts.histogram() == want_hist, where
    assert counts.stats() == (len(want_hist), want_distinct) and len(counts) == want_distinct, where
    assert counts.occupancy() == ref.occupancy(), where
    got = counts.lookup(list(reads), per_window=True)
    for i, want in enumerate(ref.lookup(reads)):
        assert got.windows(i).tolist() == want, (where, i)


def fixed_reads(n, seed, length=100):
    """(n, length) uint8 reads of genome 0 with 2 % substitutions, and the same as strings."""
    strings = jr.noisy_reads(seed, n=n, shortest=length, longest=length)
    return np.frombuffer("".join(strings).encode(), dtype=np.uint8).reshape(n, length).copy(), list(strings)


# ---- 1, 2: key widths, and probe chains past zero-count keys ---------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 12, 13, 21, 31])
def test_key_widths_and_chains_past_zero_counts(hip_lib, k, canonical):
    """k = 5 and 12: no first slot; 13: the smallest with one; 21; 31: the top of one word.  A seeded half of the reads
    is removed: keys whose probe chain runs through a slot of count 0 must still be found, held < occupied; the half
    added back gives the untouched table, in the same slots."""
    from covest_amd.kmer_hist import KmerCounts
    reads = jr.noisy_reads(1)
    gone = seeded_half(len(reads), 10 + k)
    out, stay = [r for r, g in zip(reads, gone) if g], [r for r, g in zip(reads, gone) if not g]
    ref = rr.Table(k, canonical).add(reads)
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        counts.add_reads(reads)
        untouched = (counts.histogram(), counts.stats(), counts.occupancy())
        same_state(counts, ref, reads, (k, canonical, "added"))
        counts.remove(out)
        ref.remove(out)
        same_state(counts, ref, reads, (k, canonical, "half removed"))
        held, occupied = counts.occupancy()
        assert occupied == untouched[2][1] and (held < occupied or k == 5)
        assert counts.histogram() == kr.histogram(stay, k, canonical)[0]
        counts.add_reads(out)
        ref.add(out)
        same_state(counts, ref, reads, (k, canonical, "added back"))
        assert (counts.histogram(), counts.stats(), counts.occupancy()) == untouched
    finally:
        counts.close()


@pytest.mark.parametrize("k", [12, 13])
def test_table_of_1024_slots_near_half_full(hip_lib, k):
    """About 500 keys in 2^10 slots, the table kept at the size it was created with: long chains, on both sides of the
    first slot's boundary."""
    from covest_amd.kmer_hist import KmerCounts
    reads = jr.noisy_reads(3, n=7)
    ref = rr.Table(k, True).add(reads)
    assert 400 <= len(ref.counts) <= 620
    counts = KmerCounts(k, canonical=True, min_slots=1 << 10)
    try:
        add_without_reserve(counts, reads)
        assert counts.slots == 1 << 10
        counts.remove(reads[:4])
        ref.remove(reads[:4])
        same_state(counts, ref, reads, (k, "four of seven removed"))
        add_without_reserve(counts, reads[:2])
        ref.add(reads[:2])
        same_state(counts, ref, reads, (k, "two added back"))
        assert counts.slots == 1 << 10
    finally:
        counts.close()


# ---- 3: reads of their own lengths, reads of one length -----------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_ragged_reads_with_short_and_empty_ones(hip_lib, canonical):
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    g = jr.genome(0)
    short = [g[:k - 1], "", g[40:45], g[100:100 + k - 1], g[:k - 1], g[7:7 + k], ""]
    reads = list(jr.noisy_reads(2, n=120)) + short
    out = short[:3] + reads[:50]
    ref = rr.Table(k, canonical).add(reads)
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        counts.add_reads(reads)
        counts.remove(out)
        ref.remove(out)
        same_state(counts, ref, reads, "short reads removed")
        assert ref.counts[kr._key("", k, canonical)] == 1                      # one of the two empty reads is left
        counts.remove(reads[50:120] + short[3:])                               # ... and now everything else
        assert counts.occupancy() == (0, len(ref.counts)) and counts.histogram() == [0]
    finally:
        counts.close()


@pytest.mark.parametrize("k", [12, 21])
def test_reads_of_one_length_on_the_device(dev, k):
    """301 reads of 100 bases: 80 or 89 windows a read (no multiple of 64), 301 * windows no multiple of 256 -- the
    windows numbered through, more than one workgroup, a last one partly filled.  Unweighted and weighted forms."""
    from covest_amd.kmer_hist import KmerCounts
    n, length = 301, 100
    assert (n * (length - k + 1)) % 256 and (length - k + 1) % 64
    blob, strings = fixed_reads(n, 4)
    d_bases = dev.up(blob)
    w_add = np.array([WEIGHTS[(i * 7) % 4] for i in range(n)], dtype=np.uint32)
    w_sub = np.array([min(int(w), WEIGHTS[(i // 3) % 4]) for i, w in enumerate(w_add)], dtype=np.uint32)
    assert set(w_sub.tolist()) == set(WEIGHTS) and (w_sub < w_add).any()
    d_add, d_sub, d_rest = dev.up(w_add), dev.up(w_sub), dev.up(w_add - w_sub)
    ref = rr.Table(k, True).add(strings).add(strings, w_add)
    counts = KmerCounts(k, canonical=True)
    try:
        counts.add_device(d_bases, n, length)
        counts.add_weighted_device(d_bases, n, length, d_add)
        counts.remove_device(d_bases + 100 * length, 150, length)                 # ranks 100 .. 249, unweighted
        ref.remove(strings[100:250])
        counts.remove_weighted_device(d_bases, n, length, d_sub)
        ref.remove(strings, w_sub)
        same_state(counts, ref, strings[::7], (k, "device forms"))
        counts.remove_weighted_device(d_bases + 3 * length, n - 3, length, d_rest + 4 * 3)   # a sub-range with its weights
        ref.remove(strings[3:], (w_add - w_sub)[3:])
        same_state(counts, ref, strings[:40], (k, "what the weights had left, from read 3 on"))
    finally:
        counts.close()


# ---- 4: weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_weights(hip_lib, canonical):
    """Weights 0, 1, 13 and 70 000 on ragged reads; weight 0 on reads that were never added is no underflow."""
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads = list(jr.noisy_reads(5, n=160))
    strangers = list(jr.noisy_reads(6, n=20, which=1))
    w = np.array([WEIGHTS[(3 * i + i // 7) % 4] for i in range(len(reads))])
    ref = rr.Table(k, canonical).add(reads).add(reads, w)
    counts = KmerCounts(k, canonical=canonical, min_slots=1024)
    try:
        counts.add_reads(reads)
        counts.add_weighted(reads, w)
        same_state(counts, ref, reads[::5], "weighted add")
        counts.remove_weighted(reads + strangers, np.concatenate([w, np.zeros(len(strangers), dtype=np.int64)]))
        ref.remove(reads, w)
        same_state(counts, ref, reads[::5], "weighted removal")
        assert counts.histogram() == kr.histogram(reads, k, canonical)[0]
        part = np.where(np.arange(len(reads)) % 3 == 0, 1, 0)
        counts.remove_weighted(reads, part)
        ref.remove(reads, part)
        same_state(counts, ref, reads[::5], "a third removed by flags")
    finally:
        counts.close()


# ---- 5: removing everything, then other reads --------------------------------------------------------------------------
def test_remove_everything_then_add_others(hip_lib):
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads, others = jr.noisy_reads(1), jr.noisy_reads(6, which=1)
    n_keys = len(kr.count(reads, k, True))
    counts = KmerCounts(k, canonical=True, min_slots=1024)
    try:
        counts.add_reads(reads)
        slots = counts.slots
        counts.remove(reads)
        assert counts.histogram() == [0] and counts.stats() == (1, 0) and counts.occupancy() == (0, n_keys)
        counts.compact()
        assert counts.occupancy() == (0, 0) and counts.slots == slots
        counts.add_reads(others)
        want = kr.histogram(others, k, True)
        assert counts.histogram() == want[0] and counts.occupancy() == (want[1], want[1])
    finally:
        counts.close()


def test_reserve_for_counts_occupied_slots(dev):
    """A table sized for its reads, emptied by removal and fed other reads: _reserve_for sees the slots the zero-count
    keys still take -- 10 457 of them; with the 24 000 occurrences of the next batch they pass half of 2^16 slots, the
    held keys (none) do not -- and compacts instead of growing.  No overflow, and the half-full rule holds after."""
    from covest_amd.kmer_hist import KmerCounts
    k, n, length = 21, 300, 100
    blob, strings = fixed_reads(n, 1)
    blob_b = np.frombuffer("".join(jr.noisy_reads(6, n=n, which=1, shortest=length, longest=length)).encode(), dtype=np.uint8)
    strings_b = list(jr.noisy_reads(6, n=n, which=1, shortest=length, longest=length))
    n_a, n_b = len(kr.count(strings, k, True)), len(kr.count(strings_b, k, True))
    occurrences = n * (length - k + 1)
    slots = 1 << 16
    assert 2 * (n_a + occurrences) + 1024 > slots >= 2 * occurrences + 1024
    d_a, d_b = dev.up(blob), dev.up(blob_b)
    counts = KmerCounts(k, canonical=True, min_slots=slots)
    try:
        counts.add_device(d_a, n, length, reserve=False)
        counts.remove_device(d_a, n, length)
        assert counts.occupancy() == (0, n_a)
        counts.add_device(d_b, n, length)
        assert counts.histogram() == kr.histogram(strings_b, k, True)[0]
        assert counts.occupancy() == (n_b, n_b) and counts.slots == slots
    finally:
        counts.close()


# ---- 6: covest_kmer_reserve after removals -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [12, 21])
def test_reserve_to_a_larger_table_after_removals(hip_lib, k):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    reads = jr.noisy_reads(3, n=7)
    ref = rr.Table(k, True).add(reads)
    counts = KmerCounts(k, canonical=True, min_slots=1 << 10)
    try:
        add_without_reserve(counts, reads)
        counts.remove(reads[:3])
        ref.remove(reads[:3])
        held, occupied = counts.occupancy()
        assert held < occupied
        _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 1 << 10), "covest_kmer_reserve")   # large enough: nothing
        assert counts.occupancy() == (held, occupied) and counts.slots == 1 << 10
        _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 1 << 12), "covest_kmer_reserve")
        assert counts.slots == 1 << 12 and counts.occupancy() == (held, held)
        same_state(counts, ref.compact(), reads, (k, "grown"))
    finally:
        counts.close()


# ---- 7: the join ---------------------------------------------------------------------------------------------------------
def test_join_with_zero_count_keys_on_either_side(hip_lib):
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads_a, reads_b = jr.noisy_reads(1), jr.noisy_reads(2)
    ref_a, ref_b = rr.Table(k, True).add(reads_a), rr.Table(k, True).add(reads_b)
    a, b = KmerCounts(k, canonical=True, min_slots=1024), KmerCounts(k, canonical=True, min_slots=1024)
    try:
        a.add_reads(reads_a)
        b.add_reads(reads_b)
        for side, ref, gone in ((a, ref_a, reads_a[:120]), (b, ref_b, reads_b[100:260])):
            side.remove(gone)
            ref.remove(gone)
            assert side.occupancy()[0] < side.occupancy()[1]
            for x, y, rx, ry in ((a, b, ref_a, ref_b), (b, a, ref_b, ref_a)):
                for rows, cols in ((5, 4), (1, 1), jr.unclipped_shape(rx.held(), ry.held())):
                    got = x.join_histogram(y, rows, cols)
                    assert np.array_equal(got, jr.join(rx.held(), ry.held(), rows, cols)), (rows, cols)
                    assert got[0, 0] == 0 or (rows, cols) == (1, 1)
                    assert got.sum() == len(set(rx.held()) | set(ry.held()))
        zero_both = {x for x, n in ref_a.counts.items() if n == 0} & {x for x, n in ref_b.counts.items() if n == 0}
        assert zero_both   # keys that occupy a slot on both sides and are held by neither: in no cell
    finally:
        a.close()
        b.close()


# ---- 8: underflow --------------------------------------------------------------------------------------------------------
def test_underflow_is_a_status(hip_lib, dev):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads = list(jr.noisy_reads(1, n=40))
    strangers = list(jr.noisy_reads(6, n=5, which=1))
    counts = KmerCounts(k, canonical=True, min_slots=1024)
    other = KmerCounts(k, canonical=True, min_slots=1024)
    try:
        counts.add_reads(reads)
        other.add_reads(reads)
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_remove.*underflow"):
            counts.remove(strangers)                              # never added: the host form says so itself
        for _ in range(2):
            with pytest.raises(_capi.CovestHipError, match="covest_kmer_histogram.*underflow"):
                counts.histogram()
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_reserve.*underflow"):     # sticky across a reserve
            _capi.check(hip_lib.covest_kmer_reserve(counts._handle, 1 << 14), "covest_kmer_reserve")
        assert hip_lib.covest_kmer_reserve(counts._handle, 1 << 14) == _capi.COVEST_E_INVALID
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_compact.*underflow"):
            counts.compact()
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_lookup_reads.*underflow"):
            counts.lookup(reads[:2])
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_join_histogram.*underflow"):
            counts.join_histogram(other, 3, 3)
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_join_histogram.*underflow"):
            other.join_histogram(counts, 3, 3)
        with pytest.raises(_capi.CovestHipError, match="underflow"):
            counts.add_reads(reads[:1])                           # an add does not erase it
        with pytest.raises(_capi.CovestHipError, match="underflow"):
            counts.histogram()
        counts.clear()                                            # gone after clear()
        assert counts.histogram() == [0]
        counts.add_reads(reads)
        assert counts.histogram() == other.histogram()
        # a weight larger than the held count does the same; the device form never looks, the next histogram does
        blob, strings = fixed_reads(8, 7)
        d_bases, d_w = dev.up(blob), dev.up(np.array([1, 1, 1, 2, 1, 1, 1, 1], dtype=np.uint32))
        counts.clear()
        counts.add_device(d_bases, 8, 100)
        counts.remove_weighted_device(d_bases, 8, 100, d_w)
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_histogram.*underflow"):
            counts.histogram()
        counts.clear()
        counts.add_weighted(strings, [3] * 8)
        with pytest.raises(_capi.CovestHipError, match="covest_kmer_remove_weighted.*underflow"):
            counts.remove_weighted(strings, [3, 3, 3, 3, 3, 4, 3, 3])
    finally:
        counts.close()
        other.close()


def test_an_overflow_before_an_underflow_is_still_reported(hip_lib):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    counts = KmerCounts(21, canonical=True, min_slots=1 << 10)
    try:
        with pytest.raises(_capi.CovestHipError, match="overflow"):
            add_without_reserve(counts, jr.noisy_reads(1))        # thousands of keys into 2^10 slots
        with pytest.raises(_capi.CovestHipError) as e:
            counts.remove(list(jr.noisy_reads(6, n=5, which=1)))
        assert "overflow" in str(e.value)
        rc = hip_lib.covest_kmer_histogram(counts._handle, None, 0, None, None)
        assert rc == _capi.COVEST_E_NOMEM and "overflow" in _capi.last_error()
        counts.clear()
        assert counts.histogram() == [0]
    finally:
        counts.close()


# ---- 9: refusals, each naming its call --------------------------------------------------------------------------------------
def _calls(lib, handle, d_bases=0, d_weights=0):
    blob = np.frombuffer(b"ACGT" * 25, dtype=np.uint8).copy()
    offsets = np.array([0, 100], dtype=np.int64)
    w = np.ones(1, dtype=np.uint32)
    out = (ctypes.c_int64 * 2)()
    vp = ctypes.c_void_p
    return {
        "covest_kmer_remove": lambda: lib.covest_kmer_remove(handle, vp(blob.ctypes.data), vp(offsets.ctypes.data), 1),
        "covest_kmer_remove_weighted": lambda: lib.covest_kmer_remove_weighted(handle, vp(blob.ctypes.data),
                                                                               vp(offsets.ctypes.data), 1, vp(w.ctypes.data)),
        "covest_kmer_remove_device": lambda: lib.covest_kmer_remove_device(handle, vp(d_bases), None, 1, 100, None),
        "covest_kmer_remove_weighted_device": lambda: lib.covest_kmer_remove_weighted_device(handle, vp(d_bases), None, 1, 100,
                                                                                             vp(d_weights), None),
        "covest_kmer_occupancy": lambda: lib.covest_kmer_occupancy(handle, out),
        "covest_kmer_compact": lambda: lib.covest_kmer_compact(handle),
    }


def test_refusals_name_their_call(hip_lib, dev):
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    blob, _ = fixed_reads(300, 8)
    d_bases, d_w = dev.up(blob), dev.up(np.ones(300, dtype=np.uint32))
    wide, bulk, plain = KmerCounts(32), KmerCounts(21, canonical=True), KmerCounts(21)
    try:
        for name, call in _calls(hip_lib, wide._handle, d_bases, d_w).items():       # k = 32
            assert call() == _capi.COVEST_E_UNSUPPORTED and _capi.last_error().startswith(name + ":"), name
        assert bulk.count_reads_device(d_bases, 300, 100) == "partitioned"
        for name, call in _calls(hip_lib, bulk._handle, d_bases, d_w).items():       # a partitioned result
            assert call() == _capi.COVEST_E_INVALID, name
            assert _capi.last_error().startswith(name + ":") and "covest_kmer_count_reads_device" in _capi.last_error(), name
        for name, call in _calls(hip_lib, None, d_bases, d_w).items():               # a null counter
            assert call() == _capi.COVEST_E_INVALID and _capi.last_error().startswith(name + ":"), name
        vp, h = ctypes.c_void_p, plain._handle
        offsets = np.array([0, 100], dtype=np.int64)
        null_and_misaligned = {
            "covest_kmer_remove": lambda: hip_lib.covest_kmer_remove(h, vp(blob.ctypes.data), None, 1),
            "covest_kmer_remove_device": lambda: hip_lib.covest_kmer_remove_device(h, None, None, 1, 100, None),
            "covest_kmer_remove_weighted": lambda: hip_lib.covest_kmer_remove_weighted(h, vp(blob.ctypes.data),
                                                                                       vp(offsets.ctypes.data), 1, None),
            "covest_kmer_remove_weighted_device": lambda: hip_lib.covest_kmer_remove_weighted_device(h, vp(d_bases), None, 1, 100,
                                                                                                     vp(d_w + 2), None),
            "covest_kmer_occupancy": lambda: hip_lib.covest_kmer_occupancy(h, None),
        }
        for name, call in null_and_misaligned.items():
            assert call() == _capi.COVEST_E_INVALID and _capi.last_error().startswith(name + ":"), name
        assert hip_lib.covest_kmer_remove_weighted(h, vp(blob.ctypes.data), vp(offsets.ctypes.data), 1,
                                                   vp(blob.ctypes.data + 1)) == _capi.COVEST_E_INVALID
        assert "aligned" in _capi.last_error()
        assert hip_lib.covest_kmer_remove_weighted_device(h, vp(d_bases), None, 1, 100, None, None) == _capi.COVEST_E_INVALID
        assert "null weights" in _capi.last_error()
        assert plain.histogram() == [0]   # none of the refused calls touched the counter
        with pytest.raises(ValueError, match="31"):
            from covest_amd.jackknife import leave_group_out_histograms
            leave_group_out_histograms(blob, 32, 4, route="remove")
    finally:
        for c in (wide, bulk, plain):
            c.close()


def _add_calls(lib, handle, d_bases=0, d_weights=0, bases="blob", offsets=(0, 100), weights="ones", n_reads=1):
    """The four add forms on one read of 100 bases, by name.  bases / weights None: a null pointer; weights "odd": a
    pointer that is no multiple of 4.  The arrays live as long as the lambdas do."""
    blob = np.frombuffer(b"ACGT" * 25, dtype=np.uint8).copy()
    offs = None if offsets is None else np.array(offsets, dtype=np.int64)
    ones = np.ones(2, dtype=np.uint32)
    vp = ctypes.c_void_p
    h_bases = vp(blob.ctypes.data) if bases is not None else None
    h_offs = vp(offs.ctypes.data) if offs is not None else None
    h_w = {None: None, "ones": vp(ones.ctypes.data), "odd": vp(ones.ctypes.data + 1)}[weights]
    d_b = vp(d_bases) if bases is not None else None
    d_w = {None: None, "ones": vp(d_weights), "odd": vp(d_weights + 2)}[weights]
    keep = (blob, offs, ones)
    u8p, i64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)   # (covest_kmer_add's prototype is typed)
    return {
        "covest_kmer_add": lambda keep=keep: lib.covest_kmer_add(handle, h_bases and ctypes.cast(h_bases, u8p),
                                                                 h_offs and ctypes.cast(h_offs, i64p), n_reads),
        "covest_kmer_add_weighted": lambda keep=keep: lib.covest_kmer_add_weighted(handle, h_bases, h_offs, n_reads, h_w),
        "covest_kmer_add_device": lambda: lib.covest_kmer_add_device(handle, d_b, None, n_reads, 100, None),
        "covest_kmer_add_weighted_device": lambda: lib.covest_kmer_add_weighted_device(handle, d_b, None, n_reads, 100, d_w,
                                                                                       None),
    }


ADD_FORMS = ("covest_kmer_add", "covest_kmer_add_weighted", "covest_kmer_add_device", "covest_kmer_add_weighted_device")
HOST_ADDS, WEIGHTED_ADDS = ADD_FORMS[:2], ADD_FORMS[1::2]
BULK_TEXT = (": the counter holds a covest_kmer_count_reads_device result (its keys are not in the table); "
             "covest_kmer_clear first")


def test_refusals_of_the_add_forms(hip_lib, dev):
    """Return code and the whole covest_last_error text of the four add forms under every refusal they have, as the
    forms stood before they went over one host path: the host forms report a partitioned result
    under the name of their device form; the host forms call null bases "bad offsets", the device forms "bad argument".
    Keys of two words are added by all four; no reads is no work and no error."""
    from covest_amd import _capi
    from covest_amd.kmer_hist import KmerCounts
    blob, _ = fixed_reads(300, 8)
    d_bases, d_w = dev.up(blob), dev.up(np.ones(300, dtype=np.uint32))
    wide, bulk, plain = KmerCounts(32), KmerCounts(21, canonical=True), KmerCounts(21)
    invalid = _capi.COVEST_E_INVALID

    def refused(calls, texts):
        for name, text in texts.items():
            assert calls[name]() == invalid, name
            assert _capi.last_error() == text, name

    try:
        refused(_add_calls(hip_lib, None, d_bases, d_w), {name: name + ": bad argument" for name in ADD_FORMS})
        assert bulk.count_reads_device(d_bases, 300, 100) == "partitioned"
        device_form = {"covest_kmer_add": "covest_kmer_add_device", "covest_kmer_add_weighted": "covest_kmer_add_weighted_device"}
        refused(_add_calls(hip_lib, bulk._handle, d_bases, d_w),
                {name: device_form.get(name, name) + BULK_TEXT for name in ADD_FORMS})
        h = plain._handle
        refused(_add_calls(hip_lib, h, d_bases, d_w, bases=None),                       # null bases, one read
                {name: name + (": bad offsets" if name in HOST_ADDS else ": bad argument") for name in ADD_FORMS})
        refused(_add_calls(hip_lib, h, d_bases, d_w, offsets=None), {name: name + ": bad argument" for name in HOST_ADDS})
        refused(_add_calls(hip_lib, h, d_bases, d_w, weights=None), {name: name + ": null weights" for name in WEIGHTED_ADDS})
        refused(_add_calls(hip_lib, h, d_bases, d_w, weights="odd"),
                {name: name + ": the weights must be aligned to 4 bytes" for name in WEIGHTED_ADDS})
        refused(_add_calls(hip_lib, h, d_bases, d_w, offsets=(100, 0)), {name: name + ": bad offsets" for name in HOST_ADDS})
        assert plain.histogram() == [0]   # none of the refused calls touched the counter
        # no reads: nothing to look at, whatever the pointers
        for kwargs in ({}, {"bases": None, "offsets": None, "weights": None}):
            for name, call in _add_calls(hip_lib, h, d_bases, d_w, n_reads=0, **kwargs).items():
                assert call() == COVEST_OK, (name, kwargs)
        assert plain.histogram() == [0]
        # k = 32: all four forms add
        for name, call in _add_calls(hip_lib, wide._handle, d_bases, d_w).items():
            assert call() == COVEST_OK, (name, _capi.last_error())
        on_host, on_device = "ACGT" * 25, blob[0].tobytes().decode()
        assert wide.histogram() == kr.histogram([on_host, on_host, on_device, on_device], 32)[0]
    finally:
        for c in (wide, bulk, plain):
            c.close()


# ---- 9b: add and removal through every branch of the walk they share ---------------------------------------------------------
WALK_GENOME = 400   # bases: a few hundred keys, so that 2^10 slots hold the ragged and the one-length reads together


def walk_reads(k):
    """(ragged, fixed): three reads of each of the lengths 0, 1, k - 1, k, k + 1, k + 63, k + 64, k + 65 -- the
    short-read key, one window, and both sides of a lane's second round -- and as many reads of k + 64 bases, all from
    the first WALK_GENOME bases of the genome."""
    rng = np.random.default_rng(400 + k)
    g = jr.genome(0)[:WALK_GENOME]

    def cut(length):
        at = int(rng.integers(0, len(g) - length + 1))
        return g[at:at + length]

    lengths = [0, 1, k - 1, k, k + 1, k + 63, k + 64, k + 65] * 3
    return [cut(n) for n in lengths], [cut(k + 64) for _ in lengths]


def _host_call(fn, name, handle, reads, weights=None):
    from covest_amd import _capi
    blob = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    args = (handle, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            len(reads))
    if weights is not None:
        args += (ctypes.c_void_p(weights.ctypes.data),)
    _capi.check(fn(*args), name)


@pytest.mark.parametrize("k", [12, 13, 31])
def test_add_and_removal_through_every_branch_of_the_walk(hip_lib, dev, k):
    """One table of 2^10 slots, canonical; k = 12 | 13 is where has_first_slot switches, 31 the top of one word.
    Weighted add, weighted removal of the same, unweighted add: the histogram of the unweighted reads -- on ragged
    reads through the host forms (a wave a read: empty, shorter than k, one window, a lane's second round) and on reads
    of one length through the (n, L) device forms (the windows numbered through).  Weights 0, 1, 2, ...; the read of
    weight 0 of the removal is one the table never saw.  Then everything removed: no key held, every slot still
    occupied.  No underflow anywhere: every host form would say so."""
    from covest_amd.kmer_hist import KmerCounts
    lib = hip_lib
    ragged, fixed = walk_reads(k)
    n, length = len(fixed), k + 64
    stranger = jr.genome(1)[:k + 65]
    w = np.arange(n, dtype=np.uint32)
    assert w[0] == 0 and not set(kr.count([stranger], k, True)) & set(kr.count(ragged + fixed, k, True))
    fixed_blob = np.frombuffer("".join(fixed).encode(), dtype=np.uint8).reshape(n, length).copy()
    stranger_blob = fixed_blob.copy()
    stranger_blob[0] = np.frombuffer(stranger[:length].encode(), dtype=np.uint8)
    d_fixed, d_stranger, d_w = dev.up(fixed_blob), dev.up(stranger_blob), dev.up(w)
    counts = KmerCounts(k, canonical=True, min_slots=1 << 10)
    try:
        h = counts._handle
        _host_call(lib.covest_kmer_add_weighted, "covest_kmer_add_weighted", h, ragged, w)
        _host_call(lib.covest_kmer_remove_weighted, "covest_kmer_remove_weighted", h, [stranger] + ragged[1:], w)
        _host_call(lib.covest_kmer_add, "covest_kmer_add", h, ragged)
        want = kr.histogram(ragged, k, True)
        assert counts.histogram() == want[0]
        held, occupied = counts.occupancy()
        assert held == want[1] and occupied >= held
        counts.add_weighted_device(d_fixed, n, length, d_w, reserve=False)
        counts.remove_weighted_device(d_stranger, n, length, d_w)
        counts.add_device(d_fixed, n, length, reserve=False)
        want = kr.histogram(ragged + fixed, k, True)
        assert counts.histogram() == want[0]
        held, occupied = counts.occupancy()
        assert held == want[1] and occupied >= held
        counts.remove_device(d_fixed, n, length)
        _host_call(lib.covest_kmer_remove, "covest_kmer_remove", h, ragged)
        assert counts.stats() == (1, 0) and counts.histogram() == [0]
        assert counts.occupancy() == (0, occupied) and counts.slots == 1 << 10
    finally:
        counts.close()


# ---- 10: replace_reads -----------------------------------------------------------------------------------------------------
def test_replace_reads_after_a_correction(hip_lib):
    """correct()'s output and the reads it changed feed replace_reads: the table then equals a fresh count of the
    corrected reads."""
    from covest_amd.kmer_hist import KmerCounts
    k = 21
    reads = list(jr.noisy_reads(9, n=300, rate=0.01))
    counts, fresh = KmerCounts(k, canonical=True), KmerCounts(k, canonical=True)
    try:
        counts.add_reads(reads)
        fixed = counts.correct(reads, cutoff=3)
        after = fixed.strings()
        changed = np.array([a != b for a, b in zip(reads, after)])
        assert changed.any() and not changed.all()
        counts.replace_reads(reads, (fixed.bases, fixed.offsets), changed)
        fresh.add_reads(after)
        want = kr.histogram(after, k, True)
        assert counts.histogram() == fresh.histogram() == want[0] and len(counts) == want[1]
        assert counts.occupancy()[1] >= counts.occupancy()[0] == want[1]
        got, ref = counts.lookup(after), fresh.lookup(after)
        assert np.array_equal(got.abundance, ref.abundance) and np.array_equal(got.summary, ref.summary)
    finally:
        counts.close()
        fresh.close()


# ---- 11: the jackknife's routes ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jackknife_reads(ragged):
    if ragged:
        strings = list(jr.noisy_reads(11, n=400)) + ["", jr.genome(0)[:9]]
        blob = np.frombuffer("".join(strings).encode(), dtype=np.uint8)
        offsets = np.zeros(len(strings) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in strings], out=offsets[1:])
        return blob, offsets
    return fixed_reads(401, 12)[0]


@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("groups", [2, 5, 32])
def test_leave_group_out_routes_agree(hip_lib, monkeypatch, groups, ragged):
    from covest_amd import jackknife
    from covest_amd.read_sets import ResidentReads
    left = []
    leave = ResidentReads.__exit__

    def exit_and_note(self, *exc):
        if self.counts is not None:
            left.append(self.histogram())   # what the counter holds when the loop is over
        return leave(self, *exc)

    monkeypatch.setattr(ResidentReads, "__exit__", exit_and_note)
    reads = jackknife_reads(ragged)
    recount = jackknife.leave_group_out_histograms(reads, 21, groups, seed=5, canonical=True)
    remove = jackknife.leave_group_out_histograms(reads, 21, groups, seed=5, canonical=True, route="remove")
    assert recount[0] == remove[0] and recount[2] == remove[2] and len(remove[1]) == groups
    for g, (a, b) in enumerate(zip(recount[1], remove[1])):
        assert a == b, g
    assert left[1] == remove[0]   # all reads are back in the counter
    assert len({tuple(sorted(h.items())) for h in remove[1]}) > 1


@functools.lru_cache(maxsize=None)
def fitted():
    """(reads, model, estimate) of the basic model on simulated reads: 20 000-base genome, coverage 10, e = 0.02, k = 15."""
    from covest_amd import constants, simulate as sim
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import compute_coverage_apx
    from covest_amd.kmer_hist import KmerCounts
    from covest_amd.models import BasicModel
    g = sim.random_genome(20_000, 21)
    reads = sim.simulate_reads(g, 100, coverage=10, error_rate=0.02, seed=21, both_strands=False)
    counts = reads.add_to(KmerCounts(15))
    hist = {i: int(v) for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    model = BasicModel(15, 100, hist, 0, max_error=constants.MAX_ERRORS)
    est, ok = CoverageEstimator(model).compute_coverage(list(compute_coverage_apx(hist, 15, 100)))
    assert ok
    return reads, model, [float(v) for v in est]


def test_read_jackknife_routes_agree_bit_for_bit(hip_lib):
    from covest_amd import jackknife
    reads, model, est = fitted()
    a = jackknife.read_jackknife(model, est, reads, groups=4, seed=3)
    b = jackknife.read_jackknife(model, est, reads, groups=4, seed=3, route="remove")
    assert "route" not in a and b["route"] == "remove"
    assert a["estimates"].tobytes() == b["estimates"].tobytes() and a["full_estimate"] == b["full_estimate"]
    assert a["standard_errors"] == b["standard_errors"] and a["intervals"] == b["intervals"] and a["bias"] == b["bias"]
    assert a["occurrences"] == b["occurrences"] and a["group_sizes"] == b["group_sizes"]
    assert all(v is not None and v > 0 for v in b["standard_errors"].values())
