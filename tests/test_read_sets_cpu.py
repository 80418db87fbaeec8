"""The host side of the read-level resampling (jackknife.py, read_bootstrap.py, report.py) without library or device:
recording stand-ins take the place of sample._DeviceArena, kmer_hist.KmerCounts, sample.split_reads_device and
read_bootstrap.bootstrap_weights_device, and what is held fixed is what a caller or the device can observe -- every
arena and counter call with its arguments and in its order, the closing order when a loop raises, the device check's
text, the keys read_jackknife and read_bootstrap share, and the record print_output writes for both."""
import ctypes
import sys

import numpy as np
import pytest

SEED = 5
K = 5
# the stand-in arena's buffers: a fixed address a name
IN, OFF, OUT, OUT_OFF, FIRST, W = (i << 20 for i in range(1, 7))
ADDRESS = {"in": IN, "offsets": OFF, "out": OUT, "out_offsets": OUT_OFF, "group_first": FIRST, "weights": W}


def put(monkeypatch, name, value):
    """`value` under `name` in every module of the package that holds the name (a module that imported it by name has
    a reference of its own)."""
    import covest_amd.bootstrap, covest_amd.jackknife, covest_amd.read_bootstrap  # noqa: E401,F401  (they bring the others in)
    for module in ("sample", "kmer_hist", "bootstrap", "jackknife", "read_bootstrap", "read_sets"):
        module = sys.modules.get("covest_amd." + module)
        if module is not None and hasattr(module, name):
            monkeypatch.setattr(module, name, value)


class Recorder:
    """The stand-ins, writing to one log.  `current`: the device hipGetDevice reports; `fail_clear`: the clear (counted
    from 1) that raises; `no_room`: the arena buffer whose reservation fails."""

    def __init__(self, monkeypatch, current=0, fail_clear=None, no_room=None):
        from covest_amd import _capi
        log = self.log = []
        state = {"histograms": 0, "clears": 0, "replicate": 0}

        class Hip:
            @staticmethod
            def hipGetDevice(ref):
                log.append(("hipGetDevice",))
                ref._obj.value = current
                return 0

        class Arena:
            def __init__(self, who="sampled_histogram"):
                log.append(("arena", who))
                self.hip = Hip()

            def reserve(self, name, n_bytes):
                log.append(("reserve", name, n_bytes))
                if name == no_room:
                    raise _capi.CovestHipError("stand-in: hipMalloc failed (HIP error 2)")
                return ADDRESS[name]

            def upload(self, name, host_ptr, n_bytes):
                log.append(("upload", name, n_bytes, ctypes.string_at(host_ptr, n_bytes)))
                return ADDRESS[name]

            def download(self, name, array):
                log.append(("download", name, array.nbytes))
                if name == "group_first":  # group 1 is empty, and so the ranks before group 0 and behind the last
                    array[:] = [0, 2] + [2] * (array.size - 3) + [state["n"]]
                else:
                    array[:] = np.arange(array.size) + state["replicate"]

            def close(self):
                log.append(("arena.close",))

        class Counts:
            def __init__(self, k=20, canonical=False, device=-1, min_slots=1 << 16):
                log.append(("KmerCounts", k, canonical, device))

            def _reserve_for(self, n_new):
                log.append(("_reserve_for", n_new))

            def add_device(self, d_bases_ptr, n_reads, read_len, d_offsets_ptr=None, stream=None, reserve=True):
                log.append(("add_device", d_bases_ptr, n_reads, read_len, d_offsets_ptr, stream, reserve))

            def add_weighted_device(self, d_bases_ptr, n_reads, read_len, d_weights_ptr, d_offsets_ptr=None, stream=None,
                                    reserve=True):
                log.append(("add_weighted_device", d_bases_ptr, n_reads, read_len, d_weights_ptr, d_offsets_ptr, stream, reserve))

            def clear(self, stream=None):
                log.append(("clear", stream))
                state["clears"] += 1
                if state["clears"] == fail_clear:
                    raise RuntimeError("stand-in: clear failed")

            def histogram(self):
                log.append(("histogram",))
                state["histograms"] += 1
                return [0, 4 + state["histograms"], 0, 2]

            def close(self):
                log.append(("counts.close",))

        def split(bases_ptr, n_reads, out_bases_ptr, group_first_ptr, groups, seed=0, first_read=0, read_len=0,
                  offsets_ptr=None, out_offsets_ptr=None, read_index_ptr=None, stream=None, device=-1):
            state["n"] = n_reads
            log.append(("split", bases_ptr, n_reads, out_bases_ptr, group_first_ptr, groups, seed, first_read, read_len,
                        offsets_ptr, out_offsets_ptr, read_index_ptr, stream, device))

        def weights(out_ptr, n_reads, replicate, seed=0, first_read=0, stream=None, device=-1):
            state["replicate"] = replicate
            log.append(("weights", out_ptr, n_reads, replicate, seed, first_read, stream, device))

        put(monkeypatch, "_DeviceArena", Arena)
        put(monkeypatch, "KmerCounts", Counts)
        put(monkeypatch, "split_reads_device", split)
        put(monkeypatch, "bootstrap_weights_device", weights)


def hist(c):
    """The stand-in counter's c-th histogram (from 1) as {abundance: k-mers}; its occurrences are 10 + c."""
    return {1: 4 + c, 3: 2}


def fixed_reads():
    return np.frombuffer(b"ACGTTGCAACGG" * 6, dtype=np.uint8).reshape(6, 12).copy()


def ragged_reads():
    """Five reads of 4, 0, 7, 3 and 9 bases: an empty one, and two shorter than K."""
    return np.frombuffer(b"ACGT" b"" b"ACGTACG" b"TTT" b"GATTACAGA", dtype=np.uint8).copy(), np.array([0, 4, 4, 11, 14, 23])


def simulated_reads():
    from covest_amd.simulate import SimulatedReads
    return SimulatedReads(fixed_reads(), np.arange(6, dtype=np.int64) << 1 | 1, 1000, 0.0, 3, first_read=7)


def jackknife_calls(ragged, n, step, first_read, device, canonical, blob, offsets, reserve):
    """What leave_group_out_histograms asks of arena, split and counter at 3 groups, the split's boundaries [0, 2, 2, n]:
    `step` the bytes a rank takes in the buffer the sub-ranges move in (the read length, or 8 in the offsets)."""
    def add(lo, hi):
        if ragged:
            return ("add_device", OUT, hi - lo, 0, OUT_OFF + step * lo, None, False)
        return ("add_device", OUT + step * lo, hi - lo, step, None, None, False)
    calls = [("arena", "leave_group_out_histograms")] + ([("hipGetDevice",)] if device >= 0 else [])
    calls += [("upload", "in", len(blob), blob)] + ([("upload", "offsets", 8 * (n + 1), offsets)] if ragged else [])
    calls += [("reserve", "out", len(blob))] + ([("reserve", "out_offsets", 8 * (n + 1))] if ragged else [])
    calls += [("reserve", "group_first", 32),
              ("split", IN, n, OUT, FIRST, 3, SEED, first_read, 0 if ragged else step, OFF if ragged else None,
               OUT_OFF if ragged else None, None, None, device),
              ("download", "group_first", 32),
              ("KmerCounts", K, canonical, device), ("_reserve_for", reserve),
              add(0, n), ("histogram",),
              ("clear", None), add(2, n), ("histogram",),                # group 0: no rank before it
              ("clear", None), add(0, 2), add(2, n), ("histogram",),     # group 1: empty
              ("clear", None), add(0, 2), ("histogram",),                # group 2: no rank behind it
              ("counts.close",), ("arena.close",)]
    return calls


def bootstrap_calls(ragged, n, read_len, first_read, device, canonical, blob, offsets, reserve):
    """What bootstrap_histograms asks of arena, generator and counter at 3 replicates."""
    d_off = OFF if ragged else None
    calls = [("arena", "bootstrap_histograms")] + ([("hipGetDevice",)] if device >= 0 else [])
    calls += [("upload", "in", len(blob), blob)] + ([("upload", "offsets", 8 * (n + 1), offsets)] if ragged else [])
    calls += [("reserve", "weights", 4 * n), ("KmerCounts", K, canonical, device), ("_reserve_for", reserve),
              ("add_device", IN, n, read_len, d_off, None, False), ("histogram",)]
    for b in range(3):
        calls += [("weights", W, n, b, SEED, first_read, None, device), ("clear", None),
                  ("add_weighted_device", IN, n, read_len, W, d_off, None, False), ("histogram",),
                  ("download", "weights", 4 * n)]
    return calls + [("counts.close",), ("arena.close",)]


def cases():
    """(name, reads, ragged, n, read length, first_read, device, canonical, blob, offsets' bytes, _reserve_for's amount)"""
    bases, offsets = ragged_reads()
    plain = fixed_reads().tobytes()
    return [
        ("array", fixed_reads(), False, 6, 12, 0, -1, False, plain, None, 6 * (12 - K + 1)),
        ("ragged", (bases, offsets), True, 5, 0, 0, -1, False, bases.tobytes(), offsets.astype(np.int64).tobytes(), 23 + 5),
        ("simulated", simulated_reads(), False, 6, 12, 7, 0, True, plain, None, 6 * (12 - K + 1)),
    ]


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_leave_group_out_call_sequence(monkeypatch, case):
    from covest_amd import jackknife
    _, reads, ragged, n, read_len, first_read, device, canonical, blob, offsets, reserve = case
    rec = Recorder(monkeypatch)
    full, hists, occ = jackknife.leave_group_out_histograms(reads, K, 3, seed=SEED, canonical=canonical, device=device)
    assert rec.log == jackknife_calls(ragged, n, 8 if ragged else read_len, first_read, device, canonical, blob, offsets, reserve)
    assert full == hist(1) and hists == [hist(2), hist(3), hist(4)] and occ == [12, 13, 14]
    first = jackknife._leave_group_out(reads, K, 3, SEED, canonical, device)[3]
    assert first.dtype == np.int64 and first.tolist() == [0, 2, 2, n]


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_bootstrap_histograms_call_sequence(monkeypatch, case):
    from covest_amd.read_bootstrap import bootstrap_histograms
    _, reads, ragged, n, read_len, first_read, device, canonical, blob, offsets, reserve = case
    rec = Recorder(monkeypatch)
    full, hists, occ, drawn = bootstrap_histograms(reads, K, 3, seed=SEED, canonical=canonical, device=device)
    assert rec.log == bootstrap_calls(ragged, n, read_len, first_read, device, canonical, blob, offsets, reserve)
    assert full == hist(1) and hists == [hist(2), hist(3), hist(4)] and occ == [12, 13, 14]
    assert drawn == [n * (n - 1) // 2 + n * b for b in range(3)]


def test_an_exception_in_mid_loop_closes_counter_then_arena(monkeypatch):
    from covest_amd import jackknife
    from covest_amd.read_bootstrap import bootstrap_histograms
    rec = Recorder(monkeypatch, fail_clear=2)
    with pytest.raises(RuntimeError, match="clear failed"):
        jackknife.leave_group_out_histograms(fixed_reads(), K, 3, seed=SEED)
    assert rec.log[-3:] == [("clear", None), ("counts.close",), ("arena.close",)]
    assert [c[0] for c in rec.log].count("clear") == 2 and [c[0] for c in rec.log].count("histogram") == 2
    rec = Recorder(monkeypatch, fail_clear=2)
    with pytest.raises(RuntimeError, match="clear failed"):
        bootstrap_histograms(ragged_reads(), K, 3, seed=SEED)
    assert rec.log[-4:] == [("weights", W, 5, 1, SEED, 0, None, -1), ("clear", None), ("counts.close",), ("arena.close",)]
    assert [c[0] for c in rec.log].count("histogram") == 2


def test_another_current_device_and_reads_that_do_not_fit(monkeypatch):
    from covest_amd import _capi, jackknife
    from covest_amd.read_bootstrap import bootstrap_histograms
    calls = {"leave_group_out_histograms": lambda: jackknife.leave_group_out_histograms(fixed_reads(), K, 3, device=0),
             "bootstrap_histograms": lambda: bootstrap_histograms(fixed_reads(), K, 3, device=0)}
    for who, call in calls.items():
        rec = Recorder(monkeypatch, current=1)
        with pytest.raises(_capi.CovestHipError) as e:
            call()
        assert str(e.value) == "%s: the reads are staged on the calling thread's current device (1), not device 0" % who
        assert rec.log == [("arena", who), ("hipGetDevice",), ("arena.close",)]
    # the buffer behind the reads has no room: each function says what it had asked for beside them
    texts = {"leave_group_out_histograms": ("out", "their copy in group order"),
             "bootstrap_histograms": ("weights", "a weight a read")}
    for who, call in calls.items():
        rec = Recorder(monkeypatch, no_room=texts[who][0])
        with pytest.raises(_capi.CovestHipError) as e:
            call()
        assert str(e.value) == ("%s: 72 bases of reads do not fit the device together with %s "
                                "(stand-in: hipMalloc failed (HIP error 2))" % (who, texts[who][1]))
        assert rec.log[-2:] == [("reserve", texts[who][0], {"out": 72, "weights": 24}[texts[who][0]]), ("arena.close",)]


# ---- the shared refit ------------------------------------------------------------------------------------------------------
B = 3
REFITTED = np.array([[10.0, 0.02], [9.0, 0.5], [12.0, 0.03], [11.0, 0.5]])   # row B: the full set's, on a bound as row 1
SUCCESS = np.array([True, False, True, True])
SHARED = ("estimates", "success", "at_bound", "occurrences", "occurrences_full", "full_estimate", "full_success",
          "full_minus_given", "keys_added", "params", "estimate", "level", "seed", "refit")


class RefitModel:
    params, k, device, sample_factor = ("coverage", "error_rate"), K, -1, 1
    bounds = ((0.0, None), (0.0, 0.5))

    @staticmethod
    def correct_c(c):
        return 0.8 * c


def stub_refit(monkeypatch, log, fail=False):
    class Closing:
        def __init__(self, name):
            self.name = name

        def close(self):
            log.append((self.name + ".close",))

    def batch_of(model, hists, hist_full, trim=None):
        log.append(("jackknife_batch", model, list(hists), hist_full, trim))
        return Closing("twin"), Closing("batch"), 4

    def refit(model, estimate, replicates, seed, n_draws, fix, estimator_options, analytic=False, batch=None):
        log.append(("_refit_lockstep", model.name, list(estimate), replicates, seed, n_draws, fix, dict(estimator_options),
                    analytic, batch.name))
        if fail:
            raise RuntimeError("stand-in: the refit failed")
        return REFITTED.copy(), SUCCESS.copy(), None

    put(monkeypatch, "jackknife_batch", batch_of)
    put(monkeypatch, "_refit_lockstep", refit)


def test_read_jackknife_and_read_bootstrap_share_their_refit(monkeypatch):
    from covest_amd.jackknife import read_jackknife
    from covest_amd.read_bootstrap import read_bootstrap
    model, given, fix = RefitModel(), [10.5, 0.025], [None, None]
    outs = {}
    for name, call in (("jackknife", lambda **kw: read_jackknife(model, given, fixed_reads(), groups=B, **kw)),
                       ("bootstrap", lambda **kw: read_bootstrap(model, given, fixed_reads(), replicates=B, **kw))):
        rec = Recorder(monkeypatch)
        stub_refit(monkeypatch, rec.log)
        out = outs[name] = call(seed=SEED, fix=fix, level=0.9, trim=7, refit="lockstep", maxiter=3)
        at = [c[0] for c in rec.log].index("jackknife_batch")
        assert rec.log[at - 1] == ("arena.close",)                       # the reads have left the device before the refit
        assert rec.log[at:] == [
            ("jackknife_batch", model, [hist(2), hist(3), hist(4)], hist(1), 7),
            ("_refit_lockstep", "twin", given, B + 1, SEED, 0, fix, {"maxiter": 3}, False, "batch"),
            ("batch.close",), ("twin.close",)]
        # row B is the full set's refit; the rows before it are the groups' or the replicates'
        assert out["estimates"].tolist() == REFITTED[:B].tolist() and out["success"].tolist() == [True, False, True]
        assert out["at_bound"].dtype == bool and out["at_bound"].tolist() == [[False, False], [False, True], [False, False]]
        assert out["full_estimate"] == [11.0, 0.5] and out["full_success"] is True
        assert out["full_minus_given"] == [11.0 - 10.5, 0.5 - 0.025]
        assert out["occurrences"] == [12, 13, 14] and out["occurrences_full"] == 11 and out["keys_added"] == 4
        assert out["params"] == ["coverage", "error_rate"] and out["estimate"] == given
        assert (out["level"], out["seed"], out["refit"]) == (0.9, SEED, "lockstep")
        assert out["used"] == 2 and out["failed"] == 1
    for key in SHARED:
        a, b = outs["jackknife"][key], outs["bootstrap"][key]
        assert (a.tobytes() == b.tobytes() and a.dtype == b.dtype) if isinstance(a, np.ndarray) else a == b, key
    assert outs["jackknife"]["groups"] == B and outs["jackknife"]["group_sizes"] == [2, 0, 4]
    assert outs["bootstrap"]["replicates"] == B and outs["bootstrap"]["reads_drawn"] == [15, 21, 27]
    assert set(outs["jackknife"]) == set(SHARED) | {"groups", "group_sizes", "mean", "standard_errors", "bias",
                                                    "bias_corrected", "intervals", "failed", "used"}
    assert set(outs["bootstrap"]) == set(SHARED) | {"replicates", "reads_drawn", "mean", "standard_errors", "bias",
                                                    "intervals", "bound_share", "failed", "used"}
    # the default route is the analytic one; a refit that raises still closes the batch, then the twin
    for call in (lambda: read_jackknife(model, given, fixed_reads(), groups=B),
                 lambda: read_bootstrap(model, given, fixed_reads(), replicates=B)):
        rec = Recorder(monkeypatch)
        stub_refit(monkeypatch, rec.log, fail=True)
        with pytest.raises(RuntimeError, match="the refit failed"):
            call()
        assert rec.log[-3:] == [("_refit_lockstep", "twin", given, B + 1, 0, 0, None, {}, True, "batch"),
                                ("batch.close",), ("twin.close",)]


# ---- the record ------------------------------------------------------------------------------------------------------------
class RecordModel:
    params = ("coverage", "error_rate", "q1")
    hist = {1: 10, 2: 5, 7: 1}

    @staticmethod
    def short_name():
        return "stand-in"


def test_print_output_writes_the_same_record_for_jackknife_and_read_bootstrap():
    """Both dicts have a fixed parameter (q1: None everywhere).  The expected records are written out from a run before
    the two blocks of print_output were made one."""
    from covest_amd import __version__, print_output
    jack = {"groups": 8, "used": 7, "failed": 1, "level": 0.9,
            "standard_errors": {"coverage": 0.25, "error_rate": 0.001, "q1": None, "genome_size": 120.5},
            "bias": {"coverage": -0.5, "error_rate": 0.0, "q1": None, "genome_size": 33},
            "intervals": {"coverage": [9.5, 10.5], "error_rate": (0.018, 0.022), "q1": None, "genome_size": [4800, 5200.5]},
            "mean": {"coverage": 10.0}, "bias_corrected": {"coverage": 10.5}}
    boot = {"replicates": 16, "used": 16, "failed": 0, "level": 0.95,
            "standard_errors": {"coverage": 0.5, "error_rate": 0.002, "q1": None, "genome_size": 250.0},
            "bias": {"coverage": -2.75, "error_rate": 0.004, "q1": None, "genome_size": 1400.0},
            "intervals": {"coverage": [7.0, 7.5], "error_rate": [0.02, 0.03], "q1": None, "genome_size": [6000.0, 6500.0]},
            "bound_share": {"coverage": 0.0}}
    head = [("model", "stand-in"), ("hist_size", 7), ("sample_factor", 1), ("orig_sample_factor", 1), ("success", True),
            ("version", __version__), ("starting_points", 1), ("use_grid_search", False)]
    want_jack = [
        ("jackknife_groups", 8), ("jackknife_used", 7), ("jackknife_failed", 1), ("jackknife_level", 0.9),
        ("jackknife_se_coverage", 0.25), ("jackknife_bias_coverage", -0.5), ("jackknife_interval_coverage", [9.5, 10.5]),
        ("jackknife_se_error_rate", 0.001), ("jackknife_bias_error_rate", 0.0), ("jackknife_interval_error_rate", [0.018, 0.022]),
        ("jackknife_se_genome_size", 120.5), ("jackknife_bias_genome_size", 33.0),
        ("jackknife_interval_genome_size", [4800.0, 5200.5])]
    want_boot = [
        ("read_bootstrap_replicates", 16), ("read_bootstrap_used", 16), ("read_bootstrap_failed", 0),
        ("read_bootstrap_level", 0.95),
        ("read_bootstrap_se_coverage", 0.5), ("read_bootstrap_bias_coverage", -2.75),
        ("read_bootstrap_interval_coverage", [7.0, 7.5]),
        ("read_bootstrap_se_error_rate", 0.002), ("read_bootstrap_bias_error_rate", 0.004),
        ("read_bootstrap_interval_error_rate", [0.02, 0.03]),
        ("read_bootstrap_se_genome_size", 250.0), ("read_bootstrap_bias_genome_size", 1400.0),
        ("read_bootstrap_interval_genome_size", [6000.0, 6500.0])]
    record = print_output(None, RecordModel(), True, 1, silent=True, jackknife=jack, read_bootstrap=boot)
    assert list(record.items()) == head + want_jack + want_boot
    for key, value in want_jack + want_boot:                              # 33 and 4800 went in as integers
        assert type(record[key]) is type(value), key
        if isinstance(value, list):
            assert all(type(v) is float for v in record[key]), key
    assert list(print_output(None, RecordModel(), True, 1, silent=True, jackknife=jack).items()) == head + want_jack
    assert list(print_output(None, RecordModel(), True, 1, silent=True, read_bootstrap=boot).items()) == head + want_boot
