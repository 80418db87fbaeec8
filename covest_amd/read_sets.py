"""What the statistics over resampled READS share (jackknife.py, read_bootstrap.py; DESIGN.md sections 6aa, 6ak): one read
set staged on the device with one reserved counter (ResidentReads), the rules of a refit request (check_refit_request),
the refit of B + 1 histograms on one key set (jackknife_batch, refit_histogram_set) and the table of quantities a summary
is taken over (quantity_rows).  A resampling scheme adds its own loop and its own statistics.  There is no CPU path."""
import ctypes

import numpy as np

from . import _capi

REFITS = ("lockstep", "lockstep-gradient")


def _hist_dict(counts):
    """KmerCounts.histogram()'s list as {abundance: k-mers}, the abundances that occur."""
    return {i: int(v) for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}


def _occurrences(hist):
    return int(sum(i * n for i, n in hist.items()))


def check_sets(noun, value, scheme, most, most_text):
    """How many sets a `scheme` resamples (`noun`: its groups, its replicates), as an int: an integer in 2 .. `most`."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s must be an integer" % noun)
    if value < 2:
        raise ValueError("a %s needs at least two %s" % (scheme, noun))
    if value > most:
        raise ValueError("%s must be within 2 .. %s" % (noun, most_text))
    return int(value)


class ResidentReads:
    """`reads` -- a SimulatedReads, an (n, L) uint8 array or a pair (bases, offsets) in the packed layout -- uploaded once
    (`d_in`, and `d_offsets` for reads of their own lengths, else None), and ONE KmerCounts whose table is reserved once
    for the k-mers of the whole set.  `n`, `read_len` (0 with offsets), `n_bases`, `first_read` (a SimulatedReads' own,
    else 0) describe the set.  The buffers live on the calling thread's current device, which `device` has to name (or
    -1).  `who` names the caller in the errors and `beside` says what it reserves beside the reads, for the one that
    tells that they do not fit.  Leaving the block closes the counter, then the arena."""

    def __init__(self, reads, k, canonical, device, who, beside):
        from .sample import _packed
        if int(k) != k or k < 1:
            raise ValueError("k must be a positive integer")
        self.blob, self.offsets, self.n, self.read_len, source = _packed(reads)
        self.first_read = int(source.first_read) if source is not None else 0
        self.n_bases = int(self.offsets[-1]) if self.offsets is not None else self.n * self.read_len
        self.k, self.canonical, self.device, self.who, self.beside = int(k), canonical, device, who, beside
        self.arena = self.counts = None

    def __enter__(self):
        from .sample import _DeviceArena
        try:
            self.arena = _DeviceArena(self.who)
            if self.device >= 0:
                current = ctypes.c_int(-1)
                self.arena.hip.hipGetDevice(ctypes.byref(current))
                if current.value != int(self.device):
                    raise _capi.CovestHipError("%s: the reads are staged on the calling thread's current device (%d), not "
                                               "device %d" % (self.who, current.value, self.device))
            self.d_in = self.reserve("in", self.n_bases, self.blob)
            self.d_offsets = self.reserve("offsets", 8 * (self.n + 1), self.offsets) if self.offsets is not None else None
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        if self.counts is not None:
            self.counts.close()
        if self.arena is not None:
            self.arena.close()

    def reserve(self, name, n_bytes, host=None):
        """A buffer of the arena beside the reads, filled from the array `host` where one is given: its device pointer."""
        try:
            if host is None:
                return self.arena.reserve(name, n_bytes)
            return self.arena.upload(name, host.ctypes.data, n_bytes)
        except _capi.CovestHipError as e:
            raise _capi.CovestHipError("%s: %d bases of reads do not fit the device together with %s (%s)"
                                       % (self.who, self.n_bases, self.beside, e))

    def download(self, name, array):
        self.arena.download(name, array)  # (the null stream: waits for what was launched)

    def open_counter(self):
        """The counter, its table reserved for the k-mers the whole set can add: sum(max(len - k + 1, 1)), bounded as
        add_packed bounds it.  Called once, behind what the caller reserves and launches before it counts."""
        from .kmer_hist import KmerCounts
        self.counts = KmerCounts(self.k, canonical=self.canonical, device=self.device)
        self.counts._reserve_for(self.n_bases + self.n if self.offsets is not None
                                 else self.n * max(self.read_len - self.k + 1, 1))

    def count(self, d_bases, d_offsets, lo, hi, d_weights=None):
        """Add the reads at ranks [lo, hi) of (`d_bases`, `d_offsets`) -- the input, or a copy of it in another order --
        to the counter, read r `d_weights`[r] times where weights are given.  A sub-range addresses the same buffer:
        offsets + lo for reads of their own lengths, bases + lo * read_len for reads of one length."""
        ragged = self.offsets is not None
        where = (d_bases, hi - lo, 0) if ragged else (d_bases + lo * self.read_len, hi - lo, self.read_len)
        d_offsets = d_offsets + 8 * lo if ragged else None
        if d_weights is None:
            self.counts.add_device(*where, d_offsets_ptr=d_offsets, reserve=False)
        else:
            self.counts.add_weighted_device(*where, d_weights + 4 * lo, d_offsets_ptr=d_offsets, reserve=False)

    def uncount(self, d_bases, d_offsets, lo, hi):
        """Take the reads at ranks [lo, hi) of (`d_bases`, `d_offsets`) out of the counter again (k <= 31): count's
        inverse on the same sub-range.  The keys stay in their slots with a count of 0 where nothing else supports them,
        so the table reserved by open_counter stays large enough for counting them back in."""
        ragged = self.offsets is not None
        where = (d_bases, hi - lo, 0) if ragged else (d_bases + lo * self.read_len, hi - lo, self.read_len)
        self.counts.remove_device(*where, d_offsets_ptr=d_offsets + 8 * lo if ragged else None)

    def clear(self):
        self.counts.clear()

    def histogram(self):
        """{abundance: k-mers} of what was counted since the last clear (waits for the counter)."""
        return _hist_dict(self.counts)


def check_refit_request(who, model, estimate, refit=None, estimator_options=None, level=0.95, fix=None, trim=None,
                        sample_factor=None, refits=None):
    """The argument rules of a refit from `estimate`, before the library is asked (ValueError): (estimate as floats, the
    parameter names).  One estimate per parameter; with `refits`, `refit` one of them and the estimator's `gradient`
    option the one that goes with it; `level` in (0, 1); with `sample_factor` (None: no such rule) it and the model's
    both 1; `fix` None or one entry per parameter; `trim` None or a positive integer."""
    estimate = [float(v) for v in estimate]
    names = list(model.params)
    if len(estimate) != len(names):
        raise ValueError("%s: %d parameters expected, %d given" % (who, len(names), len(estimate)))
    if refits is not None:
        if refit not in refits:
            raise ValueError("refit must be %s or \"%s\"" % (", ".join('"%s"' % r for r in refits[:-1]), refits[-1]))
        if refit == "lockstep" and estimator_options.get('gradient', 'fd') != 'fd':
            raise ValueError('refit="lockstep" goes with gradient="fd" only: the analytic gradient is refit="lockstep-gradient"')
        if refit == "lockstep-gradient" and estimator_options.get('gradient', 'analytic') != 'analytic':
            raise ValueError('refit="lockstep-gradient" goes with gradient="analytic" only: finite differences are '
                             'refit="lockstep"')
    try:
        inside = 0.0 < level < 1.0
    except TypeError:  # (no number)
        inside = False
    if not inside:
        raise ValueError("level must be in (0, 1)")
    if sample_factor is not None and (sample_factor != 1 or getattr(model, 'sample_factor', 1) != 1):
        raise ValueError("%s needs a model built with sample factor 1: a down-sampled histogram is rounded at random and "
                         "is not a function of the reads" % who)
    if fix is not None and len(fix) != len(names):
        raise ValueError("%s: fix needs one entry per parameter" % who)
    if trim is not None and (int(trim) != trim or trim < 1):
        raise ValueError("trim must be a positive integer")
    return estimate, names


def _cut(hist, trim):
    """(kept, tail) of one histogram under the model's cut (hist_steps.trim_hist); trim None: no cut."""
    if trim is None or not hist:
        return dict(hist), 0
    from .hist_steps import trim_hist
    return trim_hist(hist, trim)


def jackknife_batch(model, hists, hist_full, trim=None):
    """(twin, batch, keys_added): the leave-out histograms (rows 0 .. G - 1) and the full one (row G) as ONE
    HistogramBatch on a twin of `model` whose key set is the model's keys and behind them, ascending, the keys any of
    the histograms keeps beyond those, zero counts kept.  Each histogram is cut as read_jackknife states.  Both are the
    caller's to close (batch first)."""
    from .batch import HistogramBatch
    from .bootstrap import _replicate_model
    if trim is None and model.tail != 0:
        trim = max(model.hist) + 1
    cut = [_cut(h, trim) for h in list(hists) + [hist_full]]
    own = list(model.hist.keys())
    added = sorted(set().union(*(kept.keys() for kept, _ in cut)) - set(own))
    keys = own + added
    counts = np.array([[kept.get(j, 0) for j in keys] for kept, _ in cut], dtype=np.float64)
    tails = np.array([tail for _, tail in cut], dtype=np.float64)
    twin = _replicate_model(model, keys, counts[-1], float(tails[-1]))
    try:
        return twin, HistogramBatch(twin, counts, tails), len(added)
    except Exception:
        twin.close()
        raise


def refit_histogram_set(model, estimate, hists, hist_full, seed, fix, level, trim, refit, estimator_options):
    """The B histograms `hists` and `hist_full` refitted together from `estimate` (floats): jackknife_batch puts them on
    one key set, bootstrap._refit_lockstep refits the B + 1 rows, `refit` as in parametric_bootstrap.  Returns what
    read_jackknife and read_bootstrap both return: seed, refit, level, params, estimate, estimates (B x P, rows 0 .. B - 1),
    success (B), at_bound (B x P), occurrences (B), occurrences_full, full_estimate (row B's refit), full_success,
    full_minus_given, keys_added."""
    from .bootstrap import _on_bound, _refit_lockstep
    B = len(hists)
    twin, batch, added = jackknife_batch(model, hists, hist_full, trim)
    try:
        estimates, success, _ = _refit_lockstep(twin, estimate, B + 1, seed, 0, fix, estimator_options,
                                                analytic=refit == "lockstep-gradient", batch=batch)
    finally:
        batch.close()
        twin.close()
    full = [float(v) for v in estimates[B]]
    return {'seed': int(seed), 'refit': refit, 'level': float(level), 'params': list(model.params), 'estimate': estimate,
            'estimates': estimates[:B].copy(), 'success': success[:B].copy(),
            'at_bound': np.array([_on_bound(row, model.bounds) for row in estimates[:B]], dtype=bool),
            'occurrences': [_occurrences(h) for h in hists], 'occurrences_full': _occurrences(hist_full),
            'full_estimate': full, 'full_success': bool(success[B]),
            'full_minus_given': [a - b for a, b in zip(full, estimate)], 'keys_added': added}


def quantity_rows(who, estimates, success, full, occurrences, occurrences_full, names, fix, level, correct_c, noun):
    """(used, mask, rows) of the quantities summarize_jackknife and summarize_read_bootstrap state, their arguments: `mask`
    is `success` as booleans, `used` = B' their number, and a row is (name, the B' values over the successful refits,
    the value on the full set, free, the parameter it goes with) -- every parameter, the coverage rescaled to the full
    read set, and behind them 'genome_size', which goes with the coverage.  `noun` is what one of the B sets is in
    `who`'s ValueError; `level` has to lie in (0, 1)."""
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    names = list(names)
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, len(names))
    ok = np.asarray(success, dtype=bool).reshape(-1)
    occ = np.asarray(occurrences, dtype=np.float64).reshape(-1)
    full = np.asarray(full, dtype=np.float64).reshape(-1)
    if not (len(est) == len(ok) == len(occ)) or len(full) != len(names):
        raise ValueError("%s: one estimate, success flag and occurrence count per %s" % (who, noun))
    fix = [None] * len(names) if fix is None else list(fix)
    good, good_occ = est[ok], occ[ok]
    rows = []
    for d, name in enumerate(names):
        values = good[:, d] * (float(occurrences_full) / good_occ) if d == 0 else good[:, d]
        rows.append((name, values, float(full[d]), fix[d] is None, d))
    rows.append(('genome_size', np.array([o / correct_c(c) for o, c in zip(good_occ, good[:, 0])], dtype=np.float64),
                 float(occurrences_full) / correct_c(float(full[0])), fix[0] is None, 0))
    return int(ok.sum()), ok, rows
