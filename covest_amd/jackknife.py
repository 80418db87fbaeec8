"""The delete-a-group jackknife over READS: standard errors that see what no function of the
histogram can -- that the k-mers of one read come and go together.

    est, ok = CoverageEstimator(model).compute_coverage(guess)
    jack = read_jackknife(model, est, reads, groups=32, seed=1)
    print_output(hist_orig, model, ok, 1, estimated=est, jackknife=jack)

The reads are dealt into G seeded groups (covest_split_reads: the group of read r is a stated function of (seed, r)),
leave-out histogram g is the k-mer histogram of every read OUTSIDE group g, the G histograms and the full one are
refitted together on one HistogramBatch, and the spread of the G refits is the variance.  Whole reads are deleted, never
single k-mers: that is what lets the number speak about the dependence between overlapping k-mers.

The only device work that is new is the split (split_reads.hip): after it every group is one contiguous run of the
packed reads, and "all reads but group g" is two covest_kmer_add_device calls on sub-ranges of one buffer.  There is no
CPU path: without the library or a HIP device the calls raise CovestHipError.
"""
import math

import numpy as np

from . import _capi
from .sample import MAX_GROUPS, _DeviceArena, _check_split, _packed, split_reads_device

REFITS = ("lockstep", "lockstep-gradient")


def _hist_dict(counts):
    """KmerCounts.histogram()'s list as {abundance: k-mers}, the abundances that occur."""
    return {i: int(v) for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}


def _occurrences(hist):
    return int(sum(i * n for i, n in hist.items()))


def _check_groups(groups):
    if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)):
        raise ValueError("groups must be an integer")
    if groups < 2:
        raise ValueError("a jackknife needs at least two groups")
    if groups > MAX_GROUPS:
        raise ValueError("groups must be within 2 .. %d" % MAX_GROUPS)
    return int(groups)


def leave_group_out_histograms(reads, k, groups, seed=0, canonical=False, device=-1):
    """(hist_full, [hist_g for g in range(groups)], occurrences) of `reads` -- a SimulatedReads, an (n, L) uint8 array
    or a pair (bases, offsets) in the packed layout --: hist_g the k-mer histogram {abundance: k-mers} of the reads
    outside group g of covest_split_reads(groups, seed), hist_full that of all reads, occurrences[g] = sum i hist_g[i].

    The reads go up once and are split once on the device; each histogram comes from ONE KmerCounts whose table is
    reserved once for the whole set: clear, add_device on the ranks before the group, add_device on the ranks behind it,
    histogram.  The sub-ranges address the same buffer (ragged reads: offsets + first; reads of one length: bases + first
    * read_len).  The buffers live on the calling thread's current device, which `device` has to name (or -1).  Reads
    that do not fit the device together with their copy raise CovestHipError; streaming a file in passes is not built."""
    return _leave_group_out(reads, k, groups, seed, canonical, device)[:3]


def _leave_group_out(reads, k, groups, seed, canonical, device):
    """leave_group_out_histograms, and the split's group_first behind its three results."""
    groups = _check_groups(groups)
    groups, seed, _ = _check_split(groups, seed, 0)
    if int(k) != k or k < 1:
        raise ValueError("k must be a positive integer")
    blob, offsets, n, read_len, source = _packed(reads)
    first_read = int(source.first_read) if source is not None else 0
    from .kmer_hist import KmerCounts
    n_bases = int(offsets[-1]) if offsets is not None else n * read_len
    arena = counts = None
    try:
        arena = _DeviceArena("leave_group_out_histograms")
        if device >= 0:
            import ctypes
            current = ctypes.c_int(-1)
            arena.hip.hipGetDevice(ctypes.byref(current))
            if current.value != int(device):
                raise _capi.CovestHipError("leave_group_out_histograms: the reads are staged on the calling thread's current "
                                           "device (%d), not device %d" % (current.value, device))
        try:
            d_in = arena.upload("in", blob.ctypes.data, n_bases)
            d_off = arena.upload("offsets", offsets.ctypes.data, 8 * (n + 1)) if offsets is not None else None
            d_out = arena.reserve("out", n_bases)
            d_out_off = arena.reserve("out_offsets", 8 * (n + 1)) if offsets is not None else None
            d_first = arena.reserve("group_first", 8 * (groups + 1))
        except _capi.CovestHipError as e:
            raise _capi.CovestHipError("leave_group_out_histograms: %d bases of reads do not fit the device together with "
                                       "their copy in group order (%s)" % (n_bases, e))
        split_reads_device(d_in, n, d_out, d_first, groups, seed=seed, first_read=first_read, read_len=read_len,
                           offsets_ptr=d_off, out_offsets_ptr=d_out_off, device=device)
        first = np.empty(groups + 1, dtype=np.int64)
        arena.download("group_first", first)  # (the null stream: waits for the split)

        counts = KmerCounts(k, canonical=canonical, device=device)
        # k-mers the whole set can add: sum(max(len - k + 1, 1)), bounded as add_packed bounds it
        counts._reserve_for(n_bases + n if offsets is not None else n * max(read_len - int(k) + 1, 1))

        def add(lo, hi):  # ranks [lo, hi) of the split buffer
            if hi <= lo:
                return
            if offsets is not None:
                counts.add_device(d_out, hi - lo, 0, d_offsets_ptr=d_out_off + 8 * lo, reserve=False)
            else:
                counts.add_device(d_out + lo * read_len, hi - lo, read_len, reserve=False)

        add(0, n)
        hist_full = _hist_dict(counts)  # (waits for the counter)
        hists = []
        for g in range(groups):
            counts.clear()
            add(0, int(first[g]))
            add(int(first[g + 1]), n)
            hists.append(_hist_dict(counts))
        return hist_full, hists, [_occurrences(h) for h in hists], first
    finally:
        if counts is not None:
            counts.close()
        if arena is not None:
            arena.close()


def summarize_jackknife(estimates, success, full, occurrences, occurrences_full, names, fix, level, correct_c):
    """The delete-a-group jackknife's arithmetic on arrays (pure numpy): `estimates` (G, P) the leave-out refits, `success`
    (G,), `full` (P,) the refit of the full set, `occurrences` (G,) and `occurrences_full` the k-mer occurrences sum i h_i
    of each set, `names` the P parameter names (the coverage first), `fix` None or P entries (None: free), `correct_c` the
    model's map from coverage to k-mer coverage.

    The quantities: every parameter but the first as it is (error rate, q1, q2, q are scale-free); the coverage of
    leave-out set g rescaled to the full read set, c_g * occurrences_full / occurrences[g] -- deleting a group lowers the
    coverage by construction, what is uncertain is the genome size --; and 'genome_size' = occurrences[g] /
    correct_c(c_g), report.py's formula on the leave-out set (occurrences_full / correct_c(c_full) for the full one).
    Over the G' successful leave-out refits, per quantity theta: mean; standard_errors = sqrt((G' - 1) / G' * sum (theta_g
    - mean)^2); bias = (G' - 1) (mean - theta_full); bias_corrected = theta_full - bias; intervals = theta_full -+
    t_{G' - 1, (1 + level) / 2} * standard error.  None for a fixed parameter (the genome size goes with the coverage),
    and for everything where G' < 2.  Also `failed` = G - G' and `used` = G'."""
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    names = list(names)
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, len(names))
    ok = np.asarray(success, dtype=bool).reshape(-1)
    occ = np.asarray(occurrences, dtype=np.float64).reshape(-1)
    full = np.asarray(full, dtype=np.float64).reshape(-1)
    if not (len(est) == len(ok) == len(occ)) or len(full) != len(names):
        raise ValueError("summarize_jackknife: one estimate, success flag and occurrence count per group")
    fix = [None] * len(names) if fix is None else list(fix)
    used = int(ok.sum())
    good, good_occ = est[ok], occ[ok]
    # (quantity, its G' leave-out values, its value on the full set, free)
    rows = []
    for d, name in enumerate(names):
        values = good[:, d] * (float(occurrences_full) / good_occ) if d == 0 else good[:, d]
        rows.append((name, values, float(full[d]), fix[d] is None))
    rows.append(('genome_size', np.array([o / correct_c(c) for o, c in zip(good_occ, good[:, 0])], dtype=np.float64),
                 float(occurrences_full) / correct_c(float(full[0])), fix[0] is None))
    out = {'mean': {}, 'standard_errors': {}, 'bias': {}, 'bias_corrected': {}, 'intervals': {},
           'failed': int(len(ok) - used), 'used': used}
    quantile = None
    if used >= 2:
        from scipy.stats import t as student_t
        quantile = float(student_t.ppf(0.5 * (1.0 + level), used - 1))
    for name, values, theta_full, free in rows:
        if not free or used < 2:
            for key in ('mean', 'standard_errors', 'bias', 'bias_corrected', 'intervals'):
                out[key][name] = None
            continue
        mean = float(values.mean())
        se = math.sqrt((used - 1) / used * float(((values - mean) ** 2).sum()))
        bias = (used - 1) * (mean - theta_full)
        out['mean'][name] = mean
        out['standard_errors'][name] = se
        out['bias'][name] = bias
        out['bias_corrected'][name] = theta_full - bias
        out['intervals'][name] = [theta_full - quantile * se, theta_full + quantile * se]
    return out


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


def read_jackknife(model, estimate, reads, groups=32, seed=0, fix=None, level=0.95, trim=None, refit="lockstep-gradient",
                   sample_factor=1, canonical=False, **estimator_options):
    """The delete-a-group jackknife of `estimate` (of `model`, whose histogram is that of `reads` at k = model.k,
    `canonical` as it was counted) over `groups` seeded groups of the reads.

    WHAT THE NUMBER IS.  Its standard errors see the dependence between the k-mers of one read -- a read is deleted
    whole -- and the randomness of where the reads start.  The genome is held fixed: nothing here speaks about another
    genome of the same kind.  The groups' sizes are binomial (a read's group is drawn on its own), not equal; the
    formulas are the equal-size ones, which is the usual approximation at n / G reads a group.  The intervals are
    Student t with G' - 1 degrees of freedom, G' the leave-out refits that succeeded: G, not the number of reads,
    limits how well the variance itself is known.

    HOW.  leave_group_out_histograms gives the G + 1 histograms.  Each is cut as the model's was: keys below `trim` are
    kept and the mass at and above goes to the tail (hist_steps.trim_hist); trim=None with model.tail == 0 means no cut,
    trim=None with a tail takes max(model.hist) + 1.  The G + 1 histograms are put on ONE key set -- the model's keys and
    behind them, ascending, the keys any of the histograms has beyond those; zero counts kept -- on a twin of the model
    (bootstrap._replicate_model: class, settings, bounds, defaults): tail * log(1 - sum p_j) sums over the keys, so all
    fits must share the cells.  Rows 0 .. G - 1 of one HistogramBatch are the leave-out histograms, row G the full one;
    all are refitted together from `estimate` by bootstrap._refit_lockstep, `refit` as in parametric_bootstrap
    ("lockstep": finite differences; "lockstep-gradient": the batch's analytic gradient).

    sample_factor other than 1 raises ValueError: sample_histogram rounds at random, so a jackknife through it would not
    be a function of the reads.

    Returns summarize_jackknife's dict (mean, standard_errors, bias, bias_corrected, intervals per parameter name and
    'genome_size'; failed, used) and: estimates (G x P, as refitted: the coverage not rescaled), success (G), at_bound
    (G x P), group_sizes (reads a group), occurrences (G), occurrences_full, full_estimate (row G's refit),
    full_success, full_minus_given (its distance from `estimate`), keys_added (keys of the union the model did not
    have), params, estimate, level, groups, seed, refit."""
    groups = _check_groups(groups)
    _check_split(groups, seed, 0)
    estimate = [float(v) for v in estimate]
    names = list(model.params)
    if len(estimate) != len(names):
        raise ValueError("read_jackknife: %d parameters expected, %d given" % (len(names), len(estimate)))
    if refit not in REFITS:
        raise ValueError('refit must be "lockstep" or "lockstep-gradient"')
    if refit == "lockstep" and estimator_options.get('gradient', 'fd') != 'fd':
        raise ValueError('refit="lockstep" goes with gradient="fd" only: the analytic gradient is refit="lockstep-gradient"')
    if refit == "lockstep-gradient" and estimator_options.get('gradient', 'analytic') != 'analytic':
        raise ValueError('refit="lockstep-gradient" goes with gradient="analytic" only: finite differences are refit="lockstep"')
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    if sample_factor != 1 or getattr(model, 'sample_factor', 1) != 1:
        raise ValueError("read_jackknife needs a model built with sample factor 1: a down-sampled histogram is rounded at "
                         "random and is not a function of the reads")
    if fix is not None and len(fix) != len(names):
        raise ValueError("read_jackknife: fix needs one entry per parameter")
    if trim is not None and (int(trim) != trim or trim < 1):
        raise ValueError("trim must be a positive integer")
    from .bootstrap import _on_bound, _refit_lockstep

    hist_full, hists, occurrences, group_first = _leave_group_out(reads, model.k, groups, seed, canonical, model.device)
    occurrences_full = _occurrences(hist_full)
    twin, batch, added = jackknife_batch(model, hists, hist_full, trim)
    try:
        estimates, success, _ = _refit_lockstep(twin, estimate, groups + 1, seed, 0, fix, estimator_options,
                                                analytic=refit == "lockstep-gradient", batch=batch)
    finally:
        batch.close()
        twin.close()
    full = [float(v) for v in estimates[groups]]
    out = {'groups': groups, 'seed': int(seed), 'refit': refit, 'level': float(level), 'params': names, 'estimate': estimate,
           'estimates': estimates[:groups].copy(), 'success': success[:groups].copy(),
           'at_bound': np.array([_on_bound(row, model.bounds) for row in estimates[:groups]], dtype=bool),
           'occurrences': list(occurrences), 'occurrences_full': occurrences_full,
           'full_estimate': full, 'full_success': bool(success[groups]),
           'full_minus_given': [a - b for a, b in zip(full, estimate)], 'keys_added': added,
           'group_sizes': np.diff(group_first).tolist()}
    out.update(summarize_jackknife(out['estimates'], out['success'], full, occurrences, occurrences_full, names, fix, level,
                                   model.correct_c))
    return out
