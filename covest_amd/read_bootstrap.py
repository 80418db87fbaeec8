"""The bootstrap over READS: whole reads resampled with replacement, the k-mers of a read coming
and going together, and percentile intervals that assume no normality.

    est, ok = CoverageEstimator(model).compute_coverage(guess)
    boot = read_bootstrap(model, est, reads, replicates=64, seed=1)
    print_output(hist_orig, model, ok, 1, estimated=est, read_bootstrap=boot)

It is the POISSON bootstrap: in replicate b read r is drawn m(r, b) ~ Poisson(1) times, a stated function of (seed, b,
r) (covest_bootstrap_weights: Philox stream 9 and thirteen thresholds, include/covest_amd.h), so a replicate holds n reads
on average, with relative spread 1 / sqrt(n), not exactly n.  The replicate's k-mer histogram is the histogram of the
reads counted with those weights (covest_kmer_add_weighted_device): the reads are neither copied nor moved.  The B
histograms and the full one are refitted together on one HistogramBatch, as the delete-a-group jackknife's are
(jackknife.py), and the coverage of a replicate is rescaled to the full read set, which takes the replicate's size out.
There is no CPU path: without the library or a HIP device the calls raise CovestHipError.

Measured: the replicates are exact and cheap, and the refits on them are biased by the duplicated
reads -- read_bootstrap's docstring says what that means for its intervals.
"""
import ctypes

import numpy as np

from . import _capi
from .jackknife import REFITS, _hist_dict, _occurrences, jackknife_batch
from .sample import _DeviceArena, _packed
from .simulate import _check_seed

def _check_weights_args(n_reads, replicate, seed, first_read):
    """The argument rules of covest_bootstrap_weights, before the library is asked (ValueError)."""
    if int(n_reads) != n_reads or n_reads < 0:
        raise ValueError("n_reads must not be negative")
    if isinstance(replicate, bool) or int(replicate) != replicate or not 0 <= replicate < 1 << 32:
        raise ValueError("replicate must fit 32 bits, not negative")
    _check_seed(seed, whole=True)
    if int(first_read) != first_read or first_read < 0:
        raise ValueError("first_read must not be negative")
    return int(n_reads), int(replicate), int(seed), int(first_read)


def bootstrap_weights(n_reads, replicate, seed=0, first_read=0, device=-1):
    """How often each of `n_reads` reads numbered from `first_read` is drawn in `replicate` of the Poisson bootstrap under
    `seed` (covest_bootstrap_weights): an (n_reads,) uint32 array, what KmerCounts.add_weighted takes.  Rows [a, a + m)
    drawn with first_read = a equal the same rows of the whole."""
    n, replicate, seed, first_read = _check_weights_args(n_reads, replicate, seed, first_read)
    out = np.empty(n, dtype=np.uint32)
    _capi.check(_capi.lib().covest_bootstrap_weights(int(device), n, first_read, seed, replicate,
                                                     ctypes.c_void_p(out.ctypes.data)), "covest_bootstrap_weights")
    return out


def bootstrap_weights_device(out_ptr, n_reads, replicate, seed=0, first_read=0, stream=None, device=-1):
    """The same into `n_reads` uint32 resident in HBM at `out_ptr` (a raw device pointer, aligned to 4 bytes),
    asynchronous on `stream` (covest_bootstrap_weights_device); nothing outside them is written."""
    n, replicate, seed, first_read = _check_weights_args(n_reads, replicate, seed, first_read)
    if n and not out_ptr:
        raise ValueError("out_ptr must not be null")
    _capi.require_shared_runtime("bootstrap_weights_device")
    _capi.check(_capi.lib().covest_bootstrap_weights_device(
        int(device), n, first_read, seed, replicate, ctypes.c_void_p(out_ptr or 0), ctypes.c_void_p(stream or 0)),
        "covest_bootstrap_weights_device")


def _check_replicates(replicates):
    if isinstance(replicates, bool) or not isinstance(replicates, (int, np.integer)):
        raise ValueError("replicates must be an integer")
    if replicates < 2:
        raise ValueError("a bootstrap needs at least two replicates")
    if replicates > 1 << 20:
        raise ValueError("replicates must be within 2 .. 2^20")
    return int(replicates)


def bootstrap_histograms(reads, k, replicates, seed=0, canonical=False, device=-1):
    """(hist_full, [hist_b for b in range(replicates)], occurrences, reads_drawn) of `reads` -- a SimulatedReads, an (n,
    L) uint8 array or a pair (bases, offsets) in the packed layout --: hist_b the k-mer histogram {abundance: k-mers} of
    the reads counted bootstrap_weights(n, b, seed, first_read)[r] times each, hist_full that of all reads counted once,
    occurrences[b] = sum i hist_b[i], reads_drawn[b] the sum of replicate b's weights.

    The reads go up once and stay where they are: there is no split and no copy of them.  One buffer of n weights and
    ONE KmerCounts, whose table is reserved once for the whole set (weights never add distinct keys), serve every
    replicate: draw the weights, clear, add_weighted_device, histogram, all on the null stream.  The buffers live on the
    calling thread's current device, which `device` has to name (or -1).  Reads that do not fit the device raise
    CovestHipError; streaming a file in passes is not built."""
    replicates = _check_replicates(replicates)
    _check_seed(seed, whole=True)
    if int(k) != k or k < 1:
        raise ValueError("k must be a positive integer")
    blob, offsets, n, read_len, source = _packed(reads)
    first_read = int(source.first_read) if source is not None else 0
    from .kmer_hist import KmerCounts
    n_bases = int(offsets[-1]) if offsets is not None else n * read_len
    arena = counts = None
    try:
        arena = _DeviceArena("bootstrap_histograms")
        if device >= 0:
            current = ctypes.c_int(-1)
            arena.hip.hipGetDevice(ctypes.byref(current))
            if current.value != int(device):
                raise _capi.CovestHipError("bootstrap_histograms: the reads are staged on the calling thread's current "
                                           "device (%d), not device %d" % (current.value, device))
        try:
            d_in = arena.upload("in", blob.ctypes.data, n_bases)
            d_off = arena.upload("offsets", offsets.ctypes.data, 8 * (n + 1)) if offsets is not None else None
            d_weights = arena.reserve("weights", 4 * n)
        except _capi.CovestHipError as e:
            raise _capi.CovestHipError("bootstrap_histograms: %d bases of reads do not fit the device together with a "
                                       "weight a read (%s)" % (n_bases, e))
        counts = KmerCounts(k, canonical=canonical, device=device)
        # k-mers the whole set can add: sum(max(len - k + 1, 1)), bounded as add_packed bounds it
        counts._reserve_for(n_bases + n if offsets is not None else n * max(read_len - int(k) + 1, 1))
        counts.add_device(d_in, n, 0 if offsets is not None else read_len, d_offsets_ptr=d_off, reserve=False)
        hist_full = _hist_dict(counts)  # (waits for the counter)
        hists, drawn = [], []
        weights = np.empty(n, dtype=np.uint32)
        for b in range(replicates):
            bootstrap_weights_device(d_weights, n, b, seed=seed, first_read=first_read, device=device)
            counts.clear()
            counts.add_weighted_device(d_in, n, 0 if offsets is not None else read_len, d_weights, d_offsets_ptr=d_off,
                                       reserve=False)
            hists.append(_hist_dict(counts))
            arena.download("weights", weights)
            drawn.append(int(weights.sum(dtype=np.int64)))
        return hist_full, hists, [_occurrences(h) for h in hists], drawn
    finally:
        if counts is not None:
            counts.close()
        if arena is not None:
            arena.close()


def summarize_read_bootstrap(estimates, success, full, occurrences, occurrences_full, names, fix, level, correct_c,
                             at_bound=None):
    """The read bootstrap's arithmetic on arrays (pure numpy): `estimates` (B, P) the replicates' refits, `success` (B,),
    `full` (P,) the refit of the full set, `occurrences` (B,) and `occurrences_full` the k-mer occurrences sum i h_i of
    each set, `names` the P parameter names (the coverage first), `fix` None or P entries (None: free), `correct_c` the
    model's map from coverage to k-mer coverage, `at_bound` None or (B, P) booleans: the refit ended on a bound.

    The quantities are the jackknife's (summarize_jackknife): every parameter but the first as it is; the coverage of
    replicate b rescaled to the full read set, c_b * occurrences_full / occurrences[b] -- a Poisson replicate does not
    hold exactly n reads, what is uncertain is the genome size --; and 'genome_size' = occurrences[b] / correct_c(c_b).
    Over the B' successful refits, per quantity theta: mean; standard_errors, the sample standard deviation (ddof = 1);
    bias = mean - theta_full; intervals, the percentile interval between the (1 -+ level) / 2 quantiles
    (bootstrap._percentiles); bound_share, the share of the B' refits that ended on a bound of the parameter (the genome
    size goes with the coverage; None without `at_bound`).  None for a fixed parameter, and for everything where B' < 2.
    Also `failed` = B - B' and `used` = B'."""
    from .bootstrap import _percentiles
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    names = list(names)
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, len(names))
    ok = np.asarray(success, dtype=bool).reshape(-1)
    occ = np.asarray(occurrences, dtype=np.float64).reshape(-1)
    full = np.asarray(full, dtype=np.float64).reshape(-1)
    if not (len(est) == len(ok) == len(occ)) or len(full) != len(names):
        raise ValueError("summarize_read_bootstrap: one estimate, success flag and occurrence count per replicate")
    bound = None if at_bound is None else np.asarray(at_bound, dtype=bool).reshape(-1, len(names))
    if bound is not None and len(bound) != len(est):
        raise ValueError("summarize_read_bootstrap: one row of at_bound per replicate")
    fix = [None] * len(names) if fix is None else list(fix)
    used = int(ok.sum())
    good, good_occ = est[ok], occ[ok]
    # (quantity, its B' values, its value on the full set, free, the parameter whose bounds it ends on)
    rows = []
    for d, name in enumerate(names):
        values = good[:, d] * (float(occurrences_full) / good_occ) if d == 0 else good[:, d]
        rows.append((name, values, float(full[d]), fix[d] is None, d))
    rows.append(('genome_size', np.array([o / correct_c(c) for o, c in zip(good_occ, good[:, 0])], dtype=np.float64),
                 float(occurrences_full) / correct_c(float(full[0])), fix[0] is None, 0))
    keys = ('mean', 'standard_errors', 'bias', 'intervals', 'bound_share')
    out = {key: {} for key in keys}
    out.update(failed=int(len(ok) - used), used=used)
    for name, values, theta_full, free, d in rows:
        if not free or used < 2:
            for key in keys:
                out[key][name] = None
            continue
        mean = float(values.mean())
        lo, hi = _percentiles(values, level)
        out['mean'][name] = mean
        out['standard_errors'][name] = float(values.std(ddof=1))
        out['bias'][name] = mean - theta_full
        out['intervals'][name] = [float(lo), float(hi)]
        out['bound_share'][name] = None if bound is None else float(bound[ok][:, d].mean())
    return out


def read_bootstrap(model, estimate, reads, replicates=64, seed=0, fix=None, level=0.95, trim=None,
                   refit="lockstep-gradient", sample_factor=1, canonical=False, **estimator_options):
    """The bootstrap of `estimate` (of `model`, whose histogram is that of `reads` at k = model.k, `canonical` as it was
    counted) over `replicates` Poisson resamples of the reads.

    WHAT THE NUMBER IS.  Its spread sees the dependence between the k-mers of one read -- a read is drawn whole, m times
    or not at all -- and the randomness of where the reads start and which bases were misread.  The genome is held
    fixed: nothing here speaks about another genome of the same kind.  A replicate holds Poisson(n) reads, not n; the
    coverage is rescaled to the full set and the genome size uses the replicate's own occurrences, so the size drops
    out to first order.  The intervals are percentile intervals of the B' refits that succeeded: no normality is
    assumed, and B limits how far into the tails they can be trusted (level 0.95 wants B of a few hundred).

    WHAT WAS MEASURED (profiles/read_bootstrap_recovery.txt).  With this estimator the intervals are NOT
    usable: a read drawn twice is two identical reads, the abundance of a k-mer in a replicate has twice the variance
    the model's Poisson mixture allows, and the refits land on another coverage, every replicate alike (basic model,
    coverage 10: 7.2).  On simulated read sets the percentile intervals held the truth in 0 of 12 where read_jackknife's
    held it in 12.  `bias` shows it: where it is many standard errors of read_jackknife, do not report the intervals.

    HOW.  bootstrap_histograms gives the B + 1 histograms.  Each is cut as the model's was, and all are put on ONE key
    set on a twin of the model and refitted together from `estimate` by bootstrap._refit_lockstep: jackknife_batch and
    read_jackknife's rules, word for word (`trim`, `refit`, `fix`, the estimator's options).

    sample_factor other than 1 raises ValueError: sample_histogram rounds at random, so a bootstrap through it would not
    be a function of the reads.

    Returns summarize_read_bootstrap's dict (mean, standard_errors, bias, intervals, bound_share per parameter name and
    'genome_size'; failed, used) and: estimates (B x P, as refitted: the coverage not rescaled), success (B), at_bound
    (B x P), occurrences (B), occurrences_full, reads_drawn (B), full_estimate (row B's refit), full_success,
    full_minus_given (its distance from `estimate`), keys_added (keys of the union the model did not have), params,
    estimate, level, replicates, seed, refit."""
    replicates = _check_replicates(replicates)
    _check_seed(seed, whole=True)
    estimate = [float(v) for v in estimate]
    names = list(model.params)
    if len(estimate) != len(names):
        raise ValueError("read_bootstrap: %d parameters expected, %d given" % (len(names), len(estimate)))
    if refit not in REFITS:
        raise ValueError('refit must be "lockstep" or "lockstep-gradient"')
    if refit == "lockstep" and estimator_options.get('gradient', 'fd') != 'fd':
        raise ValueError('refit="lockstep" goes with gradient="fd" only: the analytic gradient is refit="lockstep-gradient"')
    if refit == "lockstep-gradient" and estimator_options.get('gradient', 'analytic') != 'analytic':
        raise ValueError('refit="lockstep-gradient" goes with gradient="analytic" only: finite differences are refit="lockstep"')
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    if sample_factor != 1 or getattr(model, 'sample_factor', 1) != 1:
        raise ValueError("read_bootstrap needs a model built with sample factor 1: a down-sampled histogram is rounded at "
                         "random and is not a function of the reads")
    if fix is not None and len(fix) != len(names):
        raise ValueError("read_bootstrap: fix needs one entry per parameter")
    if trim is not None and (int(trim) != trim or trim < 1):
        raise ValueError("trim must be a positive integer")
    from .bootstrap import _on_bound, _refit_lockstep

    hist_full, hists, occurrences, drawn = bootstrap_histograms(reads, model.k, replicates, seed, canonical, model.device)
    occurrences_full = _occurrences(hist_full)
    twin, batch, added = jackknife_batch(model, hists, hist_full, trim)
    try:
        estimates, success, _ = _refit_lockstep(twin, estimate, replicates + 1, seed, 0, fix, estimator_options,
                                                analytic=refit == "lockstep-gradient", batch=batch)
    finally:
        batch.close()
        twin.close()
    full = [float(v) for v in estimates[replicates]]
    out = {'replicates': replicates, 'seed': int(seed), 'refit': refit, 'level': float(level), 'params': names,
           'estimate': estimate, 'estimates': estimates[:replicates].copy(), 'success': success[:replicates].copy(),
           'at_bound': np.array([_on_bound(row, model.bounds) for row in estimates[:replicates]], dtype=bool),
           'occurrences': list(occurrences), 'occurrences_full': occurrences_full, 'reads_drawn': list(drawn),
           'full_estimate': full, 'full_success': bool(success[replicates]),
           'full_minus_given': [a - b for a, b in zip(full, estimate)], 'keys_added': added}
    out.update(summarize_read_bootstrap(out['estimates'], out['success'], full, occurrences, occurrences_full, names, fix,
                                        level, model.correct_c, at_bound=out['at_bound']))
    return out
