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
from .read_sets import (REFITS, ResidentReads, _occurrences, check_refit_request, check_sets, quantity_rows,
                        refit_histogram_set)
from .simulate import _check_first_read, _check_seed


def _check_weights_args(n_reads, replicate, seed, first_read):
    """The argument rules of covest_bootstrap_weights, before the library is asked (ValueError)."""
    if int(n_reads) != n_reads or n_reads < 0:
        raise ValueError("n_reads must not be negative")
    if isinstance(replicate, bool) or int(replicate) != replicate or not 0 <= replicate < 1 << 32:
        raise ValueError("replicate must fit 32 bits, not negative")
    _check_seed(seed, whole=True)
    return int(n_reads), int(replicate), int(seed), _check_first_read(first_read)


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
    replicates = check_sets("replicates", replicates, "bootstrap", 1 << 20, "2^20")
    _check_seed(seed, whole=True)
    with ResidentReads(reads, k, canonical, device, "bootstrap_histograms", "a weight a read") as rs:
        d_weights = rs.reserve("weights", 4 * rs.n)
        rs.open_counter()
        rs.count(rs.d_in, rs.d_offsets, 0, rs.n)
        hist_full = rs.histogram()
        hists, drawn = [], []
        weights = np.empty(rs.n, dtype=np.uint32)
        for b in range(replicates):
            bootstrap_weights_device(d_weights, rs.n, b, seed=seed, first_read=rs.first_read, device=device)
            rs.clear()
            rs.count(rs.d_in, rs.d_offsets, 0, rs.n, d_weights)
            hists.append(rs.histogram())
            rs.download("weights", weights)
            drawn.append(int(weights.sum(dtype=np.int64)))
        return hist_full, hists, [_occurrences(h) for h in hists], drawn


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
    used, ok, rows = quantity_rows("summarize_read_bootstrap", estimates, success, full, occurrences, occurrences_full,
                                   names, fix, level, correct_c, "replicate")
    bound = None if at_bound is None else np.asarray(at_bound, dtype=bool).reshape(-1, len(rows) - 1)
    if bound is not None and len(bound) != len(ok):
        raise ValueError("summarize_read_bootstrap: one row of at_bound per replicate")
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
    replicates = check_sets("replicates", replicates, "bootstrap", 1 << 20, "2^20")
    _check_seed(seed, whole=True)
    estimate, names = check_refit_request("read_bootstrap", model, estimate, refit, estimator_options, level, fix, trim,
                                          sample_factor, REFITS)
    hist_full, hists, _, drawn = bootstrap_histograms(reads, model.k, replicates, seed, canonical, model.device)
    out = {'replicates': replicates}
    for key, value in refit_histogram_set(model, estimate, hists, hist_full, seed, fix, level, trim, refit,
                                          estimator_options).items():
        out[key] = value
        if key == 'occurrences_full':  # (the replicates' sizes stand beside their occurrences)
            out['reads_drawn'] = list(drawn)
    out.update(summarize_read_bootstrap(out['estimates'], out['success'], out['full_estimate'], out['occurrences'],
                                        out['occurrences_full'], names, fix, level, model.correct_c, at_bound=out['at_bound']))
    return out
