"""The parametric bootstrap of an estimate: histograms drawn from the MODEL at a known
parameter point, each refitted, and the centre and spread of the refits.

    est, ok = CoverageEstimator(model).compute_coverage(guess)
    boot = parametric_bootstrap(model, est, replicates=100, seed=1, hist_orig=hist_orig, sample_factor=sf)
    print_output(hist_orig, model, ok, sf, estimated=est, bootstrap=boot)

It answers what curvature at the estimate (Wald intervals, the sandwich, the profile) cannot: whether the estimator is
biased at this coverage even when the data are exactly the model's, and how far from normal its distribution is --
bias, standard errors, percentile intervals, the share of refits that fail or end on a bound.

What it is not: a replicate is n independent draws from the model's cell probabilities, the same independence
assumption the Wald errors make.  It measures bias and non-normality of the estimator UNDER THE MODEL, not the
dependence between overlapping k-mers; its standard errors are as small as the model's own.

studentized=True adds the bootstrap-t interval: every replicate's observed information at its own refit comes from ONE
batch call (information.observed_information_batch), t_b = (theta_b - theta^) / se_b is formed per
parameter, and the interval is [theta^ - q_hi se, theta^ - q_lo se] with q the quantiles of t and se the original's own
standard error.  It is second-order accurate where the percentile interval is first-order: it corrects the estimator's
skew and bias UNDER THE MODEL.  The caveat above holds for it unchanged -- it does not correct the dependence between
overlapping k-mers, and it is as narrow as the model's own errors.

The generator is a device kernel (draw_hist.hip; the definition of a draw is in include/covest_amd.h): every count is
a stated function of (weights, seed, replicate, draw index), so a run is reproducible, a run of replicates equals the
same rows of a larger run, and n draws are the first n of any longer row.  There is no CPU path: without the library
or a HIP device draw_histograms raises CovestHipError.
"""
import ctypes
import math

import numpy as np

from . import _capi
from .read_sets import check_refit_request

# the kernel's constants (csrc/kernels.h; tests/test_draw_cpu.py compares): the cap on m, the two LDS layouts' limits,
# the guide table's size and the draws a workgroup takes
MAX_CELLS = 65536
LDS_BOTH_CELLS = 12288
LDS_THRESHOLD_CELLS = 16384
GUIDE_SIZE = 2048
CHUNK_DRAWS = 1 << 17


def _weights_array(weights):
    """The argument rules of covest_draw_thresholds, before the library is asked (ValueError)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError("weights must be one-dimensional, at least one")
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("a weight is negative, NaN or infinite")
    with np.errstate(over="ignore"):
        total = float(np.cumsum(w)[-1])
    if not (total > 0.0 and math.isfinite(total)):
        raise ValueError("the weights' total is 0 or not finite")
    return w


def draw_thresholds(weights):
    """uint64[m]: t_i = floor(cdf_i / total * 2^63), the thresholds a draw is compared with (include/covest_amd.h).
    Host arithmetic of the library: needs no device."""
    w = _weights_array(weights)
    out = np.empty(w.size, dtype=np.uint64)
    _capi.check(_capi.lib().covest_draw_thresholds(w.size, w.ctypes.data, out.ctypes.data), "covest_draw_thresholds")
    return out


def _check_draws(m, n_draws, replicates, seed, first_replicate):
    if int(n_draws) != n_draws or n_draws < 0:
        raise ValueError("n_draws must be an integer, not negative")
    if int(replicates) != replicates or replicates < 0:
        raise ValueError("replicates must be an integer, not negative")
    if int(first_replicate) != first_replicate or first_replicate < 0 or first_replicate + replicates > 1 << 32:
        raise ValueError("a replicate index must be in 0 .. 2^32 - 1")
    if int(seed) != seed or not (0 <= seed < 1 << 64):
        raise ValueError("seed must fit 64 bits")
    if m > MAX_CELLS:
        raise ValueError("more than %d cells" % MAX_CELLS)


def draw_histograms(weights, n_draws, replicates, seed=0, first_replicate=0, device=-1):
    """int64 (replicates, m): row b counts, by cell, `n_draws` independent draws of replicate first_replicate + b from
    the distribution weights / sum(weights).  Drawn on the device (covest_draw_histograms)."""
    w = _weights_array(weights)
    _check_draws(w.size, n_draws, replicates, seed, first_replicate)
    out = np.empty((int(replicates), w.size), dtype=np.int64)
    _capi.check(_capi.lib().covest_draw_histograms(int(device), w.size, w.ctypes.data, int(n_draws), int(first_replicate),
                                                   int(replicates), int(seed), out.ctypes.data), "covest_draw_histograms")
    return out


def draw_histograms_device(thresholds_ptr, m, n_draws, replicates, out_ptr, seed=0, first_replicate=0, stream=None,
                           device=-1):
    """The same into replicates * m int64 of device memory at `out_ptr` from `m` thresholds (draw_thresholds) resident
    at `thresholds_ptr` (raw device pointers); asynchronous on `stream`."""
    if int(m) != m or m < 1:
        raise ValueError("m must be at least 1")
    _check_draws(m, n_draws, replicates, seed, first_replicate)
    _capi.require_shared_runtime("draw_histograms_device")
    _capi.check(_capi.lib().covest_draw_histograms_device(
        int(device), int(m), ctypes.c_void_p(thresholds_ptr), int(n_draws), int(first_replicate), int(replicates),
        int(seed), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0)), "covest_draw_histograms_device")


def model_cells(model, estimate):
    """(keys, weights, has_tail): the cells a replicate of `model`'s histogram is drawn over.  The weights are p_j at
    every key of the histogram, in its order, from compute_probabilities at the estimate after fit_to_bounds; with a
    tail (model.tail != 0) one more cell max(0, 1 - fsum(p)) takes the abundances beyond the keys.  Without a tail
    the draw is conditional on the keys: the weights are normalised by the thresholds' division by their total."""
    args = model.fit_to_bounds(list(estimate))
    p = model.compute_probabilities(*args)
    keys = list(model.hist.keys())
    weights = [float(p[j]) for j in keys]
    has_tail = model.tail != 0
    if has_tail:
        weights.append(max(0.0, 1.0 - math.fsum(weights)))
    return np.asarray(keys, dtype=np.int64), np.asarray(weights, dtype=np.float64), has_tail


def _replicate_model(model, keys, counts, tail):
    """A model of `model`'s class and settings on the histogram (keys, counts) -- the same key set, zero counts kept,
    so that the sum of p_j runs over the same keys."""
    options = {'max_error': model.max_error, 'device': model.device}
    if getattr(model, 'threshold', None) is not None:
        options['threshold'] = model.threshold
    twin = model.__class__(model.k, model.r, (np.asarray(keys, dtype=np.int32), np.asarray(counts, dtype=np.float64)),
                           tail, **options)
    twin.bounds = model.bounds
    twin.defaults = model.defaults
    return twin


def _refit(model, keys, counts, tail, estimate, fix, estimator_options):
    """(estimate, success, log-likelihood) of one replicate, refitted from `estimate`; its model is closed here."""
    from .estimator import CoverageEstimator
    twin = _replicate_model(model, keys, counts, tail)
    try:
        x, success = CoverageEstimator(twin, fix=fix, **estimator_options).compute_coverage(list(estimate))
        return [float(v) for v in x], bool(success), float(twin.compute_loglikelihood(*x))
    finally:
        twin.close()


def _refit_lockstep(model, estimate, replicates, seed, n_draws, fix, estimator_options, analytic=False, batch=None):
    """(estimates, success, log-likelihoods) of all replicates refitted TOGETHER: the histograms are drawn into a
    HistogramBatch and never leave the device, one CoverageEstimator._optimize per replicate runs under the estimator's
    _LockStep, and a merged round -- every replicate's point and its finite-difference neighbours -- is ONE
    loglikelihood_pairs call, each request tagged with its replicate.  No model per replicate.

    analytic (refit="lockstep-gradient"): the estimators run with gradient="analytic", a round holds ONE request per live
    replicate instead of P + 1, and is ONE loglikelihood_gradient_pairs call whose values and gradients go back as the
    rows negll_gradient_points returns (optimiser space: CoverageEstimator._optimiser_rows).  `batch`: the histograms,
    where the caller has them already (it stays the caller's)."""
    from .batch import HistogramBatch
    from .estimator import CoverageEstimator, _LockStep
    route = "lockstep-gradient" if analytic else "lockstep"
    if analytic:
        estimator_options = dict(estimator_options, gradient="analytic")
    est = CoverageEstimator(model, fix=fix, **estimator_options)
    if not est.batched or est.reference_specials:
        raise ValueError('refit="%s" goes with neither batched=False nor reference_specials=True' % route)
    own = batch is None
    if own:
        batch = HistogramBatch.draw(model, estimate, replicates, seed=seed, n_draws=n_draws)
    try:
        def evaluate_merged(requests):  # [(replicate, optimiser-space vector)] of one round
            index = [b for b, _ in requests]
            points = np.array([est._model_args(x) for _, x in requests], dtype=np.float64)
            if analytic:
                return est._optimiser_rows(*batch.loglikelihood_gradient_pairs(index, points))
            return -batch.loglikelihood_pairs(index, points)

        start = list(estimate)
        start[est.ERROR_RATE] *= est.err_scale

        def refine(b, evaluate):
            return est._optimize(start, lambda xs: evaluate([(b, x) for x in xs]))

        results = _LockStep(evaluate_merged, replicates).map(refine, list(range(replicates)))
        estimates = np.empty((replicates, len(estimate)), dtype=np.float64)
        for b, res in enumerate(results):
            x = [float(v) for v in res.x]
            x[est.ERROR_RATE] /= est.err_scale
            estimates[b] = x
        success = np.array([bool(res.success) for res in results], dtype=bool)
        loglik = batch.loglikelihood_pairs(np.arange(replicates), estimates) if replicates else np.empty(0)
        return estimates, success, loglik
    finally:
        if own:
            batch.close()


def _on_bound(values, bounds):
    return [(lo is not None and v <= lo) or (hi is not None and v >= hi) for v, (lo, hi) in zip(values, bounds)]


def _percentiles(values, level):
    lo, hi = np.percentile(values, [50.0 * (1.0 - level), 50.0 * (1.0 + level)], axis=0)
    return lo, hi


def summarize(estimates, success, estimate, names, fix=None, level=0.95):
    """The summary of B refits over the successful ones: {mean, bias, standard_errors, percentile_intervals} per
    parameter name and `failed`.  bias = mean - estimate; the standard error is the sample standard deviation (n - 1;
    None below two refits); the interval runs between the (1 -+ level) / 2 quantiles (numpy's linear interpolation).
    A parameter fixed by `fix` gives None everywhere."""
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, len(names))
    ok = np.asarray(success, dtype=bool).reshape(-1)
    good = est[ok]
    fix = [None] * len(names) if fix is None else list(fix)
    out = {'mean': {}, 'bias': {}, 'standard_errors': {}, 'percentile_intervals': {}, 'failed': int((~ok).sum())}
    lo, hi = _percentiles(good, level) if len(good) else (None, None)
    for d, name in enumerate(names):
        free = fix[d] is None and len(good) > 0
        mean = float(good[:, d].mean()) if free else None
        out['mean'][name] = mean
        out['bias'][name] = mean - float(estimate[d]) if free else None
        out['standard_errors'][name] = float(good[:, d].std(ddof=1)) if free and len(good) > 1 else None
        out['percentile_intervals'][name] = [float(lo[d]), float(hi[d])] if free else None
    return out


def t_intervals(estimates, success, replicate_se, estimate, standard_errors, names, level=0.95):
    """The bootstrap-t arithmetic on arrays: (intervals, used).  Per parameter d the replicates that succeeded and have a
    standard error (finite, > 0) give t_b = (estimates[b, d] - estimate[d]) / replicate_se[b, d]; used[name] counts them;
    intervals[name] = [estimate[d] - q_hi se, estimate[d] - q_lo se] with q_lo, q_hi the (1 -+ level) / 2 quantiles of t
    (numpy's linear interpolation) and se = standard_errors[name], the original's -- None where that is None or fewer
    than two replicates qualify."""
    if not (0.0 < level < 1.0):
        raise ValueError("level must be in (0, 1)")
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, len(names))
    rse = np.asarray(replicate_se, dtype=np.float64).reshape(-1, len(names))
    ok = np.asarray(success, dtype=bool).reshape(-1)
    intervals, used = {}, {}
    for d, name in enumerate(names):
        with np.errstate(invalid="ignore"):
            take = ok & np.isfinite(rse[:, d]) & (rse[:, d] > 0.0) & np.isfinite(est[:, d])
        used[name] = int(take.sum())
        se = standard_errors.get(name)
        if se is None or used[name] < 2:
            intervals[name] = None
            continue
        t = (est[take, d] - float(estimate[d])) / rse[take, d]
        q_lo, q_hi = _percentiles(t, level)
        intervals[name] = [float(estimate[d] - q_hi * se), float(estimate[d] - q_lo * se)]
    return intervals, used


def _replicate_standard_errors(infos, names):
    """B x P from observed_information_batch's dicts, NaN where a replicate has no standard error for the parameter."""
    out = np.full((len(infos), len(names)), np.nan)
    for b, info in enumerate(infos):
        for d, name in enumerate(names):
            if info['standard_errors'][name] is not None:
                out[b, d] = info['standard_errors'][name]
    return out


def parametric_bootstrap(model, estimate, replicates=100, seed=0, fix=None, level=0.95, hist_orig=None, sample_factor=1,
                         refit="sequential", studentized=False, **estimator_options):
    """`replicates` histograms of round(sum(counts) + tail) draws from `model` at `estimate` (model_cells), each
    refitted by CoverageEstimator(model_b, fix=fix, **estimator_options) started at `estimate`, one after the other.

    refit="lockstep": the same replicates (the same draws) as a HistogramBatch on the device, all refits advancing
    together, one loglikelihood_pairs launch per round and no model per replicate (_refit_lockstep).  Finite-difference
    gradients only: with gradient="analytic" it raises ValueError -- that is the next route's.  The two routes evaluate
    with different kernels, so a refit may stop an L-BFGS-B step apart; the result has the same keys, and `refit`.

    refit="lockstep-gradient": the same draws and the same lock step, each refit a CoverageEstimator(gradient="analytic"):
    a round holds one request per live replicate, not P + 1, and is one loglikelihood_gradient_pairs call -- the batch's
    analytic gradient, without the 1e-8 differencing step.  It honours `fix` and err_scale;
    gradient="fd" with it raises ValueError.

    Returns a dict: replicates, seed, n_draws; estimates (B x P), success (B), loglikelihood (B), at_bound (B x P: the
    refit ended on a bound of the model); mean, bias (mean - estimate), standard_errors and percentile_intervals at
    `level` per parameter name over the successful refits (None for a fixed parameter), failed; and, with `hist_orig`,
    genome_size {mean, standard_error, interval}: a replicate's genome size is sum i * h_i of hist_orig -- held
    fixed: the number of k-mer occurrences is a property of the read set -- over correct_c(c_b * sample_factor).

    studentized=True, on every `refit` route: the replicates' observed information at their own refits from one batch
    call (information.observed_information_batch; the lock-step routes keep their batch for it, the sequential route
    builds HistogramBatch(model, counts, tails) from the rows it drew), and three more keys: replicate_standard_errors
    (B x P, NaN where a replicate has none: a fixed parameter, one on its bound, an information that is not positive
    definite), studentized_used (per name the replicates behind t) and t_intervals (t_intervals above, with
    information.observed_information(model, estimate, fix)'s standard errors of the original); with `hist_orig`
    genome_size['t_interval'], the coverage interval's endpoints through the monotone map c -> genome size.
    See the module's docstring for what these numbers do and do not say."""
    replicates, seed = int(replicates), int(seed)
    estimate, names = check_refit_request("parametric_bootstrap", model, estimate, refit, estimator_options, level,
                                          refits=("sequential", "lockstep", "lockstep-gradient"))
    n_draws = int(round(float(sum(model.hist.values())) + float(model.tail)))
    estimates = np.full((replicates, len(names)), np.nan)
    success = np.zeros(replicates, dtype=bool)
    loglik = np.full(replicates, np.nan)
    at_bound = np.zeros((replicates, len(names)), dtype=bool)
    batch = None  # (studentized) the replicates' histograms, for their observed information
    try:
        if refit != "sequential":
            if studentized:
                from .batch import HistogramBatch
                batch = HistogramBatch.draw(model, estimate, replicates, seed=seed, n_draws=n_draws)
            estimates, success, loglik = _refit_lockstep(model, estimate, replicates, seed, n_draws, fix, estimator_options,
                                                         analytic=refit == "lockstep-gradient", batch=batch)
            for b in range(replicates):
                at_bound[b] = _on_bound(estimates[b], model.bounds)
        else:
            keys, weights, has_tail = model_cells(model, estimate)
            counts = draw_histograms(weights, n_draws, replicates, seed=seed, device=model.device)
            n_keys = len(keys)
            for b in range(replicates):
                tail_b = int(counts[b, n_keys]) if has_tail else 0
                x, ok, ll = _refit(model, keys, counts[b, :n_keys], tail_b, estimate, fix, estimator_options)
                estimates[b], success[b], loglik[b] = x, ok, ll
                at_bound[b] = _on_bound(x, model.bounds)
            if studentized:
                from .batch import HistogramBatch
                batch = HistogramBatch(model, counts[:, :n_keys].astype(np.float64),
                                       counts[:, n_keys].astype(np.float64) if has_tail else None)
        if studentized:
            from .information import observed_information, observed_information_batch
            replicate_se = _replicate_standard_errors(observed_information_batch(batch, estimates, fix), names)
            original = observed_information(model, estimate, fix)
    finally:
        if batch is not None:
            batch.close()
    out = {'replicates': replicates, 'seed': seed, 'n_draws': n_draws, 'level': float(level), 'params': names,
           'estimate': estimate, 'estimates': estimates, 'success': success, 'loglikelihood': loglik, 'at_bound': at_bound,
           'refit': refit}
    out.update(summarize(estimates, success, estimate, names, fix=fix, level=level))
    if studentized:
        intervals, used = t_intervals(estimates, success, replicate_se, estimate, original['standard_errors'], names, level)
        out.update(replicate_standard_errors=replicate_se, studentized_used=used, t_intervals=intervals)
    if hist_orig is not None:
        occurrences = sum(i * h for i, h in hist_orig.items())
        good = estimates[success, 0]
        sizes = np.array([occurrences / model.correct_c(c * sample_factor) for c in good], dtype=np.float64)
        lo, hi = _percentiles(sizes, level) if len(sizes) else (None, None)
        out['genome_size'] = {'mean': float(sizes.mean()) if len(sizes) else None,
                              'standard_error': float(sizes.std(ddof=1)) if len(sizes) > 1 else None,
                              'interval': [float(lo), float(hi)] if len(sizes) else None}
        if studentized:  # (the genome size falls as the coverage rises: the endpoints change places)
            c_int = out['t_intervals'][names[0]]
            ends = None if c_int is None else [model.correct_c(c * sample_factor) for c in c_int]
            out['genome_size']['t_interval'] = (sorted(float(occurrences / v) for v in ends)
                                                if ends is not None and all(v > 0 for v in ends) else None)
    return out
