"""The observed information at an estimate: the Hessian of -LL in closed form from the device
(covest_eval_points_hess), its inverse over the identified parameters as a covariance, standard errors,
correlations and Wald intervals -- for every parameter and the genome size, without a grid around the estimate.
observed_information_batch does the same for every histogram of a HistogramBatch at its own point, from one call
(covest_batch_eval_pairs_hess).

What these numbers are and are not (the caveat of DESIGN.md 6d, unchanged): the model treats the k-mer counts as
independent and |LL| is 1e7..1e8 on real histograms, so the curvature is huge and the standard errors are very small.
They are the MODEL's standard errors -- how sharply this likelihood singles out its optimum -- not a statement about
how far the estimate is from the truth.  sandwich_covariance corrects them for ONE way the model can be wrong: misfit
of the mixture (the histogram does not follow the model's law), through the robust covariance A^-1 B A^-1 with B the
centred outer product of the per-k-mer scores (covest_eval_points_opg).  It does NOT correct for the
other: the unit is still one distinct k-mer counted as independent of the others, overlapping k-mers are not, and a
histogram carries no information to correct that -- robust standard errors are still far too small as a statement about
the truth.
"""
import math

import numpy as np


def _inside(value, bound):
    lo, hi = bound
    return (lo is None or value > lo) and (hi is None or value < hi)


def observed_information(model, estimate, fix=None):
    """The observed information of `model` at `estimate` (the model's parameters: the error rate NOT multiplied by an
    err_scale).  `fix`: per parameter None or the value it was held at, as CoverageEstimator takes it.

    A parameter is FREE when it is not fixed, lies strictly inside its bounds, and its row of the Hessian is not
    entirely zero (at q1 = 1 the factor (1 - q1) annihilates every q2 and q entry: those are not identified at that
    point).  The block of the free parameters is inverted by Cholesky; if it is not positive definite, or not finite,
    every standard error is None and `reason` says why -- nothing is regularised or pseudo-inverted.

    Returns a dict: hessian (of -LL, P x P, lists), free (the indices used), covariance and correlation (of the free
    block, in the order of `free`; None where there is none), standard_errors ({name: se or None}), reason (None when
    all is well), and params, estimate, bounds, loglikelihood, gradient for what builds on it (wald_intervals,
    genome_size_se, report.print_output).  See the module's docstring for what such standard errors mean."""
    est = [float(v) for v in estimate]
    names = list(model.params)
    P = len(names)
    if len(est) != P:
        raise ValueError("observed_information: %d parameters expected, %d given" % (P, len(est)))
    fix = [None] * P if fix is None else list(fix)
    if len(fix) != P:
        raise ValueError("observed_information: `fix` must have one entry per parameter")
    ll, grad, hess = model.loglikelihood_hessian_points([est])
    return _information(names, est, [tuple(b) for b in model.bounds], fix, float(np.asarray(ll).reshape(-1)[0]),
                        np.asarray(grad).reshape(-1), np.asarray(hess, dtype=np.float64).reshape(P, P))


def _information(names, est, bounds, fix, ll, grad, hess):
    """observed_information's dict from the value, gradient and Hessian OF LL at `est`: the free set, the Cholesky
    inverse of its block, `reason`.  The one place these rules are written: observed_information (one model's own
    histogram) and observed_information_batch (every histogram of a batch) both end here."""
    P = len(names)
    H = -np.asarray(hess, dtype=np.float64).reshape(P, P)
    info = {
        'params': names, 'estimate': est, 'bounds': bounds, 'loglikelihood': ll,
        'gradient': [float(v) for v in grad], 'hessian': H.tolist(), 'free': [],
        'covariance': None, 'correlation': None, 'standard_errors': {n: None for n in names}, 'reason': None,
    }
    if not np.all(np.isfinite(H)):
        info['reason'] = "the Hessian is not finite at this point"
        return info
    free = [d for d in range(P) if fix[d] is None and _inside(est[d], bounds[d]) and np.any(H[d] != 0.0)]
    info['free'] = free
    if not free:
        info['reason'] = "no free parameter: every one is fixed, on its bound or has an all-zero row"
        return info
    block = H[np.ix_(free, free)]
    try:
        chol = np.linalg.cholesky(block)
    except np.linalg.LinAlgError:
        info['reason'] = "the information of the free parameters (%s) is not positive definite" % ", ".join(
            names[d] for d in free)
        return info
    inv_chol = np.linalg.solve(chol, np.eye(len(free)))
    cov = inv_chol.T @ inv_chol
    se = np.sqrt(np.diag(cov))
    info['covariance'] = cov.tolist()
    info['correlation'] = (cov / np.outer(se, se)).tolist()
    for at, d in enumerate(free):
        info['standard_errors'][names[d]] = float(se[at])
    return info


def observed_information_batch(batch, estimates, fix=None):
    """observed_information for every histogram of a HistogramBatch at its own point: estimates[b] is the estimate of
    histogram b (B x P, the model's parameters).  ONE batch.loglikelihood_hessian_pairs(arange(B), estimates) call -- the
    derivative kernel walks each point once at order 2 and the counts enter through a contraction (DESIGN.md section
    6x) --, then per histogram the rules of observed_information: the free set, Cholesky, `reason`.  Returns the list of
    B dicts, each as observed_information's.  The standard errors of the replicates of a parametric bootstrap
    (bootstrap.parametric_bootstrap(studentized=True)); the module's docstring says what such errors mean."""
    model = batch.model
    names = list(model.params)
    P = len(names)
    est = np.asarray(estimates, dtype=np.float64).reshape(-1, P)
    if len(est) != len(batch):
        raise ValueError("observed_information_batch: one estimate per histogram of the batch")
    fix = [None] * P if fix is None else list(fix)
    if len(fix) != P:
        raise ValueError("observed_information_batch: `fix` must have one entry per parameter")
    if not len(est):
        return []
    ll, grad, hess = batch.loglikelihood_hessian_pairs(np.arange(len(est)), est)
    bounds = [tuple(b) for b in model.bounds]
    return [_information(names, [float(v) for v in est[b]], bounds, fix, float(ll[b]), grad[b], hess[b]) for b in range(len(est))]


def sandwich_covariance(model, estimate, fix=None, info=None):
    """The robust (sandwich) covariance of `estimate`: V = A^-1 B_c A^-1 over observed_information's `free` set, with
    A = -Hessian the observed information and B_c = B - g g^T / n the centred outer product of the per-k-mer scores,
    B = model.loglikelihood_score_outer_points's matrix at the estimate, g the gradient that call returns and
    n = sum h + tail the number of observations.  If the mixture is the true law of the abundances B_c ~ A and V ~ A^-1.
    `info`: observed_information's dict for the same model, estimate and fix, computed here when None.

    Returns that dict (a copy) extended with opg (B as returned, P x P, lists), robust_covariance (of the free block,
    in the order of `free`), robust_standard_errors ({name: se or None}), se_ratio ({name: robust / model or None}) and
    information_ratio (the eigenvalues of A^-1 B_c on the free block, ascending; all ~ 1 when the model fits).  Where
    the sandwich cannot be formed -- no covariance to start from, or B not finite -- these are None and `reason` says
    why; A^-1 comes from the Cholesky factor of the same block, nothing is regularised.  See the module's docstring
    for what the sandwich does and does not correct."""
    if info is None:
        info = observed_information(model, estimate, fix)
    out = dict(info)
    names = list(out['params'])
    P = len(names)
    ll, grad, opg = model.loglikelihood_score_outer_points([out['estimate']])
    B = np.asarray(opg, dtype=np.float64).reshape(P, P)
    g = np.asarray(grad, dtype=np.float64).reshape(P)
    out.update(opg=B.tolist(), robust_covariance=None, robust_standard_errors={n: None for n in names},
               se_ratio={n: None for n in names}, information_ratio=None)
    if out['covariance'] is None:
        if out['reason'] is None:
            out['reason'] = "no covariance of the model to build the sandwich on"
        return out
    free = list(out['free'])
    if not (np.all(np.isfinite(B)) and np.all(np.isfinite(g))):
        out['reason'] = "the outer product of the scores is not finite at this point"
        return out
    n_obs = float(sum(model.hist.values())) + float(model.tail)
    A = np.asarray(out['hessian'], dtype=np.float64)[np.ix_(free, free)]
    centred = B[np.ix_(free, free)] - np.outer(g[free], g[free]) / n_obs
    inv_chol = np.linalg.solve(np.linalg.cholesky(A), np.eye(len(free)))
    middle = inv_chol @ centred @ inv_chol.T  # L^-1 B_c L^-T: similar to A^-1 B_c, and symmetric
    cov = inv_chol.T @ middle @ inv_chol
    out['robust_covariance'] = cov.tolist()
    out['information_ratio'] = [float(v) for v in np.linalg.eigvalsh(middle)]
    for at, d in enumerate(free):
        if cov[at, at] >= 0.0:
            se = math.sqrt(cov[at, at])
            out['robust_standard_errors'][names[d]] = se
            out['se_ratio'][names[d]] = se / out['standard_errors'][names[d]]
    return out


def _z(level):
    if not (isinstance(level, (int, float)) and 0.0 < level < 1.0):
        raise ValueError("level must be inside (0, 1)")
    from scipy.stats import norm  # (here, not at import: model construction stays free of scipy)
    return float(norm.ppf(0.5 + 0.5 * level))


def wald_intervals(info, level=0.95, robust=False):
    """{name: (lo, hi) or None}: estimate +- z se with z the normal quantile of `level`, clipped to the model's bounds;
    None where the parameter has no standard error.  The model's intervals (module docstring), or with `robust` those of
    sandwich_covariance's robust_standard_errors (`info` is then its dict)."""
    z = _z(level)
    errors = info['robust_standard_errors' if robust else 'standard_errors']
    out = {}
    for name, value, (lo, hi) in zip(info['params'], info['estimate'], info['bounds']):
        se = errors[name]
        if se is None:
            out[name] = None
            continue
        a, b = value - z * se, value + z * se
        out[name] = (a if lo is None else max(a, lo), b if hi is None else min(b, hi))
    return out


def genome_size_se(model, hist_orig, info, sample_factor=1, level=0.95, robust=False):
    """The delta method on G = sum_i i h_i / correct_c(c * sample_factor): G is proportional to 1 / c, so
    se_G = G se_c / c.  Returns {'genome_size': G (not rounded), 'genome_size_se', 'genome_size_wald_interval':
    (G - z se_G, G + z se_G)}; the last two None where the coverage has no standard error.  `info`:
    observed_information's dict, or with `robust` sandwich_covariance's, whose robust standard error is then used."""
    z = _z(level)
    scale = 1 if sample_factor is None else sample_factor
    c = info['estimate'][0]
    occurrences = sum(i * n for i, n in hist_orig.items())
    corrected = model.correct_c(c * scale)
    size = occurrences / corrected if corrected != 0 else float('inf')
    se_c = info['robust_standard_errors' if robust else 'standard_errors'][info['params'][0]]
    if se_c is None or not math.isfinite(size):
        return {'genome_size': size, 'genome_size_se': None, 'genome_size_wald_interval': None}
    se = size * se_c / abs(c)
    return {'genome_size': size, 'genome_size_se': se, 'genome_size_wald_interval': (size - z * se, size + z * se)}
