"""The observed information at an estimate: the Hessian of -LL in closed form from the device
(covest_eval_points_hess), its inverse over the identified parameters as a covariance, standard errors,
correlations and Wald intervals -- for every parameter and the genome size, without a grid around the estimate.

What these numbers are and are not (the caveat of DESIGN.md 6d, unchanged): the model treats the k-mer counts as
independent and |LL| is 1e7..1e8 on real histograms, so the curvature is huge and the standard errors are very small.
They are the MODEL's standard errors -- how sharply this likelihood singles out its optimum -- not a statement about
how far the estimate is from the truth.  Nothing here corrects for that (no sandwich covariance).
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
    H = -np.asarray(hess, dtype=np.float64).reshape(P, P)
    bounds = [tuple(b) for b in model.bounds]
    info = {
        'params': names, 'estimate': est, 'bounds': bounds, 'loglikelihood': float(np.asarray(ll).reshape(-1)[0]),
        'gradient': [float(v) for v in np.asarray(grad).reshape(-1)], 'hessian': H.tolist(), 'free': [],
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


def _z(level):
    if not (isinstance(level, (int, float)) and 0.0 < level < 1.0):
        raise ValueError("level must be inside (0, 1)")
    from scipy.stats import norm  # (here, not at import: model construction stays free of scipy)
    return float(norm.ppf(0.5 + 0.5 * level))


def wald_intervals(info, level=0.95):
    """{name: (lo, hi) or None}: estimate +- z se with z the normal quantile of `level`, clipped to the model's bounds;
    None where the parameter has no standard error.  The model's intervals (module docstring)."""
    z = _z(level)
    out = {}
    for name, value, (lo, hi) in zip(info['params'], info['estimate'], info['bounds']):
        se = info['standard_errors'][name]
        if se is None:
            out[name] = None
            continue
        a, b = value - z * se, value + z * se
        out[name] = (a if lo is None else max(a, lo), b if hi is None else min(b, hi))
    return out


def genome_size_se(model, hist_orig, info, sample_factor=1, level=0.95):
    """The delta method on G = sum_i i h_i / correct_c(c * sample_factor): G is proportional to 1 / c, so
    se_G = G se_c / c.  Returns {'genome_size': G (not rounded), 'genome_size_se', 'genome_size_wald_interval':
    (G - z se_G, G + z se_G)}; the last two None where the coverage has no standard error.  `info`:
    observed_information's dict."""
    z = _z(level)
    scale = 1 if sample_factor is None else sample_factor
    c = info['estimate'][0]
    occurrences = sum(i * n for i, n in hist_orig.items())
    corrected = model.correct_c(c * scale)
    size = occurrences / corrected if corrected != 0 else float('inf')
    se_c = info['standard_errors'][info['params'][0]]
    if se_c is None or not math.isfinite(size):
        return {'genome_size': size, 'genome_size_se': None, 'genome_size_wald_interval': None}
    se = size * se_c / abs(c)
    return {'genome_size': size, 'genome_size_se': se, 'genome_size_wald_interval': (size - z * se, size + z * se)}
