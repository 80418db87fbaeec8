"""Profile likelihood: a dense grid reduced over its nuisance axes on the device, and the likelihood-ratio interval
read off a one-dimensional profile.

The profile of -LL over the axes in `keep` is, per cell of their product, the minimum of -LL over the grid's nodes of
the other axes (covest_grid_axis_min; the selection rule of covest/grid.py:65-70 per cell).  For `keep = (coverage,
error_rate)` it is the picture notebooks/VisualiseLikelihood.ipynb draws with q1, q2, q frozen, here minimised over
them; for `keep = (coverage,)` it gives the interval {c : -LL_prof(c) - min <= chi2_1(level) / 2}.

What the interval is and is not: the model treats the k-mer counts as independent and |LL| is 1e7..1e8
on real histograms, so the interval is very narrow; and the profile is a minimum over the GRID's nuisance nodes, not
over the continuum.  It is the model's statement, reported as such.
"""
import math

import numpy as np

from . import grid as _grid


def profile_negll(model, axes, keep, kernel="auto", devices=None):
    """Evaluate the dense grid `axes` and reduce it over the axes not in `keep` (numbers or parameter names), one
    call: (negll, flat_index, grid_shape) -- the two arrays shaped like the kept axes, flat_index into the whole grid
    (np.unravel_index(flat_index, grid_shape) gives the nuisance nodes that attain the minimum; -1: no node of the
    cell is below +inf).  devices: HIP ordinals to spread the grid's blocks over (grid.DeviceBlocks)."""
    _grid.resolve_keep(model.params, keep)  # (a bad `keep` is refused before anything is evaluated)
    shape = tuple(len(a) for a in axes)
    if devices is not None:
        blocks = _grid.DeviceBlocks(model, axes, list(devices))
        try:
            blocks.evaluate(kernel=kernel)
            val, idx = blocks.axis_minima(keep)
        finally:
            blocks.close()
        return val, idx, shape
    g = _grid.DenseGrid(model, axes)
    try:
        g.evaluate(kernel=kernel)
        val, idx = g.axis_minima(keep)
    finally:
        g.close()
    return val, idx, shape


def likelihood_interval(values, profile, level=0.95):
    """The likelihood-ratio interval of a 1-D profile: `values` the axis nodes (ascending), `profile` -LL minimised
    over everything else at each.  Threshold min + chi2_1.ppf(level) / 2; an endpoint is where the straight line
    between the last node inside and the first node outside, going out from the minimum, crosses it.  A side on which
    the profile never rises above the threshold before the axis ends is OPEN: None, never the axis end.  Non-finite
    cells count as outside (an endpoint next to one is the last node inside).  Returns (lo, hi, argmin_value)."""
    from scipy.stats import chi2  # (here, not at import: model construction stays free of scipy, models._comb_float)
    x = np.asarray(values, dtype=np.float64).reshape(-1)
    p = np.asarray(profile, dtype=np.float64).reshape(-1)
    if x.shape != p.shape or x.size == 0:
        raise ValueError("likelihood_interval: values and profile must be 1-D of one length")
    if not 0.0 < level < 1.0:
        raise ValueError("likelihood_interval: level must be inside (0, 1)")
    finite = np.isfinite(p)
    if not finite.any():
        raise ValueError("likelihood_interval: the profile has no finite cell")
    best = int(np.flatnonzero(finite & (p == p[finite].min()))[0])  # (the first minimum, as everywhere)
    threshold = p[best] + 0.5 * float(chi2.ppf(level, 1))

    def side(step):
        i = best
        while True:
            j = i + step
            if j < 0 or j >= x.size:
                return None  # the axis ended inside the interval
            if not finite[j]:
                return float(x[i])
            if p[j] > threshold:
                return float(x[i] + (threshold - p[i]) * (x[j] - x[i]) / (p[j] - p[i]))
            i = j

    return side(-1), side(+1), float(x[best])


def genome_size_at(model, hist_orig, coverage, sample_factor=1):
    """covest/data.py:152-156 at one coverage: round(sum_i i h_i / correct_c(c * sample_factor)); None for None
    (an open side) and where the quotient is infinite."""
    if coverage is None:
        return None
    occurrences = sum(i * n for i, n in hist_orig.items())
    size = round(occurrences / model.correct_c(coverage * sample_factor))
    return None if size == float('inf') else int(size)


def coverage_interval(model, estimate, axes, level=0.95, sample_factor=1, hist_orig=None, kernel="auto", devices=None):
    """The likelihood-ratio interval of the coverage from the profile along axis 0 of the grid `axes`, which the
    caller lays around `estimate` (the estimated parameters; wide enough for both sides to close, fine enough for the
    interval to hold a few nodes).  Returns a dict: coverage_interval (lo, hi) in the units of the record's
    `coverage` (times sample_factor; None = open side), coverage_argmin (the profile's best node), level, estimate,
    and genome_size_interval -- with `hist_orig`, the genome size at the two endpoints, the order reversed since a
    larger coverage is a smaller genome -- else None.  print_output(..., intervals=) takes it."""
    val, _, _ = profile_negll(model, axes, (0,), kernel=kernel, devices=devices)
    lo, hi, at = likelihood_interval(axes[0], val, level)
    scale = 1 if sample_factor is None else sample_factor
    out = {
        'coverage_interval': (None if lo is None else lo * scale, None if hi is None else hi * scale),
        'coverage_argmin': at * scale,
        'genome_size_interval': None,
        'level': float(level),
        'estimate': tuple(float(v) for v in estimate),
    }
    if hist_orig is not None:
        out['genome_size_interval'] = (genome_size_at(model, hist_orig, hi, scale), genome_size_at(model, hist_orig, lo, scale))
    return out
