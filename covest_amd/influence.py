"""The influence of single reads on the score, and the linearised delete-one jackknife: a
read-level standard error from ONE pass over the reads, with no recount and no refit.

    est, ok = CoverageEstimator(model).compute_coverage(guess)
    counts = KmerCounts(model.k, canonical=...).add_reads(reads)
    infl = read_influence(model, est, counts, reads)
    print_output(hist_orig, model, ok, 1, estimated=est, read_influence=infl)

Write the log-likelihood as L(theta) = sum over the distinct k-mers x of log p_{a(x)}(theta), cut into a tail at the
trim, and g(a) = grad log p_a, with g(0) = 0 (the k-mer vanishes) and g(a) = grad log(1 - sum p_j) at and beyond the
trim.  Deleting read r moves every distinct key x of r from abundance a_x to a_x - m_x, m_x its windows in r, so

    Delta_r = grad L_(-r)(theta) - grad L(theta) = sum over the distinct x of r of [ g(a_x - m_x) - g(a_x) ]

exactly.  The device forms these rows from the k-mer table and the table of g (kmer_influence.hip); one Newton step
gives theta_(-r) - theta ~ A^-1 Delta_r with A the observed information, and the delete-one jackknife variance is
(n - 1) / n A^-1 C A^-1 with C the centred cross-moments of the rows (the moments kernel, same file).

WHAT THE NUMBER CLAIMS.  The genome is held fixed; the step is first order in A^-1 (the refit of the jackknife is
replaced by one Newton step from the full estimate, at the full set's information); and it is delete-ONE, known from n
reads, where jackknife.read_jackknife is delete-a-group, known from G groups.  A read shorter than k: the counter counts
a pseudo-key for it, the influence gives it zero.  There is no CPU path: without the library or a HIP device the calls
raise CovestHipError.
"""
import ctypes
import math

import numpy as np

from . import _capi
from .batch import pair_index
from .read_sets import check_refit_request

MAX_MOMENT_COLUMNS = 9  # csrc/kmer_influence.h kMomentsMaxQ


def score_rows(model, estimate):
    """(twin, table) for KmerCounts.read_influence: the table of g(a) = grad log p_a of `model` at `estimate`.

    `twin` is bootstrap._replicate_model of the model on the DENSE key set 1 .. max key: zero counts kept, the model's
    counts and tail.  `table` is (max key + 1 + [1 if model.tail else 0], P): row 0 is zeros (a k-mer that vanishes), row a
    the score d_k p_a / p_a of key a from HistogramBatch(twin, ...).score_table([estimate]), and -- when the model has
    a tail -- the last row is the tail's score grad log(1 - sum p_j), which every abundance at or beyond the trim takes.

    Where the model's keys have gaps below the trim the twin's likelihood DIFFERS from the model's: tail * log(1 - sum
    p_j) sums over the keys, and the twin has them all.  The influence is the twin's.  The twin
    is the caller's to close."""
    from .batch import HistogramBatch
    from .bootstrap import _replicate_model
    estimate = [float(v) for v in estimate]
    if len(estimate) != len(model.params):
        raise ValueError("score_rows: %d parameters expected, %d given" % (len(model.params), len(estimate)))
    top = int(max(model.hist))
    keys = np.arange(1, top + 1, dtype=np.int64)
    counts = np.array([model.hist.get(int(j), 0) for j in keys], dtype=np.float64)
    has_tail = model.tail != 0
    twin = _replicate_model(model, keys, counts, model.tail)
    try:
        batch = HistogramBatch(twin, counts[None, :], [float(model.tail)])
        try:
            _, score, tail = batch.score_table([estimate])
        finally:
            batch.close()
    except Exception:
        twin.close()
        raise
    P = len(estimate)
    table = np.zeros((top + 1 + (1 if has_tail else 0), P), dtype=np.float64)
    table[1:top + 1] = score[0].T
    if has_tail:
        table[top + 1] = tail[0, 1:]
    return twin, table


def _moment_arrays(q):
    return np.zeros(q, dtype=np.float64), np.zeros(q * (q + 1) // 2, dtype=np.float64)


def _check_q(q):
    if not 1 <= q <= MAX_MOMENT_COLUMNS:
        raise ValueError("rows_moments: 1 .. %d columns" % MAX_MOMENT_COLUMNS)


def rows_moments(rows, centre=None):
    """(sum (q,), cross (q (q + 1) / 2,)) of an (n, q) float64 array about `centre` (zeros when None), 1 <= q <= 9, on
    the device (covest_rows_moments): sum[k] = sum_r (rows[r, k] - centre[k]), cross[batch.pair_index(q, k, l)] =
    sum_r (rows[r, k] - centre[k]) (rows[r, l] - centre[l]) for k <= l.  The shape of the reduction is a function of n
    alone and no atomic is used: the same input gives the same bits on every run."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
    if rows.ndim != 2:
        raise ValueError("rows_moments: rows must be an (n, q) array")
    n, q = rows.shape
    _check_q(q)
    centre = np.zeros(q, dtype=np.float64) if centre is None else np.ascontiguousarray(np.asarray(centre, dtype=np.float64))
    if centre.shape != (q,):
        raise ValueError("rows_moments: one centre per column")
    total, cross = _moment_arrays(q)
    _capi.check(_capi.lib().covest_rows_moments(
        ctypes.c_void_p(rows.ctypes.data if n else 0), n, q, ctypes.c_void_p(centre.ctypes.data),
        ctypes.c_void_p(total.ctypes.data), ctypes.c_void_p(cross.ctypes.data)), "covest_rows_moments")
    return total, cross


def rows_moments_device(d_rows_ptr, n, q, d_centre_ptr, d_sum_ptr, d_cross_ptr, stream=None):
    """rows_moments on device arrays (raw pointers, on the calling thread's current device; covest_rows_moments_device):
    asynchronous on `stream`."""
    _check_q(int(q))
    if int(n) < 0:
        raise ValueError("rows_moments_device: n must not be negative")
    _capi.require_shared_runtime("rows_moments_device")
    _capi.check(_capi.lib().covest_rows_moments_device(
        ctypes.c_void_p(d_rows_ptr or 0), int(n), int(q), ctypes.c_void_p(d_centre_ptr or 0), ctypes.c_void_p(d_sum_ptr or 0),
        ctypes.c_void_p(d_cross_ptr or 0), ctypes.c_void_p(stream or 0)), "covest_rows_moments_device")


def unpack_cross(cross, q):
    """The packed upper triangle of rows_moments as the symmetric (q, q) matrix."""
    cross = np.asarray(cross, dtype=np.float64).reshape(-1)
    if cross.size != q * (q + 1) // 2:
        raise ValueError("unpack_cross: %d entries expected for %d columns" % (q * (q + 1) // 2, q))
    at = np.array([[pair_index(q, min(a, b), max(a, b)) for b in range(q)] for a in range(q)])
    return cross[at]


def influence_map(info, occurrences_full, correct_c):
    """(M (P + 1, P + 1), free): the linear map from a row u_r = (Delta_r, W_r) to the shifts of summarize_jackknife's
    quantities when read r is deleted, in the order names + ['genome_size'] -- summarize_influence states them.  `free`
    are info['free']; rows of parameters that are not free are zero.  info['covariance'] must not be None."""
    P = len(info['params'])
    free = list(info['free'])
    inverse = np.zeros((P, P), dtype=np.float64)
    inverse[np.ix_(free, free)] = np.asarray(info['covariance'], dtype=np.float64)
    c = float(info['estimate'][0])
    N = float(occurrences_full)
    M = np.zeros((P + 1, P + 1), dtype=np.float64)
    M[:P, :P] = inverse
    if 0 in free:
        M[0, P] = c / N
        M[P] = -(N / correct_c(c)) / c * M[0]
    return M, free


def summarize_influence(sum, cross, n, info, occurrences_full, names, fix, level, correct_c):
    """The linearised delete-one jackknife's arithmetic on arrays (pure numpy).  `sum` (P + 1,): the column sums of
    the n rows u_r = (Delta_r, W_r) of KmerCounts.read_influence; `cross`: their cross-moments CENTRED at the mean
    sum / n, the packed upper triangle of rows_moments; `info`: observed_information's dict at the estimate;
    `occurrences_full` N = sum i h_i of the read set; `names` the P parameter names (the coverage first); `fix` None or P
    entries (None: free); `correct_c` the model's map from coverage to k-mer coverage.

    With delta_r = A_free^-1 Delta_r (zero for parameters that are not free: fixed, on a bound or not identified --
    info['free']), the quantities of jackknife.summarize_jackknife to first order, as SHIFTS when read r is deleted:
    every parameter but the first, delta_r[d]; the coverage rescaled to the full set, kappa_r = delta_r[0] + c W_r / N;
    'genome_size', -S kappa_r / c with S = N / correct_c(c).  All are linear in the P + 1 columns, shift_r = M u_r, so
    the delete-one jackknife covariance is V = (n - 1) / n M C M^T with C the centred cross-moments.

    Returns `standard_errors` (sqrt of V's diagonal), `intervals` (estimate -+ the normal quantile of `level` times the
    standard error; S for the genome size), `mean_shift` (M sum / n) per parameter name and 'genome_size' -- None for a
    parameter that is not free, the genome size going with the coverage --, `covariance` (V, (P + 1) x (P + 1) lists in the
    order `quantities` = names + ['genome_size'], zero rows where not free), `reads` = n, `level`, `free`, `reason`.
    Where info['covariance'] is None every entry is None and `reason` is info's; with fewer than two reads likewise."""
    from .information import _z
    z = _z(level)
    names = list(names)
    P = len(names)
    n = int(n)
    total = np.asarray(sum, dtype=np.float64).reshape(-1)
    if total.size != P + 1 or list(info['params']) != names:
        raise ValueError("summarize_influence: P + 1 column sums, and the information of the same parameters")
    C = unpack_cross(cross, P + 1)
    fix = [None] * P if fix is None else list(fix)
    if len(fix) != P:
        raise ValueError("summarize_influence: fix needs one entry per parameter")
    if n < 0:
        raise ValueError("summarize_influence: n must not be negative")
    quantities = names + ['genome_size']
    out = {'standard_errors': {q: None for q in quantities}, 'intervals': {q: None for q in quantities},
           'mean_shift': {q: None for q in quantities}, 'covariance': None, 'quantities': quantities, 'reads': n,
           'level': float(level), 'free': list(info['free']), 'reason': None}
    if info['covariance'] is None:
        out['reason'] = info['reason'] if info['reason'] is not None else "no covariance of the model to start from"
        return out
    if n < 2:
        out['reason'] = "a jackknife needs at least two reads"
        return out
    M, free = influence_map(info, occurrences_full, correct_c)
    V = (n - 1) / n * (M @ C @ M.T)
    shift = M @ (total / n)
    out['covariance'] = V.tolist()
    c = float(info['estimate'][0])
    centres = [float(v) for v in info['estimate']] + [float(occurrences_full) / correct_c(c)]
    for d, name in enumerate(quantities):
        of = 0 if d == P else d
        if of not in free or fix[of] is not None or not V[d, d] >= 0.0:
            continue
        se = math.sqrt(V[d, d])
        out['standard_errors'][name] = se
        out['intervals'][name] = [centres[d] - z * se, centres[d] + z * se]
        out['mean_shift'][name] = float(shift[d])
    return out


class ReadInfluence:
    """What read_influence returns.  `rows` (n, P + 1): Delta_r and the windows W_r of every read; `gradient`: the
    twin's at the estimate (P,); `info`: observed_information(twin, estimate, fix); `occurrences_full`: sum i h_i of the
    counter's histogram; `params`, `estimate`, `fix`, `level`; `table`: score_rows' table."""

    def __init__(self, rows, gradient, info, occurrences_full, params, estimate, fix, level, correct_c, table):
        self.rows = rows
        self.gradient = gradient
        self.info = info
        self.occurrences_full = int(occurrences_full)
        self.params = list(params)
        self.estimate = list(estimate)
        self.fix = fix
        self.level = float(level)
        self.correct_c = correct_c
        self.table = table

    @property
    def n_reads(self):
        return self.rows.shape[0]

    def moments(self):
        """(sum about 0, cross about the mean sum / n) of the rows: two calls of the moments kernel."""
        n = self.n_reads
        total, _ = rows_moments(self.rows)
        _, cross = rows_moments(self.rows, total / n if n else None)
        return total, cross

    def shifts(self):
        """(n, P + 1): the first-order shift of every quantity (params + ['genome_size']) when each read alone is
        deleted, rows @ influence_map^T on the host; None where the information has no covariance."""
        if self.info['covariance'] is None:
            return None
        M, _ = influence_map(self.info, self.occurrences_full, self.correct_c)
        return self.rows @ M.T

    def summary(self):
        """summarize_influence of the rows' moments."""
        total, cross = self.moments()
        return summarize_influence(total, cross, self.n_reads, self.info, self.occurrences_full, self.params, self.fix,
                                   self.level, self.correct_c)


def read_influence(model, estimate, counts, reads, fix=None, level=0.95):
    """The delete-one-read influence of `reads` on `model` at `estimate` -> ReadInfluence.  `counts`: the KmerCounts that
    holds the k-mers of exactly these reads (k = model.k <= 31; the counter's own `canonical`); `reads`: what
    KmerCounts.lookup takes; the model's histogram is that of `counts`, cut as the model was.

    score_rows gives the twin and the table of g; KmerCounts.read_influence the rows; the gradient and the observed
    information are the twin's.  The module's docstring says what the numbers claim.

    A sample factor other than 1 raises ValueError: sample_histogram rounds at random, so the histogram would not be a
    function of the reads."""
    # (a level that is no int or float is refused here as NaN is: the jackknife's rule takes any number)
    estimate, names = check_refit_request("read_influence", model, estimate, fix=fix, sample_factor=1,
                                          level=level if isinstance(level, (int, float)) else math.nan)
    if int(counts.k) != int(model.k):
        raise ValueError("read_influence: the counter's k (%d) is not the model's (%d)" % (counts.k, model.k))
    from .batch import HistogramBatch
    from .information import observed_information
    from .kmer_hist import _packed_reads
    packed = _packed_reads(reads)
    twin, table = score_rows(model, estimate)
    batch = None
    try:
        keys = list(twin.hist.keys())
        batch = HistogramBatch(twin, np.array([[twin.hist[j] for j in keys]], dtype=np.float64), [float(twin.tail)])
        _, grad = batch.loglikelihood_gradient_cross([estimate])
        info = observed_information(twin, estimate, fix)
    finally:
        if batch is not None:
            batch.close()
        twin.close()
    rows = counts.read_influence(packed, table)
    occurrences = sum(i * int(v) for i, v in enumerate(counts.histogram()))
    return ReadInfluence(rows, np.ascontiguousarray(grad[0, 0]), info, occurrences, names, estimate, fix, level,
                         model.correct_c, table)
