"""A batch of histograms on ONE model's key set, scored in one pass (covest_batch_* of
include/covest_amd.h).

    batch = HistogramBatch(model, counts, tails)          # counts (B, n_keys) in the model's key order
    batch = HistogramBatch.draw(model, estimate, 256, seed=1)   # or B replicates drawn from the model, on the device
    ll = batch.loglikelihood_cross(points)                # (B, n): every histogram at every point
    ll = batch.loglikelihood_pairs(index, points)         # (n,): histogram index[i] at point i
    best, arg = batch.argmin_cross(points)                # per histogram: min -LL over the points and where
    ll, grad = batch.loglikelihood_gradient_cross(points) # (B, n), (B, n, P): value and analytic gradient
    ll, grad = batch.loglikelihood_gradient_pairs(index, points)   # (n,), (n, P)
    log_p, score, tail = batch.score_table(points)        # the table behind the two: (n, n_keys), (n, P, n_keys), (n, P + 1)
    ll, grad, hess = batch.loglikelihood_hessian_cross(points)     # (B, n), (B, n, P), (B, n, P, P): with the Hessian of LL
    ll, grad, hess = batch.loglikelihood_hessian_pairs(index, points)   # (n,), (n, P), (n, P, P)
    log_p, score, curv, tail = batch.score_table(points, order=2)  # ... and its table: curv (n, P (P + 1) / 2, n_keys)

For a fixed key set p_j(theta) does not depend on the counts, so B histograms at n points cost n evaluations of p and
one B x n_keys x n contraction instead of B n evaluations.  The per-key score d_k p_j / p_j does not depend on them
either, so the gradient costs n walks of the derivative kernel and a contraction against P + 1 rows a point (DESIGN.md
section 6u).  Nor does the curvature c_kl(j) = d_k d_l p_j / p_j - (d_k p_j / p_j)(d_l p_j / p_j) of log p_j: the Hessians
of B histograms at n points cost n walks of the derivative kernel at order 2 and a contraction against
R2 = 1 + P + P (P + 1) / 2 rows a point (section 6x) -- the observed information of every bootstrap replicate at its own
refit in one call (information.observed_information_batch).  What a batch is not: its histograms share the model's keys, k, r, comb, bounds and threshold -- only the
counts and the tail differ.  There is no CPU path: without the library or a HIP device the constructor raises
CovestHipError.
"""
import ctypes

import numpy as np

from . import _capi

INFO_FIELDS = ("points_tabled", "table_chunks", "cross_tiles", "dead_points", "fixup_waves", "pairs_requests",
               "table_ns", "contraction_ns")
MAX_HISTOGRAMS = 1 << 20  # csrc/kernels.h kBatchMaxHist


def _counts_array(counts, n_keys):
    """The argument rules of covest_batch_create, before the library is asked (ValueError)."""
    h = np.ascontiguousarray(counts, dtype=np.float64)
    if h.ndim == 1 and n_keys and h.size == n_keys:
        h = h.reshape(1, n_keys)
    if h.ndim != 2 or h.shape[1] != n_keys:
        raise ValueError("counts must be (histograms, %d): one column per key of the model" % n_keys)
    if h.shape[0] > MAX_HISTOGRAMS:
        raise ValueError("more than %d histograms" % MAX_HISTOGRAMS)
    if not np.all(np.isfinite(h)) or np.any(h < 0.0):
        raise ValueError("a count is negative, NaN or infinite")
    return h


def _tails_array(tails, n_hist):
    if tails is None:
        return np.zeros(n_hist, dtype=np.float64)
    t = np.ascontiguousarray(tails, dtype=np.float64)
    if t.shape != (n_hist,):
        raise ValueError("tails must be one per histogram")
    if not np.all(np.isfinite(t)) or np.any(t < 0.0):
        raise ValueError("a tail is negative, NaN or infinite")
    return t


def _index_array(index, n_hist):
    raw = np.asarray(index)
    if raw.size and not np.issubdtype(raw.dtype, np.integer):
        if not np.all(np.isfinite(raw)) or np.any(raw != np.floor(raw)):
            raise ValueError("a histogram index is not an integer")
    idx = np.ascontiguousarray(raw, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= n_hist):
        raise ValueError("a histogram index is outside 0 .. %d" % (n_hist - 1))
    return idx


def pair_index(P, k, l):
    """Where the packed upper triangle (k <= l, row by row) holds entry (k, l): csrc/ll_deriv.hip pair_index."""
    return k * P - k * (k - 1) // 2 + (l - k)


def _unpack_hessian(packed, P):
    """(..., P (P + 1) / 2) -> (..., P, P), mirrored on the host: bit-symmetric.  One gather: entry (k, l) and entry
    (l, k) read the same packed number."""
    at = np.array([[pair_index(P, min(k, l), max(k, l)) for l in range(P)] for k in range(P)])
    return np.ascontiguousarray(packed[..., at])


class HistogramBatch:
    """`counts` (B, n_keys) in the order of model.hist's keys, `tails` (B,) or None for zeros.  The batch borrows the
    model: model.close() closes it."""

    def __init__(self, model, counts, tails=None):
        n_keys = len(model.hist)
        h = _counts_array(counts, n_keys)
        t = _tails_array(tails, h.shape[0])
        self._fields(model, h.shape[0], n_keys)
        handle = ctypes.c_void_p()
        _capi.check(_capi.lib().covest_batch_create(model.handle, self._n, h.ctypes.data, t.ctypes.data,
                                                    ctypes.byref(handle)), "covest_batch_create")
        self._adopt(handle)

    def _fields(self, model, n_hist, n_keys):
        self.model = model
        self._n = int(n_hist)
        self._n_keys = n_keys
        self._handle = None

    def _adopt(self, handle):
        self._handle = handle
        self.model._register_batch(self)

    @classmethod
    def draw(cls, model, estimate, replicates, seed=0, first_replicate=0, n_draws=None):
        """`replicates` histograms of `n_draws` draws (default round(sum(counts) + tail) of the model's own histogram)
        from the model at `estimate`, over bootstrap.model_cells: the rows bootstrap.draw_histograms gives, bit for
        bit, drawn and kept on the device."""
        from .bootstrap import _check_draws
        estimate = [float(v) for v in estimate]
        if len(estimate) != model.param_count:
            raise ValueError("HistogramBatch.draw: %d parameters expected, %d given" % (model.param_count, len(estimate)))
        if n_draws is None:
            n_draws = int(round(float(sum(model.hist.values())) + float(model.tail)))
        n_keys = len(model.hist)
        _check_draws(n_keys + (1 if model.tail != 0 else 0), n_draws, replicates, seed, first_replicate)
        if replicates > MAX_HISTOGRAMS:
            raise ValueError("more than %d histograms" % MAX_HISTOGRAMS)
        self = cls.__new__(cls)
        self._fields(model, replicates, n_keys)
        par = np.asarray(estimate, dtype=np.float64)
        handle = ctypes.c_void_p()
        _capi.check(_capi.lib().covest_batch_draw(model.handle, par.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  int(n_draws), int(first_replicate), self._n, int(seed),
                                                  ctypes.byref(handle)), "covest_batch_draw")
        self._adopt(handle)
        return self

    def __len__(self):
        return self._n

    def _open(self):
        if self._handle is None:
            raise ValueError("the batch is closed")
        return self._handle

    def _points(self, points):
        return np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.model.param_count)

    def _requests(self, index, points):
        """A pairs call's points and its histogram numbers, one per point."""
        pts = self._points(points)
        idx = _index_array(index, self._n)
        if len(idx) != len(pts):
            raise ValueError("one histogram index per point")
        return pts, idx

    def counts(self):
        """(counts (B, n_keys), tails (B,)) as the device holds them."""
        h = np.empty((self._n, self._n_keys), dtype=np.float64)
        t = np.empty(self._n, dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_counts(self._open(), h.ctypes.data, t.ctypes.data), "covest_batch_counts")
        return h, t

    def loglikelihood_cross(self, points):
        """(B, n): the log-likelihood of every histogram at every point of an (n, param_count) array."""
        pts = self._points(points)
        out = np.empty((self._n, len(pts)), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_cross(self._open(), len(pts), pts.ctypes.data, out.ctypes.data),
                    "covest_batch_eval_cross")
        return out

    def loglikelihood_pairs(self, index, points):
        """(n,): the log-likelihood of histogram index[i] at points[i]."""
        pts, idx = self._requests(index, points)
        out = np.empty(len(pts), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_pairs(self._open(), len(pts), idx.ctypes.data, pts.ctypes.data,
                                                        out.ctypes.data), "covest_batch_eval_pairs")
        return out

    def loglikelihood_gradient_cross(self, points):
        """(ll (B, n), grad (B, n, P)): every histogram's log-likelihood and its analytic gradient at every point, at
        the point after fit_to_bounds (a component whose parameter the clamp moved is 0; where the value is not finite
        every component is NaN).  Value and gradient come from ONE table, the derivative kernel's: a line search gets a
        value and a gradient of one function.  That value agrees with loglikelihood_cross (K-direct's table) to 1e-11
        relative, not to the bit."""
        pts = self._points(points)
        out = np.empty((self._n, len(pts), self.model.param_count + 1), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_cross_grad(self._open(), len(pts), pts.ctypes.data, out.ctypes.data),
                    "covest_batch_eval_cross_grad")
        return np.ascontiguousarray(out[:, :, 0]), np.ascontiguousarray(out[:, :, 1:])

    def loglikelihood_gradient_pairs(self, index, points):
        """(ll (n,), grad (n, P)): histogram index[i] at points[i], value and analytic gradient from one table as in
        loglikelihood_gradient_cross (the value is the derivative kernel's: loglikelihood_pairs' to 1e-11 relative, not
        to the bit).  A request's result does not depend on what else is in the call."""
        pts, idx = self._requests(index, points)
        out = np.empty((len(pts), self.model.param_count + 1), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_pairs_grad(self._open(), len(pts), idx.ctypes.data, pts.ctypes.data,
                                                             out.ctypes.data), "covest_batch_eval_pairs_grad")
        return np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1:])

    def loglikelihood_hessian_cross(self, points):
        """(ll (B, n), grad (B, n, P), hess (B, n, P, P)): every histogram's log-likelihood, analytic gradient and
        closed-form Hessian -- of LL, not of -LL -- at every point, at the point after fit_to_bounds (a row and a column
        whose parameter the clamp moved are 0; where the value is not finite every other entry is NaN).  All three come
        from ONE table, the derivative kernel's at order 2; the device returns the upper triangle
        and the matrix is mirrored here, so it is symmetric to the bit."""
        pts = self._points(points)
        P = self.model.param_count
        out = np.empty((self._n, len(pts), 1 + P + P * (P + 1) // 2), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_cross_hess(self._open(), len(pts), pts.ctypes.data, out.ctypes.data),
                    "covest_batch_eval_cross_hess")
        return np.ascontiguousarray(out[:, :, 0]), np.ascontiguousarray(out[:, :, 1:1 + P]), _unpack_hessian(out[:, :, 1 + P:], P)

    def loglikelihood_hessian_pairs(self, index, points):
        """(ll (n,), grad (n, P), hess (n, P, P)): histogram index[i] at points[i], as loglikelihood_hessian_cross.  A
        request's result does not depend on what else is in the call."""
        pts, idx = self._requests(index, points)
        P = self.model.param_count
        out = np.empty((len(pts), 1 + P + P * (P + 1) // 2), dtype=np.float64)
        _capi.check(_capi.lib().covest_batch_eval_pairs_hess(self._open(), len(pts), idx.ctypes.data, pts.ctypes.data,
                                                             out.ctypes.data), "covest_batch_eval_pairs_hess")
        return np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1:1 + P]), _unpack_hessian(out[:, 1 + P:], P)

    def score_table(self, points, order=1):
        """(log_p (n, n_keys), score (n, P, n_keys), tail (n, P + 1)): the table the gradient methods contract with, as
        the device holds it.  log_p is +0.0 where p_ij <= 0 and nowhere else (p = 1 is -0.0; NaN stays NaN);
        score[i, k, j] = d_k p_ij / p_ij, +0.0 at such a key and throughout where the clamp moved parameter k;
        tail[i] = [log(1 - sp_i), -S_k / (1 - sp_i) ...], all 0 where sp_i is not < 1.  It does not depend on the
        histograms.

        order=2: (log_p, score, curv (n, P (P + 1) / 2, n_keys), tail (n, R2)), the Hessian methods' table --
        curv[i, pair_index(P, k, l), j] = d_k d_l p_ij / p_ij - score_k score_l for k <= l, +0.0 at a dead key and
        throughout where the clamp moved k or l; tail[i] continues with -(S_kl / (1 - sp_i) + S_k S_l / (1 - sp_i)^2)."""
        if order not in (1, 2):
            raise ValueError("score_table: order must be 1 or 2")
        pts = self._points(points)
        P = self.model.param_count
        R = P + 1 if order == 1 else 1 + P + P * (P + 1) // 2
        rows = np.empty((len(pts), R, self._n_keys), dtype=np.float64)
        tail = np.empty((len(pts), R), dtype=np.float64)
        name = "covest_batch_score_table" if order == 1 else "covest_batch_score_table2"
        _capi.check(getattr(_capi.lib(), name)(self._open(), len(pts), pts.ctypes.data, rows.ctypes.data, tail.ctypes.data), name)
        if order == 1:
            return np.ascontiguousarray(rows[:, 0, :]), np.ascontiguousarray(rows[:, 1:, :]), tail
        return (np.ascontiguousarray(rows[:, 0, :]), np.ascontiguousarray(rows[:, 1:1 + P, :]),
                np.ascontiguousarray(rows[:, 1 + P:, :]), tail)

    def argmin_cross(self, points):
        """(min_negll (B,), arg (B,)): per histogram the smallest -LL over the points and the first index that attains
        it (NaN never wins); (inf, -1) where no value is below +inf."""
        pts = self._points(points)
        best = np.full(self._n, np.inf, dtype=np.float64)
        arg = np.full(self._n, -1, dtype=np.int64)
        _capi.check(_capi.lib().covest_batch_argmin_cross(self._open(), len(pts), pts.ctypes.data, best.ctypes.data,
                                                          arg.ctypes.data), "covest_batch_argmin_cross")
        return best, arg

    def info(self):
        """Counters of the last evaluation (covest_batch_info): a dict over INFO_FIELDS."""
        out = np.zeros(8, dtype=np.int64)
        _capi.check(_capi.lib().covest_batch_info(self._open(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
                    "covest_batch_info")
        return dict(zip(INFO_FIELDS, (int(v) for v in out)))

    def close(self):
        if getattr(self, "_handle", None) is not None:
            _capi.lib().covest_batch_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
