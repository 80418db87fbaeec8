"""What the fitted mixture says about the k-mers of each abundance.

At abundance j a distinct k-mer carries s wrong bases with probability E_s(j) and has o copies in the genome with
probability C_o(j): the terms of the sum compute_probabilities adds up (covest/models.py:92-97, :235-241), each over the
total.  The device forms them in logs throughout (covest_posterior_classes, csrc/posterior.hip), so they exist where
p_j itself is below the doubles' range.  `posterior_classes` wraps one point's arrays; everything derived from them
here -- the error cutoff, the expected counts -- is plain numpy on those arrays.

They are shares per DISTINCT k-mer of the histogram the model was fitted to, under the model's assumption that k-mers
are independent draws of the mixture: the cutoff says from which abundance on a k-mer is more likely genomic than
erroneous; it says nothing about a particular k-mer's sequence.
"""
import numpy as np


class PosteriorClasses:
    """One point's posterior classes: keys[K], counts[K] (the histogram's n_j), log_p[K], error_share[K, S] (column s:
    s wrong bases), copy_share[K, Cc] (column c: c + 1 copies; the last column Cc copies or more), mean_copies[K]."""

    def __init__(self, keys, counts, log_p, error_share, copy_share, mean_copies):
        self.keys = np.asarray(keys)
        self.counts = np.asarray(counts, dtype=np.float64)
        self.log_p = np.asarray(log_p, dtype=np.float64)
        self.error_share = np.asarray(error_share, dtype=np.float64)
        self.copy_share = np.asarray(copy_share, dtype=np.float64)
        self.mean_copies = np.asarray(mean_copies, dtype=np.float64)
        K = len(self.keys)
        if self.error_share.ndim != 2 or self.copy_share.ndim != 2 or self.copy_share.shape[1] < 1:
            raise ValueError('error_share and copy_share: one row per key')
        for a in (self.counts, self.log_p, self.error_share, self.copy_share, self.mean_copies):
            if len(a) != K:
                raise ValueError('one entry per key in every array')

    @property
    def error_free(self):
        """Share of the k-mers of each key without a wrong base: E_0."""
        return self.error_share[:, 0]

    @property
    def erroneous(self):
        """Share of the k-mers of each key with at least one wrong base: E_1 + E_2 + ..., summed -- never 1 - E_0, which
        loses every share below 1e-16."""
        return self.error_share[:, 1:].sum(axis=1)

    def error_cutoff(self, level=0.5):
        """The smallest key j* such that the erroneous share is below `level` at EVERY key >= j* (keys in ascending
        order; a NaN share counts as not below).  None where even the largest key fails.  This is not the first
        crossing: the curve need not be monotone, and a key below j* may well be below `level` too."""
        order = np.argsort(self.keys, kind='stable')
        below = self.erroneous[order] < level  # (NaN compares False)
        if not len(below) or not below[-1]:
            return None
        failing = np.flatnonzero(~below)
        first = 0 if not len(failing) else failing[-1] + 1
        return int(self.keys[order][first])

    def expected_kmers(self):
        """Expected numbers of distinct k-mers of the histogram by class: {'erroneous', 'error_free', 'copies_1', ...,
        'copies_ge_<Cc>', 'undefined'}, each the sum over the keys of n_j times the share; keys whose shares are NaN
        (no posterior exists there) are left out of every sum and their n_j counted in 'undefined'."""
        bad = (np.isnan(self.error_share).any(axis=1) | np.isnan(self.copy_share).any(axis=1))
        ok = ~bad
        n = self.counts[ok]
        out = {'erroneous': float(np.dot(n, self.erroneous[ok])),
               'error_free': float(np.dot(n, self.error_free[ok]))}
        Cc = self.copy_share.shape[1]
        for c in range(Cc):
            name = 'copies_%d' % (c + 1) if c < Cc - 1 else 'copies_ge_%d' % Cc
            out[name] = float(np.dot(n, self.copy_share[ok, c]))
        out['undefined'] = float(self.counts[bad].sum())
        return out


def posterior_classes(model, estimate, copy_columns=4, clamp=True):
    """The posterior classes of `model` at `estimate` (param_count values) -> PosteriorClasses over the model's keys, in
    the order of model.hist.  ValueError, before the library is asked, for copy_columns < 1 or an estimate of the wrong
    length."""
    copy_columns = int(copy_columns)
    if copy_columns < 1:
        raise ValueError('copy_columns must be at least 1')
    estimate = [float(v) for v in estimate]
    if len(estimate) != model.param_count:
        raise ValueError('estimate: %d values for a model of %d parameters' % (len(estimate), model.param_count))
    log_p, err, cop, mean = model.posterior_classes_points(np.asarray([estimate]), copy_columns=copy_columns, clamp=clamp)
    hist = model.hist
    return PosteriorClasses(np.fromiter(hist.keys(), dtype=np.int64, count=len(hist)),
                            np.fromiter(hist.values(), dtype=np.float64, count=len(hist)),
                            log_p[0], err[0], cop[0], mean[0])
