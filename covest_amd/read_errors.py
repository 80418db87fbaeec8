"""Which reads carry errors, and where: the k-mers of every read looked up against the counter's table and judged by
the fitted mixture's posterior classes.

    post = posterior_classes(model, estimate)
    scores = read_error_scores(model, estimate, counts, reads)
    scores.flagged            # reads with a k-mer below the posterior's error cutoff
    scores.locate_single_errors()
    fixed = correct_reads(model, estimate, counts, reads)
    fixed.strings()           # the reads with their isolated substitutions corrected (section 6af)

The lookup is the device's (KmerCounts.lookup: csrc/kmer_lookup.hip); everything here is plain numpy on what it
returns.  A flag is a statement about a READ under the model's assumption that k-mers are independent draws of the
mixture (the caveat of section 6ab): a weak k-mer is one whose abundance is more likely an erroneous k-mer's than a
genomic one's, nothing is said about its sequence.
"""
import numpy as np

from .kmer_hist import CorrectedReads
from .posterior import posterior_classes

KINDS = ("erroneous", "log_error_free")


def abundance_weights(posterior, kind="erroneous"):
    """A table over the abundances 0 .. max key of `posterior` (a PosteriorClasses) for KmerCounts.lookup's `weights`:
    the erroneous share of a k-mer of that abundance ("erroneous": the score of a read is then its expected number of
    erroneous k-mers) or the log of its error-free share ("log_error_free").  An abundance that is not a key takes the
    value at the nearest key below it, one below the smallest key the smallest key's; abundances above the largest key
    clip to it in the lookup itself (min(a, n_weights - 1): the tail is genomic)."""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s" % (KINDS,))
    keys = np.asarray(posterior.keys, dtype=np.int64)
    if keys.size < 1 or keys.min() < 0:
        raise ValueError("the posterior has no keys, or a negative one")
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    if kind == "erroneous":
        values = np.asarray(posterior.erroneous, dtype=np.float64)[order]
    else:
        with np.errstate(divide="ignore"):
            values = np.log(np.asarray(posterior.error_free, dtype=np.float64)[order])
    at = np.searchsorted(keys, np.arange(int(keys[-1]) + 1), side="right") - 1  # the nearest key at or below
    return np.ascontiguousarray(values[np.maximum(at, 0)])


class ReadErrorScores:
    """What read_error_scores returns.  Per read (int64, -1 for "none"): `min_abundance`, `weak`, `first_weak`,
    `last_weak` (KmerCounts.lookup's summary at `cutoff`); `expected_erroneous_kmers` (float64: the sum of the
    erroneous shares of the read's k-mers); `flagged` = weak > 0; `lengths`, `k`, `cutoff`, `level`.
    `flagged_share`: the share of reads that are flagged.  `predicted_share` = 1 - (1 - e)^(mean read length): the
    MODEL's share of reads with a wrong base at the fitted error rate e -- not the detector's expectation.  The two
    differ: genomic k-mers below the cutoff raise the flagged share, and errors whose k-mers reach the cutoff (a
    substitution that makes another genomic k-mer, or one seen often enough) lower it."""

    def __init__(self, k, lengths, min_abundance, weak, first_weak, last_weak, expected_erroneous_kmers, cutoff, level,
                 error_rate, weights=None):
        self.k = int(k)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.min_abundance = np.asarray(min_abundance, dtype=np.int64)
        self.weak = np.asarray(weak, dtype=np.int64)
        self.first_weak = np.asarray(first_weak, dtype=np.int64)
        self.last_weak = np.asarray(last_weak, dtype=np.int64)
        self.expected_erroneous_kmers = expected_erroneous_kmers
        self.cutoff = int(cutoff)
        self.level = None if level is None else float(level)
        self.error_rate = None if error_rate is None else float(error_rate)
        self.weights = weights  # the table the scores were summed from (abundance_weights), where one was built
        self.flagged = self.weak > 0

    @property
    def n_reads(self):
        return int(self.weak.size)

    @property
    def flagged_share(self):
        return float(self.flagged.mean()) if self.n_reads else float("nan")

    @property
    def predicted_share(self):
        if self.error_rate is None or not self.n_reads:
            return float("nan")
        return float(1.0 - (1.0 - self.error_rate) ** float(self.lengths.mean()))

    def locate_single_errors(self):
        """Per read the base position of its one error, or -1.  A single wrong base at position p makes the windows
        max(0, p - k + 1) .. min(p, last window) weak: one contiguous run [f, l] of at most k windows.  For such reads
        (weak == l - f + 1 <= k) the position is f + k - 1 if f > 0, else l if l < the last window, else -1 (the run
        covers the whole read: undecided); -1 for every other read.  From the summary alone."""
        f, l, weak = self.first_weak, self.last_weak, self.weak
        last_window = self.lengths - self.k
        run = (weak > 0) & (weak == l - f + 1) & (weak <= self.k)
        out = np.full(self.n_reads, -1, dtype=np.int64)
        inner = run & (f > 0)
        out[inner] = f[inner] + self.k - 1
        head = run & (f == 0) & (l < last_window)
        out[head] = l[head]
        return out


def read_error_scores(model, estimate, counts, reads, level=0.5, cutoff=None):
    """The reads' k-mers against `counts` (a KmerCounts that holds them, k = model.k) judged by the posterior classes
    of `model` at `estimate` -> ReadErrorScores.  `cutoff` defaults to posterior_classes(model, estimate)
    .error_cutoff(level): the abundance from which on a k-mer is more likely genomic than erroneous; ValueError where
    the posterior gives none.  The weights of the score are the erroneous shares (abundance_weights).  The table holds
    the abundances of the whole read set, so `model` must have been fitted to their histogram at sample factor 1
    (process_histogram(..., sample_factor=1)): a cutoff of a down-sampled histogram does not apply to them."""
    posterior = posterior_classes(model, estimate)
    if cutoff is None:
        cutoff = posterior.error_cutoff(level)
        if cutoff is None:
            raise ValueError("the posterior classes give no error cutoff at level %g" % level)
    weights = abundance_weights(posterior, "erroneous")
    found = counts.lookup(reads, cutoff=int(cutoff), weights=weights, per_window=False)
    return ReadErrorScores(counts.k, np.diff(found.offsets), found.min_abundance, found.weak, found.first_weak,
                           found.last_weak, found.score, cutoff, level, estimate[1], weights=weights)


class ReadCorrections(CorrectedReads):
    """What correct_reads returns: the CorrectedReads of KmerCounts.correct (`bases`, `offsets`, `runs`, `corrected`,
    `ambiguous`, `unfixable`, `changed`, `strings()`, `k`, `cutoff`) and `level`.  `corrected_share`: the share of
    reads that had runs of weak windows, all of them corrected; `unresolved_share`: the share of reads that keep a run
    (ambiguous or unfixable)."""

    def __init__(self, found, level):
        super().__init__(found.k, found.bases, found.offsets, found.fix, found.changed, found.cutoff)
        self.level = None if level is None else float(level)

    @property
    def corrected_share(self):
        return float(((self.runs > 0) & (self.corrected == self.runs)).mean()) if self.n_reads else float("nan")

    @property
    def unresolved_share(self):
        return float((self.corrected < self.runs).mean()) if self.n_reads else float("nan")


def correct_reads(model, estimate, counts, reads, level=0.5, cutoff=None):
    """The isolated substitutions of `reads` corrected from `counts` (a KmerCounts that holds them, k = model.k) at the
    posterior's error cutoff -> ReadCorrections.  `cutoff` defaults to posterior_classes(model, estimate)
    .error_cutoff(level), as in read_error_scores; ValueError where the posterior gives none.  The same caveat holds:
    the table holds the abundances of the whole read set, so `model` must have been fitted to their histogram at sample
    factor 1.  Only isolated substitutions are corrected (KmerCounts.correct); the table is not changed, so a second
    pass needs a recount of the corrected reads."""
    if cutoff is None:
        cutoff = posterior_classes(model, estimate).error_cutoff(level)
        if cutoff is None:
            raise ValueError("the posterior classes give no error cutoff at level %g" % level)
    return ReadCorrections(counts.correct(reads, int(cutoff)), level)
