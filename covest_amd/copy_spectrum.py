"""What the k-mers of each abundance ARE, where the genome is known: the matrix N[a][o] of
distinct k-mers seen a times in the reads and o times in the genome, from the join of the two counters' tables on the
device (KmerCounts.join_histogram, covest_kmer_join_histogram).  It is the empirical counterpart of the posterior
classes (covest_amd.posterior): column 0 holds the erroneous k-mers, row 0 the genomic k-mers that no read
covers, the rest, row by row, the copy shares.  Everything derived from the matrix here is plain numpy.

    counts = KmerCounts(k).add_reads(reads)
    truth = simulate.genome_counts(genome, k)
    spectrum = copy_spectrum(counts, truth)
    spectrum.compare(posterior_classes(model, estimate))

The comparison holds only where the model was fitted to the histogram of THOSE counts, with no sample_factor: the
posterior's shares are per distinct k-mer of the histogram it was fitted to.
"""
import numpy as np

MAX_CELLS = 1 << 22  # n_rows * n_cols of covest_kmer_join_histogram


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den > 0)
    return out


def _copy_names(copy_columns):
    return ['copies_%d' % (c + 1) if c < copy_columns - 1 else 'copies_ge_%d' % copy_columns for c in range(copy_columns)]


class CopySpectrum:
    """matrix[a][o]: distinct k-mers seen a times in the reads and o times in the genome (int64, at least one row and one
    column).  Where the join was clipped the last row (column) holds every abundance (copy number)
    from its index on, and everything below treats it as that index."""

    def __init__(self, matrix):
        self.matrix = np.asarray(matrix, dtype=np.int64)
        if self.matrix.ndim != 2 or self.matrix.shape[0] < 1 or self.matrix.shape[1] < 1:
            raise ValueError('the matrix has a row per abundance and a column per copy number, at least one of each')

    def abundance_histogram(self):
        """The reads' count-of-counts, indexed by abundance: the row sums for a >= 1, 0 at index 0 (as
        KmerCounts.histogram)."""
        out = self.matrix.sum(axis=1)
        out[0] = 0
        return out

    def genome_spectrum(self):
        """{o: distinct k-mers with o copies in the genome}, o >= 1: the column sums, as simulate.genome_spectrum."""
        sums = self.matrix.sum(axis=0)
        return {o: int(v) for o, v in enumerate(sums.tolist()) if o > 0 and v > 0}

    def unseen(self):
        """Row 0 by copy number: the genomic k-mers no read holds (index 0 is 0)."""
        return self.matrix[0].copy()

    def error_share(self):
        """Per abundance a >= 1 the share of its k-mers that are not in the genome, N[a][0] / sum_o N[a][o]; NaN where
        no k-mer has that abundance, and at index 0."""
        out = _ratio(self.matrix[:, 0], self.matrix.sum(axis=1))
        out[0] = np.nan
        return out

    def _copy_counts(self, copy_columns):
        """[a][c]: genomic k-mers of abundance a with c + 1 copies, the last column copy_columns copies or more."""
        copy_columns = int(copy_columns)
        if copy_columns < 1:
            raise ValueError('copy_columns must be at least 1')
        genomic = self.matrix[:, 1:]
        out = np.zeros((self.matrix.shape[0], copy_columns), dtype=np.int64)
        head = min(copy_columns - 1, genomic.shape[1])
        out[:, :head] = genomic[:, :head]
        out[:, copy_columns - 1] = genomic[:, copy_columns - 1:].sum(axis=1)
        return out

    def copy_share(self, copy_columns=4):
        """Among the GENOMIC k-mers (o >= 1) of each abundance the share with 1, 2, ... copies: (abundances,
        copy_columns), columns as PosteriorClasses.copy_share -- o = 1 .. copy_columns - 1, the last o >= copy_columns.
        NaN where no genomic k-mer has that abundance."""
        counts = self._copy_counts(copy_columns)
        return _ratio(counts, counts.sum(axis=1, keepdims=True))

    def mean_copies(self):
        """Per abundance the mean copy number of its genomic k-mers; NaN where there is none."""
        genomic = self.matrix[:, 1:]
        o = np.arange(1, self.matrix.shape[1], dtype=np.float64)
        return _ratio(genomic @ o if genomic.shape[1] else np.zeros(len(genomic)), genomic.sum(axis=1))

    def error_cutoff(self, level=0.5):
        """The rule of PosteriorClasses.error_cutoff on the measured shares: the smallest abundance a* such that the
        erroneous share is below `level` at EVERY abundance a >= a* that has k-mers.  None where even the largest
        fails, or no abundance has k-mers.  Not the first crossing: the curve need not be monotone."""
        share = self.error_share()
        keys = np.flatnonzero(~np.isnan(share))
        below = share[keys] < level
        if not len(below) or not below[-1]:
            return None
        failing = np.flatnonzero(~below)
        first = 0 if not len(failing) else failing[-1] + 1
        return int(keys[first])

    def observed_kmers(self, copy_columns=4, keys=None):
        """The dictionary of PosteriorClasses.expected_kmers with counts in place of expectations, over the k-mers the
        reads hold (a >= 1): 'erroneous' (not in the genome), 'error_free' (in it), 'copies_1' ... 'copies_ge_<Cc>'
        (the genomic ones by copy number), 'undefined' (0: every k-mer has a truth).  `keys`: only these abundances
        (those of them the matrix has a row for, each once) -- the keys of a trimmed histogram, say."""
        rows = np.arange(1, self.matrix.shape[0])
        if keys is not None:
            rows = np.intersect1d(rows, np.asarray(keys, dtype=np.int64))
        seen = self._copy_counts(copy_columns)[rows].sum(axis=0)
        out = {'erroneous': int(self.matrix[rows, 0].sum()), 'error_free': int(self.matrix[rows, 1:].sum())}
        out.update(zip(_copy_names(int(copy_columns)), (int(v) for v in seen)))
        out['undefined'] = 0
        return out

    def compare(self, posterior, min_error_free=0.99):
        """The posterior classes of a fitted model (a PosteriorClasses) beside the measurement, aligned on the
        posterior's keys -> dict:
          'keys'                  the posterior's keys
          'erroneous'             (model, measured) per key: PosteriorClasses.erroneous beside error_share(); the
                                  measured one is NaN for a key beyond the matrix or without k-mers
          'copy_keys'             the keys with the model's E_0 >= min_error_free
          'copy_share'            (model, measured) at those keys, (len(copy_keys), Cc) each.  The condition is there
                                  because the model's copy share is a marginal over ALL error classes, the measured
                                  one is of genomic k-mers only: they speak of the same k-mers only where nearly every
                                  k-mer is error-free
          'copy_expected', 'copy_observed'  the numbers of k-mers by copy number over copy_keys alone: n_j times the
                                  model's copy share, summed, beside the genomic k-mers of those abundances.  (Over ALL
                                  keys the two are not the same quantity: 'expected' below counts an erroneous k-mer
                                  under the copy number of the k-mer it was misread from, 'observed' counts genomic
                                  k-mers only.)
          'error_cutoff'          (model, measured), at level 0.5
          'expected', 'observed'  expected_kmers() and observed_kmers(Cc) over the posterior's keys (the tail of a
                                  trimmed histogram is in neither)
        It holds only where the model was fitted to the histogram of the very counts that were joined, with no
        sample_factor: the posterior's shares are per distinct k-mer of the histogram it was fitted to."""
        keys = np.asarray(posterior.keys, dtype=np.int64)
        Cc = posterior.copy_share.shape[1]
        inside = (keys >= 0) & (keys < self.matrix.shape[0])
        at = np.where(inside, keys, 0)
        measured = np.where(inside, self.error_share()[at], np.nan)
        pick = np.asarray(posterior.error_free) >= min_error_free
        measured_copies = np.where(inside[pick, None], self.copy_share(Cc)[at[pick]], np.nan)
        # ... and their totals: n_j C_c(j) summed over those keys beside the genomic k-mers of those abundances
        model_copies = posterior.copy_share[pick]
        defined = ~np.isnan(model_copies).any(axis=1)
        expected_copies = np.asarray(posterior.counts)[pick][defined] @ model_copies[defined]
        observed_copies = self._copy_counts(Cc)[np.intersect1d(keys[pick & inside], np.arange(1, self.matrix.shape[0]))].sum(axis=0)
        return {'keys': keys,
                'copy_expected': dict(zip(_copy_names(Cc), (float(v) for v in expected_copies))),
                'copy_observed': dict(zip(_copy_names(Cc), (int(v) for v in observed_copies))),
                'erroneous': (np.asarray(posterior.erroneous), measured),
                'copy_keys': keys[pick],
                'copy_share': (posterior.copy_share[pick], measured_copies),
                'error_cutoff': (posterior.error_cutoff(), self.error_cutoff()),
                'expected': posterior.expected_kmers(),
                'observed': self.observed_kmers(Cc, keys=keys)}


def copy_spectrum(counts, genome_counts, max_abundance=None, max_copies=None):
    """The CopySpectrum of `counts` (a KmerCounts of the reads) against `genome_counts` (one of the genome they came
    from: simulate.genome_counts), joined on the device.  `max_abundance`, `max_copies`: the last row, the last column,
    which take everything beyond; None: unclipped, the largest count the counter holds (its stats()).  ValueError where
    the matrix would pass 2^22 cells, naming the clip to pass."""
    def size(limit, counter, name):
        if limit is None:
            return counter.stats()[0]
        if int(limit) < 0:
            raise ValueError('%s must not be negative' % name)
        return int(limit) + 1

    rows, cols = size(max_abundance, counts, 'max_abundance'), size(max_copies, genome_counts, 'max_copies')
    if rows * cols > MAX_CELLS:
        clip, fits = (('max_abundance', MAX_CELLS // cols - 1) if max_abundance is None and (max_copies is not None or rows >= cols)
                      else ('max_copies', MAX_CELLS // rows - 1))
        raise ValueError('a matrix of %d x %d passes %d cells: pass %s (%d at most with the other side as it is)'
                         % (rows, cols, MAX_CELLS, clip, fits))
    return CopySpectrum(counts.join_histogram(genome_counts, rows, cols))
