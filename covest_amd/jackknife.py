"""The delete-a-group jackknife over READS: standard errors that see what no function of the
histogram can -- that the k-mers of one read come and go together.

    est, ok = CoverageEstimator(model).compute_coverage(guess)
    jack = read_jackknife(model, est, reads, groups=32, seed=1)
    print_output(hist_orig, model, ok, 1, estimated=est, jackknife=jack)

The reads are dealt into G seeded groups (covest_split_reads: the group of read r is a stated function of (seed, r)),
leave-out histogram g is the k-mer histogram of every read OUTSIDE group g, the G histograms and the full one are
refitted together on one HistogramBatch, and the spread of the G refits is the variance.  Whole reads are deleted, never
single k-mers: that is what lets the number speak about the dependence between overlapping k-mers.

The only device work that is new is the split (split_reads.hip): after it every group is one contiguous run of the
packed reads, and "all reads but group g" is two covest_kmer_add_device calls on sub-ranges of one buffer.  There is no
CPU path: without the library or a HIP device the calls raise CovestHipError.
"""
import math

import numpy as np

from .read_sets import (REFITS, ResidentReads, _cut, _hist_dict, _occurrences, check_refit_request, check_sets,  # noqa: F401
                        jackknife_batch, quantity_rows, refit_histogram_set)
from .sample import MAX_GROUPS, _check_split, split_reads_device


ROUTES = ("recount", "remove")
MAX_REMOVE_K = 31  # the removal takes keys of one word (covest_kmer_remove_device)


def _check_route(route, k):
    """The rule of `route` before the library is asked (ValueError): one of ROUTES, and "remove" only at k <= 31."""
    if route not in ROUTES:
        raise ValueError('route must be "recount" or "remove"')
    if route == "remove" and k > MAX_REMOVE_K:
        raise ValueError('route="remove" takes k <= %d (keys of one word); use route="recount"' % MAX_REMOVE_K)
    return route


def leave_group_out_histograms(reads, k, groups, seed=0, canonical=False, device=-1, route="recount"):
    """(hist_full, [hist_g for g in range(groups)], occurrences) of `reads` -- a SimulatedReads, an (n, L) uint8 array
    or a pair (bases, offsets) in the packed layout --: hist_g the k-mer histogram {abundance: k-mers} of the reads
    outside group g of covest_split_reads(groups, seed), hist_full that of all reads, occurrences[g] = sum i hist_g[i].

    The reads go up once and are split once on the device; each histogram comes from ONE KmerCounts whose table is
    reserved once for the whole set: clear, add_device on the ranks before the group, add_device on the ranks behind it,
    histogram.  The sub-ranges address the same buffer (ragged reads: offsets + first; reads of one length: bases + first
    * read_len).  The buffers live on the calling thread's current device, which `device` has to name (or -1).  Reads
    that do not fit the device together with their copy raise CovestHipError; streaming a file in passes is not built.

    `route`: "recount" is the loop above, G + 1 counts of the read set.  "remove" (k <= 31) counts all
    reads ONCE and, per group, takes the ranks of group g out of the table again (ResidentReads.uncount), takes the
    histogram and counts them back in: about three counts' worth of atomics in all and no clear of the table per group.
    The histograms are exact integers either way: the two routes return the same dicts, and after the loop the counter
    holds all reads again."""
    return _leave_group_out(reads, k, groups, seed, canonical, device, route)[:3]


def _leave_group_out(reads, k, groups, seed, canonical, device, route="recount"):
    """leave_group_out_histograms, and the split's group_first behind its three results."""
    groups = check_sets("groups", groups, "jackknife", MAX_GROUPS, MAX_GROUPS)
    groups, seed, _ = _check_split(groups, seed, 0)
    _check_route(route, k)
    with ResidentReads(reads, k, canonical, device, "leave_group_out_histograms", "their copy in group order") as rs:
        d_out = rs.reserve("out", rs.n_bases)
        d_out_off = rs.reserve("out_offsets", 8 * (rs.n + 1)) if rs.offsets is not None else None
        d_first = rs.reserve("group_first", 8 * (groups + 1))
        split_reads_device(rs.d_in, rs.n, d_out, d_first, groups, seed=seed, first_read=rs.first_read, read_len=rs.read_len,
                           offsets_ptr=rs.d_offsets, out_offsets_ptr=d_out_off, device=device)
        first = np.empty(groups + 1, dtype=np.int64)
        rs.download("group_first", first)  # (waits for the split)
        rs.open_counter()

        def add(lo, hi):  # ranks [lo, hi) of the split buffer
            if hi > lo:
                rs.count(d_out, d_out_off, lo, hi)

        add(0, rs.n)
        hist_full = rs.histogram()
        hists = []
        for g in range(groups):
            lo, hi = int(first[g]), int(first[g + 1])
            if route == "remove":
                if hi > lo:
                    rs.uncount(d_out, d_out_off, lo, hi)
                hists.append(rs.histogram())
                add(lo, hi)
            else:
                rs.clear()
                add(0, lo)
                add(hi, rs.n)
                hists.append(rs.histogram())
        return hist_full, hists, [_occurrences(h) for h in hists], first


def summarize_jackknife(estimates, success, full, occurrences, occurrences_full, names, fix, level, correct_c):
    """The delete-a-group jackknife's arithmetic on arrays (pure numpy): `estimates` (G, P) the leave-out refits, `success`
    (G,), `full` (P,) the refit of the full set, `occurrences` (G,) and `occurrences_full` the k-mer occurrences sum i h_i
    of each set, `names` the P parameter names (the coverage first), `fix` None or P entries (None: free), `correct_c` the
    model's map from coverage to k-mer coverage.

    The quantities: every parameter but the first as it is (error rate, q1, q2, q are scale-free); the coverage of
    leave-out set g rescaled to the full read set, c_g * occurrences_full / occurrences[g] -- deleting a group lowers the
    coverage by construction, what is uncertain is the genome size --; and 'genome_size' = occurrences[g] /
    correct_c(c_g), report.py's formula on the leave-out set (occurrences_full / correct_c(c_full) for the full one).
    Over the G' successful leave-out refits, per quantity theta: mean; standard_errors = sqrt((G' - 1) / G' * sum (theta_g
    - mean)^2); bias = (G' - 1) (mean - theta_full); bias_corrected = theta_full - bias; intervals = theta_full -+
    t_{G' - 1, (1 + level) / 2} * standard error.  None for a fixed parameter (the genome size goes with the coverage),
    and for everything where G' < 2.  Also `failed` = G - G' and `used` = G'."""
    used, ok, rows = quantity_rows("summarize_jackknife", estimates, success, full, occurrences, occurrences_full, names, fix,
                                   level, correct_c, "group")
    out = {'mean': {}, 'standard_errors': {}, 'bias': {}, 'bias_corrected': {}, 'intervals': {},
           'failed': int(len(ok) - used), 'used': used}
    quantile = None
    if used >= 2:
        from scipy.stats import t as student_t
        quantile = float(student_t.ppf(0.5 * (1.0 + level), used - 1))
    for name, values, theta_full, free, _ in rows:
        if not free or used < 2:
            for key in ('mean', 'standard_errors', 'bias', 'bias_corrected', 'intervals'):
                out[key][name] = None
            continue
        mean = float(values.mean())
        se = math.sqrt((used - 1) / used * float(((values - mean) ** 2).sum()))
        bias = (used - 1) * (mean - theta_full)
        out['mean'][name] = mean
        out['standard_errors'][name] = se
        out['bias'][name] = bias
        out['bias_corrected'][name] = theta_full - bias
        out['intervals'][name] = [theta_full - quantile * se, theta_full + quantile * se]
    return out


def read_jackknife(model, estimate, reads, groups=32, seed=0, fix=None, level=0.95, trim=None, refit="lockstep-gradient",
                   sample_factor=1, canonical=False, route="recount", **estimator_options):
    """The delete-a-group jackknife of `estimate` (of `model`, whose histogram is that of `reads` at k = model.k,
    `canonical` as it was counted) over `groups` seeded groups of the reads.

    WHAT THE NUMBER IS.  Its standard errors see the dependence between the k-mers of one read -- a read is deleted
    whole -- and the randomness of where the reads start.  The genome is held fixed: nothing here speaks about another
    genome of the same kind.  The groups' sizes are binomial (a read's group is drawn on its own), not equal; the
    formulas are the equal-size ones, which is the usual approximation at n / G reads a group.  The intervals are
    Student t with G' - 1 degrees of freedom, G' the leave-out refits that succeeded: G, not the number of reads,
    limits how well the variance itself is known.

    HOW.  leave_group_out_histograms gives the G + 1 histograms, by `route` ("recount", or "remove" at k <= 31: the same
    histograms, so the same estimates and standard errors bit for bit; the returned dict records a route other than the
    default as 'route', which print_output passes on as jackknife_route).  Each is cut as the model's was: keys below `trim` are
    kept and the mass at and above goes to the tail (hist_steps.trim_hist); trim=None with model.tail == 0 means no cut,
    trim=None with a tail takes max(model.hist) + 1.  The G + 1 histograms are put on ONE key set -- the model's keys and
    behind them, ascending, the keys any of the histograms has beyond those; zero counts kept -- on a twin of the model
    (bootstrap._replicate_model: class, settings, bounds, defaults): tail * log(1 - sum p_j) sums over the keys, so all
    fits must share the cells.  Rows 0 .. G - 1 of one HistogramBatch are the leave-out histograms, row G the full one;
    all are refitted together from `estimate` by bootstrap._refit_lockstep, `refit` as in parametric_bootstrap
    ("lockstep": finite differences; "lockstep-gradient": the batch's analytic gradient).

    sample_factor other than 1 raises ValueError: sample_histogram rounds at random, so a jackknife through it would not
    be a function of the reads.

    Returns summarize_jackknife's dict (mean, standard_errors, bias, bias_corrected, intervals per parameter name and
    'genome_size'; failed, used) and: estimates (G x P, as refitted: the coverage not rescaled), success (G), at_bound
    (G x P), group_sizes (reads a group), occurrences (G), occurrences_full, full_estimate (row G's refit),
    full_success, full_minus_given (its distance from `estimate`), keys_added (keys of the union the model did not
    have), params, estimate, level, groups, seed, refit."""
    groups = check_sets("groups", groups, "jackknife", MAX_GROUPS, MAX_GROUPS)
    _check_split(groups, seed, 0)
    _check_route(route, model.k)
    estimate, names = check_refit_request("read_jackknife", model, estimate, refit, estimator_options, level, fix, trim,
                                          sample_factor, REFITS)
    hist_full, hists, _, group_first = _leave_group_out(reads, model.k, groups, seed, canonical, model.device, route)
    out = {'groups': groups}
    if route != "recount":  # (the default leaves the dict as it always was)
        out['route'] = route
    out.update(refit_histogram_set(model, estimate, hists, hist_full, seed, fix, level, trim, refit, estimator_options))
    out['group_sizes'] = np.diff(group_first).tolist()
    out.update(summarize_jackknife(out['estimates'], out['success'], out['full_estimate'], out['occurrences'],
                                   out['occurrences_full'], names, fix, level, model.correct_c))
    return out
