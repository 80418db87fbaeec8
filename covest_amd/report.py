"""The step after the path: the result record of one estimate, field for field
what covest/data.py:106-173 print_output builds -- three likelihood evaluations (GPU, through the
model's compute_loglikelihood) and the genome size

    genome_size = round( sum_i i * h_i  /  correct_c(c * sample_factor) )        (covest/data.py:152-156)

The record is returned and, unless `silent`, printed as block-style YAML like the reference's output.
"""
import yaml

from . import __version__


def _none_filled(values, fallback):
    """`values` with its None entries taken from `fallback` (covest/data.py:94-103)."""
    if values is None or fallback is None:
        raise ValueError('Invalid arguments.')
    if len(values) != len(fallback):
        raise ValueError('Length of arguments should be equal.')
    return [f if v is None else v for v, f in zip(values, fallback)]


def _finite_int(x):
    return None if x == float('inf') else int(x)


def print_output(hist_orig, model, success, sample_factor, estimated=None, guess=None, orig=None,
                 reads_size=None, silent=False, orig_sample_factor=1, starting_points=1,
                 use_grid_search=False, intervals=None, information=None, bootstrap=None, jackknife=None,
                 posterior=None, read_errors=None, corrections=None, read_influence=None, read_bootstrap=None,
                 duplicates=None, copy_spectrum=None):
    """`intervals`: the dict covest_amd.profile.coverage_interval returns; the record then carries the likelihood-ratio
    interval of the coverage, of the genome size and its level.  Without it the record is the reference's, key for key.
    `information`: the dict covest_amd.information.observed_information returns (a key 'level' in it chooses the Wald
    level, 0.95 otherwise); the record then carries standard_errors, wald_intervals, genome_size_se,
    genome_size_wald_interval and wald_level, the coverage's in the units of the record's `coverage` (times
    sample_factor).  They are the MODEL's standard errors: it treats the k-mer counts as independent and |LL| is
    1e7..1e8, so they are very small.  Without it the record is unchanged.  When the dict is
    covest_amd.information.sandwich_covariance's (it carries 'robust_standard_errors') the record adds
    robust_standard_errors, robust_wald_intervals and genome_size_robust_se, scaled like their neighbours: corrected
    for misfit of the mixture, NOT for dependence between overlapping k-mers; otherwise it does not.
    `bootstrap`: the dict covest_amd.bootstrap.parametric_bootstrap returns; the record then carries
    bootstrap_replicates, bootstrap_failed and, per free parameter, bootstrap_bias_<param>, bootstrap_se_<param> and
    bootstrap_interval_<param> (the coverage's times sample_factor, like its neighbours), and
    bootstrap_interval_genome_size where the bootstrap was given hist_orig; and, only where the bootstrap was studentized
    (it carries 't_intervals'), bootstrap_t_interval_<param> and bootstrap_t_interval_genome_size, scaled alike
    (DESIGN.md 6x).  They share the model's independence assumption.  Without it the record is unchanged.
    `jackknife`: the dict covest_amd.jackknife.read_jackknife returns (sample factor 1 by its own rule, so nothing is
    scaled); the record then carries jackknife_groups, jackknife_used, jackknife_failed, jackknife_level and, per free
    parameter and for genome_size, jackknife_se_<name>, jackknife_bias_<name> and jackknife_interval_<name>: the
    delete-a-group jackknife over READS, which sees the dependence between the k-mers of one read, and
    where the dict carries 'route' (read_jackknife sets it for a route other than its default, "recount"), jackknife_route:
    how the leave-out histograms were made (the numbers are the same).  Without it the record is unchanged.
    `posterior`: the PosteriorClasses covest_amd.posterior.posterior_classes returns; the record then carries
    posterior_error_cutoff (error_cutoff at level 0.5, None where there is none), posterior_erroneous_kmers,
    posterior_error_free_kmers, one posterior_copies_* per copy column (expected_kmers), posterior_undefined_kmers and
    posterior_sample_factor.  They are numbers of the histogram the model was fitted to: for a sample factor other than
    1 they are recorded as such, with the factor beside them, and are NOT scaled back to the un-sampled data (DESIGN.md
    6ab).  Without it the record is unchanged.
    `read_errors`: the ReadErrorScores covest_amd.read_errors.read_error_scores returns; the record then carries
    read_errors_cutoff, read_errors_level, read_errors_reads, read_errors_flagged_share, read_errors_predicted_share
    (the model's share of reads with a wrong base, NOT the detector's expectation: DESIGN.md 6ae) and
    read_errors_mean_expected_erroneous_kmers.  Without it the record is unchanged.
    `corrections`: what covest_amd.read_errors.correct_reads (or KmerCounts.correct) returns; the record then carries
    corrections_cutoff, corrections_reads and the totals corrections_runs, corrections_corrected,
    corrections_ambiguous and corrections_unfixable.  Without it the record is unchanged.
    `read_influence`: the ReadInfluence covest_amd.influence.read_influence returns, or its summary() (sample factor 1
    by its own rule, so nothing is scaled); the record then carries read_influence_reads, read_influence_level and, per
    free parameter and for genome_size, read_influence_se_<name> and read_influence_interval_<name>: the linearised
    delete-ONE-read jackknife, the genome held fixed, first order in the inverse information.  Where it
    has no covariance to start from the record carries read_influence_reason instead.  Without it the record is
    unchanged.
    `read_bootstrap`: the dict covest_amd.read_bootstrap.read_bootstrap returns (sample factor 1 by its own rule, so
    nothing is scaled); the record then carries read_bootstrap_replicates, read_bootstrap_used, read_bootstrap_failed,
    read_bootstrap_level and, per free parameter and for genome_size, read_bootstrap_se_<name>,
    read_bootstrap_bias_<name> and read_bootstrap_interval_<name> (the percentile interval): the Poisson bootstrap over
    READS, the genome held fixed -- measured to be biased by the duplicated reads, the jackknife's fields are the ones
    to rely on.  Without it the record is unchanged.
    `duplicates`: the DedupReads covest_amd.dedup.dedup_reads returns; the record then carries duplicates_reads (the
    reads that went in), duplicates_kept, duplicates_share (the share that was dropped) and duplicates_max_copies
    (DESIGN.md 6al).  Without it the record is unchanged.
    `copy_spectrum`: the CopySpectrum covest_amd.copy_spectrum.copy_spectrum returns -- the truth, where the genome is
    known; the record then carries one copy_spectrum_* per entry of its observed_kmers() (the columns of `posterior`
    where that is given, four otherwise), named like their posterior_* counterparts, copy_spectrum_error_cutoff (the
    measured cutoff at level 0.5; the model's is posterior_error_cutoff) and copy_spectrum_q1, _q2, _q
    (spectrum_to_q of its genome_spectrum()).  They compare with the posterior_* fields only where the model was fitted
    to the histogram of the joined counts with no sample factor.  Without it the record is unchanged."""
    def named(names, values):
        """{name: value} without the None entries; the coverage (first entry) is reported for the
        un-sampled data, i.e. times sample_factor."""
        if values is None or names is None:
            return {}
        row = [None if v is None else float(v) for v in values]
        if row[0] is not None and sample_factor is not None:
            row[0] *= sample_factor
        return {name: v for name, v in zip(names, row) if v is not None}

    def resampled(prefix, result, count=None, kinds=(('se', 'standard_errors'), ('bias', 'bias'))):
        """The fields of a statistic over resampled reads under `prefix`: with `count` (the key of its groups or
        replicates) that number, used, failed and level; then, per parameter and for the genome size, the `kinds` and the
        interval where it has them."""
        if count is not None:
            for key, kind in ((count, int), ('used', int), ('failed', int), ('level', float)):
                record['%s_%s' % (prefix, key)] = kind(result[key])
        for name in list(model.params) + ['genome_size']:
            for key, source in kinds:
                value = result[source].get(name)
                if value is not None:
                    record['%s_%s_%s' % (prefix, key, name)] = float(value)
            interval = result['intervals'].get(name)
            if interval is not None:
                record['%s_interval_%s' % (prefix, name)] = [float(v) for v in interval]

    record = {
        'model': model.short_name(),
        'hist_size': max(model.hist),
        'sample_factor': sample_factor,
        'orig_sample_factor': orig_sample_factor,
        'success': success,
        'version': __version__,
        'starting_points': starting_points,
        'use_grid_search': use_grid_search,
    }
    if guess is not None:
        record.update(named(('guessed_coverage', 'guessed_error_rate'), guess))
        record['guessed_loglikelihood'] = model.compute_loglikelihood(*guess)
    if estimated is not None:
        record.update(named(model.params, estimated))
        record['orig_coverage'] = float(estimated[0] * orig_sample_factor * sample_factor)
        record['loglikelihood'] = model.compute_loglikelihood(*estimated)
        occurrences = sum(i * n for i, n in hist_orig.items())
        record['genome_size'] = _finite_int(round(occurrences / model.correct_c(estimated[0] * sample_factor)))
        if reads_size is not None:
            record['genome_size_reads'] = _finite_int(
                round(reads_size / (estimated[0] * sample_factor * orig_sample_factor)))
    if orig is not None and any(orig):
        record.update(named(['provided_%s' % name for name in model.params], orig))
        try:
            record['provided_loglikelihood'] = model.compute_loglikelihood(*_none_filled(orig, estimated))
        except ValueError:
            pass
    if intervals is not None:
        record['coverage_interval'] = list(intervals['coverage_interval'])
        record['genome_size_interval'] = (None if intervals.get('genome_size_interval') is None
                                          else list(intervals['genome_size_interval']))
        record['interval_level'] = float(intervals['level'])
    if information is not None:
        from .information import genome_size_se, wald_intervals
        level = float(information.get('level', 0.95))
        scale = 1 if sample_factor is None else sample_factor
        first = model.params[0]
        errors = {name: (None if se is None else float(se * scale if name == first else se))
                  for name, se in information['standard_errors'].items()}
        walds = {name: (None if iv is None else [float(v * scale if name == first else v) for v in iv])
                 for name, iv in wald_intervals(information, level).items()}
        size = genome_size_se(model, hist_orig, information, sample_factor=scale, level=level)
        record['standard_errors'] = errors
        record['wald_intervals'] = walds
        record['genome_size_se'] = None if size['genome_size_se'] is None else float(size['genome_size_se'])
        record['genome_size_wald_interval'] = (None if size['genome_size_wald_interval'] is None
                                               else [float(v) for v in size['genome_size_wald_interval']])
        record['wald_level'] = level
        if 'robust_standard_errors' in information:
            robust = genome_size_se(model, hist_orig, information, sample_factor=scale, level=level, robust=True)
            record['robust_standard_errors'] = {
                name: (None if se is None else float(se * scale if name == first else se))
                for name, se in information['robust_standard_errors'].items()}
            record['robust_wald_intervals'] = {
                name: (None if iv is None else [float(v * scale if name == first else v) for v in iv])
                for name, iv in wald_intervals(information, level, robust=True).items()}
            record['genome_size_robust_se'] = None if robust['genome_size_se'] is None else float(robust['genome_size_se'])
    if bootstrap is not None:
        scale = 1 if sample_factor is None else sample_factor
        first = model.params[0]
        record['bootstrap_replicates'] = int(bootstrap['replicates'])
        record['bootstrap_failed'] = int(bootstrap['failed'])
        for name in model.params:
            by = scale if name == first else 1
            for key, source in (('bias', 'bias'), ('se', 'standard_errors')):
                value = bootstrap[source].get(name)
                if value is not None:
                    record['bootstrap_%s_%s' % (key, name)] = float(value * by)
            interval = bootstrap['percentile_intervals'].get(name)
            if interval is not None:
                record['bootstrap_interval_%s' % name] = [float(v * by) for v in interval]
            t_interval = bootstrap.get('t_intervals', {}).get(name)
            if t_interval is not None:
                record['bootstrap_t_interval_%s' % name] = [float(v * by) for v in t_interval]
        size = bootstrap.get('genome_size')
        if size is not None and size.get('interval') is not None:
            record['bootstrap_interval_genome_size'] = [float(v) for v in size['interval']]
        if size is not None and size.get('t_interval') is not None:
            record['bootstrap_t_interval_genome_size'] = [float(v) for v in size['t_interval']]
    if jackknife is not None:
        resampled('jackknife', jackknife, 'groups')
        if jackknife.get('route') is not None:
            record['jackknife_route'] = str(jackknife['route'])
    if posterior is not None:
        cutoff = posterior.error_cutoff()
        record['posterior_error_cutoff'] = None if cutoff is None else int(cutoff)
        for name, value in posterior.expected_kmers().items():
            record['posterior_%s%s' % (name, '' if name.startswith('copies_') else '_kmers')] = float(value)
        record['posterior_sample_factor'] = sample_factor
    if read_errors is not None:
        n = int(read_errors.n_reads)
        record['read_errors_cutoff'] = int(read_errors.cutoff)
        record['read_errors_level'] = None if read_errors.level is None else float(read_errors.level)
        record['read_errors_reads'] = n
        record['read_errors_flagged_share'] = float(read_errors.flagged_share)
        record['read_errors_predicted_share'] = float(read_errors.predicted_share)
        record['read_errors_mean_expected_erroneous_kmers'] = (
            float(sum(read_errors.expected_erroneous_kmers.tolist()) / n) if n else float('nan'))
    if corrections is not None:
        record['corrections_cutoff'] = int(corrections.cutoff)
        record['corrections_reads'] = int(corrections.runs.size)
        for name in ('runs', 'corrected', 'ambiguous', 'unfixable'):
            record['corrections_' + name] = int(getattr(corrections, name).sum())
    if read_influence is not None:
        summary = read_influence.summary() if hasattr(read_influence, 'summary') else read_influence
        record['read_influence_reads'] = int(summary['reads'])
        record['read_influence_level'] = float(summary['level'])
        if summary.get('reason') is not None:
            record['read_influence_reason'] = str(summary['reason'])
        resampled('read_influence', summary, kinds=(('se', 'standard_errors'),))
    if read_bootstrap is not None:
        resampled('read_bootstrap', read_bootstrap, 'replicates')
    if duplicates is not None:
        record['duplicates_reads'] = int(duplicates.n_input)
        record['duplicates_kept'] = int(duplicates.n_reads)
        record['duplicates_share'] = float(duplicates.duplicate_share)
        record['duplicates_max_copies'] = int(duplicates.copies.max()) if duplicates.n_reads else 0
    if copy_spectrum is not None:
        from .simulate import spectrum_to_q
        columns = 4 if posterior is None else posterior.copy_share.shape[1]
        for name, value in copy_spectrum.observed_kmers(columns).items():
            record['copy_spectrum_%s%s' % (name, '' if name.startswith('copies_') else '_kmers')] = int(value)
        cutoff = copy_spectrum.error_cutoff()
        record['copy_spectrum_error_cutoff'] = None if cutoff is None else int(cutoff)
        for name, value in zip(('q1', 'q2', 'q'), spectrum_to_q(copy_spectrum.genome_spectrum())):
            record['copy_spectrum_' + name] = None if value is None else float(value)
    if not silent:
        print(yaml.dump(record, indent=4, default_flow_style=False))
    return record
