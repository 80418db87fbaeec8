"""The posterior classes of a fitted model against the measured truth (TEST INFRASTRUCTURE ONLY; not collected): repeat
genome -> reads (covest_amd.simulate) -> forward-strand 21-mer counts -> histogram -> fit -> posterior_classes, and the
same counts joined with the genome's own (copy_spectrum) -> compare.  The settings are tests/repeat_recovery.py's;
tools/copy_spectrum_recovery.py records it for seeds 1..8 and both models,
tests/test_gpu_copy_spectrum_recovery.py holds seed 0 to twice the worst it recorded.

The model is fitted to the histogram of the very counts that are joined, with no sample factor: what compare asks for.
"""
import math

import numpy as np

from repeat_recovery import LOOP

COPY_COLUMNS = 3          # 1 copy, 2 copies, 3 and more
MODELS = ("basic", "repeats")
PROFILE_COPIES = (1, 2, 3)


def fit(hist, model_name):
    """(model, estimate) as tests/flow_helper.py fits, the histogram not down-sampled (it may still be trimmed)."""
    from covest_amd import constants
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import process_histogram
    from covest_amd.models import select_model
    trimmed, tail, _, guess_c, guess_e = process_histogram(hist, LOOP["k"], LOOP["read_len"], sample_factor=1)
    m = select_model(model_name)(LOOP["k"], LOOP["read_len"], trimmed, tail, max_error=constants.MAX_ERRORS, max_cov=None,
                                 min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
    guess = list(m.defaults)
    if not (guess_c == 0 and guess_e == 1):
        guess[:2] = guess_c, guess_e
    est, _ = CoverageEstimator(m, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage(guess)
    return m, [float(v) for v in est]


def truncated_poisson(rate, n):
    """P(a | a >= 1), a = 0 .. n - 1 (index 0 is 0), of a Poisson of `rate`."""
    a = np.arange(1, n, dtype=np.float64)
    log_p = a * math.log(rate) - rate - np.array([math.lgamma(v + 1.0) for v in a]) - math.log1p(-math.exp(-rate))
    return np.concatenate([[0.0], np.exp(log_p)])


def moments(p):
    a = np.arange(len(p), dtype=np.float64)
    mean = float((a * p).sum())
    return mean, float((((a - mean) ** 2) * p).sum())


def relative_gap(expected, observed):
    return abs(expected - observed) / observed if observed else math.inf


def recover(seed, model_name):
    """One seed, one model -> dict: 'estimate', 'cutoff' (model, measured), 'expected' / 'observed' (the totals of
    compare; 'copy_expected' / 'observed' and 'copy_keys', the least and largest: the same over the keys with E_0 >= 0.99
    alone), 'gaps' {'error_cutoff': |model - measured|, name: |expected - observed| / observed}, 'q' ((q1, q2, q) of
    the estimate -- None for the basic model --, spectrum_to_q of the measured genome spectrum), 'profiles' {o: (N_o seen,
    mean and variance of the measured abundance profile N[a][o] / N_o over a >= 1, the same of the model's truncated
    Poisson at o times the error-free k-mer coverage, the total variation distance of the two)}."""
    from covest_amd import copy_spectrum, posterior_classes, simulate as sim
    from covest_amd.kmer_hist import KmerCounts
    g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], seed,
                          divergence=LOOP["divergence"])
    reads = sim.simulate_reads(g.bases, LOOP["read_len"], coverage=LOOP["coverage"], error_rate=LOOP["error_rate"], seed=seed,
                               both_strands=False)
    counts = reads.add_to(KmerCounts(LOOP["k"], canonical=False))
    truth = sim.genome_counts(g, LOOP["k"], canonical=False)
    try:
        hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
        spectrum = copy_spectrum(counts, truth)
    finally:
        counts.close()
        truth.close()
    model, estimate = fit(hist, model_name)
    posterior = posterior_classes(model, estimate, copy_columns=COPY_COLUMNS)
    compared = spectrum.compare(posterior)
    expected, observed = compared["expected"], compared["observed"]
    cutoff = compared["error_cutoff"]
    gaps = {"error_cutoff": math.inf if None in cutoff else abs(cutoff[0] - cutoff[1])}
    for name in ("erroneous", "copies_1", "copies_2", "copies_ge_3"):
        gaps[name] = relative_gap(expected[name], observed[name])
    for name in ("copies_1", "copies_2", "copies_ge_3"):   # like for like: over the keys the model calls error-free alone
        gaps["error_free_" + name] = relative_gap(compared["copy_expected"][name], compared["copy_observed"][name])
    rate = model.correct_c(estimate[0]) * (1.0 - estimate[1]) ** LOOP["k"]   # error-free k-mer coverage of one copy
    profiles = {}
    for o in PROFILE_COPIES:
        column = spectrum.matrix[:, o].astype(np.float64) if o < spectrum.matrix.shape[1] else np.zeros(1)
        column[0] = 0.0
        seen = column.sum()
        if not seen:
            continue
        measured = column / seen
        modelled = truncated_poisson(o * rate, max(len(measured), int(4 * o * rate) + 20))
        n = max(len(measured), len(modelled))
        pad = lambda p: np.concatenate([p, np.zeros(n - len(p))])
        profiles[o] = (int(seen),) + moments(measured) + moments(modelled) + (
            0.5 * float(np.abs(pad(measured) - pad(modelled)).sum()),)
    return {"estimate": estimate, "cutoff": cutoff, "expected": expected, "observed": observed, "gaps": gaps,
            "copy_keys": (int(compared["copy_keys"].min()), int(compared["copy_keys"].max())) if compared["copy_keys"].size else None,
            "copy_expected": compared["copy_expected"], "copy_observed": compared["copy_observed"],
            "q": (tuple(estimate[2:5]) if len(estimate) >= 5 else None, sim.spectrum_to_q(spectrum.genome_spectrum())),
            "profiles": profiles}
