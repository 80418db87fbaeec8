"""The experiment DESIGN.md section 6n leaves open, by parametric bootstrap (covest_amd.bootstrap, section 6p): is the
repeat model's estimator biased at the coverage the default flow samples down to EVEN WHEN THE DATA ARE EXACTLY THE
MODEL'S, or are the pipeline's data not the model's?

The seed-0 histogram of tests/repeat_recovery.py as the default flow processes it (sampled and trimmed), repeats model,
at two points -- the measured truth (realised c and e, spectrum_to_q of the genome) and the flow's estimate: the
log-likelihood of both on that histogram, then B = 64 model-drawn histograms from each, refitted as the flow refits
(err_scale as its default), with bias, standard errors, percentile intervals, the share of refits on a bound, and
the ratio of the bootstrap's standard error to the Wald one (information.observed_information).  The same from the
truth with the sampling switched off (sample_factor = 1).  And the basic model on tests/golden/sim_c10_e0.05.hist at
the flow's estimate -- tests/test_gpu_bootstrap.py reads that block's ratios.  Nothing is tuned: whatever the bias of
q1, q2, q turns out to be is written down.

    python tools/bootstrap_recovery.py [--replicates 64] [--out profiles/bootstrap_recovery.txt]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_hist  # noqa: E402
from repeat_recovery import LOOP  # noqa: E402
from covest_amd import (BasicModel, CoverageEstimator, RepeatsModel, constants, kmer_hist as kh,  # noqa: E402
                        observed_information, parametric_bootstrap, simulate as sim)
from covest_amd.hist_steps import process_histogram  # noqa: E402

SEED_BASIC, SEED_REPEATS = 1, 1  # (tests/test_gpu_bootstrap.py uses another)


def fit(model, guess_c, guess_e):
    """The default flow's estimate (tests/flow_helper.py): first guess from the moments, one refinement."""
    guess = list(model.defaults)
    if not (guess_c == 0 and guess_e == 1):
        guess[:2] = guess_c, guess_e
    return CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage(guess)


def block(lines, name, title, model, point, hist_orig, sample_factor, replicates, seed):
    """One bootstrap from `point`, written as a table; the '# se ratio' lines are what the test reads."""
    t0 = time.perf_counter()
    boot = parametric_bootstrap(model, point, replicates=replicates, seed=seed, hist_orig=hist_orig,
                                sample_factor=sample_factor, err_scale=constants.DEFAULT_ERR_SCALE)
    seconds = time.perf_counter() - t0
    info = observed_information(model, point)
    lines.append("# [%s] %s" % (name, title))
    lines.append("#   B = %d, seed %d, n_draws %d, failed %d, %.1f s; log-likelihood at the point %.4f; Wald: %s"
                 % (replicates, seed, boot["n_draws"], boot["failed"], seconds, model.compute_loglikelihood(*point),
                    info["reason"] or "ok"))
    lines.append("#   %-12s %12s %12s %12s %11s %11s %8s %25s %9s"
                 % ("parameter", "point", "mean", "bias", "boot se", "Wald se", "ratio", "percentile interval", "at bound"))
    good = boot["success"]
    for d, pname in enumerate(model.params):
        se, wald = boot["standard_errors"][pname], info["standard_errors"][pname]
        ratio = se / wald if se is not None and wald else float("nan")
        lo, hi = boot["percentile_intervals"][pname]
        share = float(boot["at_bound"][good, d].mean()) if good.any() else float("nan")
        lines.append("    %-12s %12.6g %12.6g %12.3g %11.3g %11.3g %8.3f %25s %9.3f"
                     % (pname, point[d], boot["mean"][pname], boot["bias"][pname], se, wald if wald else float("nan"), ratio,
                        "[%.6g, %.6g]" % (lo, hi), share))
        lines.append("# se ratio, %s %s %.4f" % (name, pname, ratio))
    size = boot["genome_size"]
    lines.append("    %-12s %12s %12.8g %12s %11.3g %11s %8s %25s"
                 % ("genome_size", "", size["mean"], "", size["standard_error"], "", "", "[%.8g, %.8g]" % tuple(size["interval"])))
    print("\n".join(lines[-(len(model.params) * 2 + 4):]), flush=True)
    return boot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bootstrap_recovery.txt"))
    args = ap.parse_args()
    B = args.replicates
    lines = ["# parametric bootstrap (covest_amd.bootstrap): B model-drawn histograms from a known point, each refitted",
             "# ratio = bootstrap se / Wald se; at bound = share of the successful refits that ended on a bound"]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # ---- the basic model on the golden histogram, at the flow's estimate
    hist_orig = load_hist("sim_c10_e0.05")
    hist, tail, sf, gc, ge = process_histogram(hist_orig, 21, 100)
    model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
    est, ok = fit(model, gc, ge)
    block(lines, "basic", "basic model, tests/golden/sim_c10_e0.05.hist, at the flow's estimate (success %s)" % ok, model, est,
          hist_orig, sf, B, SEED_BASIC)
    model.close()
    save()

    # ---- the repeat model on the seed-0 recovery histogram
    g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], 0, divergence=LOOP["divergence"])
    reads = sim.simulate_reads(g.bases, LOOP["read_len"], coverage=LOOP["coverage"], error_rate=LOOP["error_rate"], seed=0,
                               both_strands=False)
    counts = reads.add_to(kh.KmerCounts(LOOP["k"], canonical=False))
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    q_truth = sim.spectrum_to_q(sim.genome_spectrum(g, LOOP["k"], canonical=False))
    c_truth = reads.true_coverage
    e_truth = reads.substitutions(g.bases) / (reads.n_reads * reads.read_length)
    for tag, forced in (("", None), ("_unsampled", 1)):
        hist, tail, sf, gc, ge = process_histogram(hist_orig, LOOP["k"], LOOP["read_len"], sample_factor=forced)
        model = RepeatsModel(LOOP["k"], LOOP["read_len"], hist, tail, max_error=constants.MAX_ERRORS,
                             min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
        truth = [c_truth / sf, e_truth] + list(q_truth)
        where = "seed-0 recovery histogram, sample_factor %d, %d keys to %d, tail %g" % (sf, len(hist), max(hist), tail)
        lines.append("# %s: k-mer coverage at the truth %.3f" % (where, model.correct_c(truth[0]) * (1 - e_truth) ** LOOP["k"]))
        block(lines, "repeats_truth" + tag, "repeats model, %s, at the MEASURED TRUTH" % where, model, truth, hist_orig, sf, B,
              SEED_REPEATS)
        save()
        if forced is None:
            est, ok = fit(model, gc, ge)
            lines.append("# log-likelihood on that histogram: at the truth %.4f, at the estimate %.4f"
                         % (model.compute_loglikelihood(*truth), model.compute_loglikelihood(*est)))
            block(lines, "repeats_estimate", "repeats model, %s, at the flow's ESTIMATE (success %s)" % (where, ok), model, est,
                  hist_orig, sf, B, SEED_REPEATS)
            save()
        model.close()
    print("written", args.out)


if __name__ == "__main__":
    main()
