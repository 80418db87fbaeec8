"""What a fit says about the k-mers of each abundance (covest_amd.posterior): a `.hist` file and an
estimate -- given, or the default flow's own (process_histogram -> first guess -> CoverageEstimator) -- into a table per
key: count, ln p_j, erroneous share, the copy columns, mean copies; then the error cutoff and the expected counts.

    python tools/posterior_table.py tests/golden/sim_c10_e0.05.hist [--model repeats] [--estimate c e [q1 q2 q]]
                                    [--copy-columns 4] [--rows 40] [--out FILE (appended to)]
    python tools/posterior_table.py --repeat-seed 0 --model repeats      # the histogram tools/repeat_recovery.py simulates

The numbers are of the histogram the model was fitted to (after process_histogram's trimming and sampling): the sample
factor is printed beside them and nothing is scaled back.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from covest_amd import constants, posterior_classes, select_model  # noqa: E402
from covest_amd.estimator import CoverageEstimator  # noqa: E402
from covest_amd.hist_steps import load_histogram, process_histogram  # noqa: E402


def repeat_histogram(seed):
    """The forward-strand 21-mer histogram of tests/repeat_recovery.py's simulated reads of a repeat genome."""
    from repeat_recovery import LOOP
    from covest_amd import kmer_hist as kh, simulate as sim
    g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], seed,
                          divergence=LOOP["divergence"])
    reads = sim.simulate_reads(g.bases, LOOP["read_len"], coverage=LOOP["coverage"], error_rate=LOOP["error_rate"], seed=seed,
                               both_strands=False)
    counts = reads.add_to(kh.KmerCounts(LOOP["k"], canonical=False))
    hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    return hist, LOOP["k"], LOOP["read_len"]


def fit(model, guess_c, guess_e):
    guess = list(model.defaults)
    if not (guess_c == 0 and guess_e == 1):
        guess[:2] = guess_c, guess_e
    res, success = CoverageEstimator(model).compute_coverage(guess)
    return [float(v) for v in res], success


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("hist", nargs="?")
    ap.add_argument("--repeat-seed", type=int, default=None)
    ap.add_argument("--model", default="basic")
    ap.add_argument("-k", type=int, default=constants.DEFAULT_K)
    ap.add_argument("-r", type=int, default=constants.DEFAULT_READ_LENGTH)
    ap.add_argument("--estimate", type=float, nargs="+", default=None)
    ap.add_argument("--copy-columns", type=int, default=4)
    ap.add_argument("--rows", type=int, default=40, help="keys printed, in ascending order (0: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if (args.hist is None) == (args.repeat_seed is None):
        ap.error("a .hist file or --repeat-seed")
    if args.repeat_seed is not None:
        hist_orig, k, r = repeat_histogram(args.repeat_seed)
        name = "tools/repeat_recovery.py seed %d" % args.repeat_seed
    else:
        (hist_orig, _), k, r = load_histogram(args.hist), args.k, args.r
        name = os.path.relpath(args.hist, REPO) if os.path.isabs(args.hist) else args.hist
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, k, r)
    model = select_model(args.model)(k, r, hist, tail, max_error=constants.MAX_ERRORS)
    if args.estimate is not None:
        est, how = list(args.estimate), "given"
    else:
        est, success = fit(model, guess_c, guess_e)
        how = "the default flow's own (success: %s)" % success
    pc = posterior_classes(model, est, copy_columns=args.copy_columns)
    Cc = pc.copy_share.shape[1]
    names = ["copies_%d" % (c + 1) for c in range(Cc - 1)] + ["copies_ge_%d" % Cc]
    lines = ["# %s, %s model, k = %d, r = %d: %d keys, tail %g, sample factor %s" % (name, model.short_name(), k, r, len(hist),
                                                                                   tail, sample_factor),
             "# estimate, %s: %s" % (how, ", ".join("%s = %.6g" % (p, v) for p, v in zip(model.params, est))),
             "# %6s %12s %14s %12s %s %12s" % ("key", "count", "ln p_j", "erroneous", " ".join("%12s" % n for n in names),
                                               "mean copies")]
    order = sorted(range(len(pc.keys)), key=lambda i: pc.keys[i])
    bad = pc.erroneous
    for i in (order if args.rows == 0 else order[:args.rows]):
        lines.append("  %6d %12d %14.6f %12.6g %s %12.6f" % (pc.keys[i], pc.counts[i], pc.log_p[i], bad[i],
                                                           " ".join("%12.6g" % v for v in pc.copy_share[i]),
                                                           pc.mean_copies[i]))
    if args.rows and len(order) > args.rows:
        lines.append("  ... %d more keys" % (len(order) - args.rows))
    lines.append("# error cutoff (erroneous share below 0.5 at every key from it on): %s" % pc.error_cutoff())
    total = float(pc.counts.sum())
    for key, v in pc.expected_kmers().items():
        lines.append("# expected distinct k-mers, %-12s %16.1f  (%.4f of %d)" % (key, v, v / total, total))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
