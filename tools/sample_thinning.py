"""The thinning model (covest_thin_histogram, the reference's sample_histogram) against what it predicts: simulate
reads at c = 40, e = 0.02, L = 100 from a 200 000-base genome (seeds 1..8), sample them at factor 2
(covest_amd.sample), count the canonical 21-mers of the sample, and put beside that histogram the expected counts the
thinning model gives from the histogram of ALL the reads.  Per abundance with an expected count of at least 25:
(observed - expected) / sqrt(expected), and its largest magnitude.  A report, not a test: neighbouring k-mers share
their reads, so the bins' variances are not the multinomial ones.

    python tools/sample_thinning.py [--out profiles/sample_thinning.txt]
"""
import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from covest_amd import hist_steps, kmer_hist as kh, sample, simulate as sim  # noqa: E402

GENOME_LEN, READ_LEN, COVERAGE, ERROR_RATE, K, FACTOR, MIN_EXPECTED = 200_000, 100, 40, 0.02, 21, 2, 25


def histogram_of(reads):
    counts = reads.add_to(kh.KmerCounts(K, canonical=True))
    hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_thinning.txt"))
    ap.add_argument("--seeds", default="1-8")
    args = ap.parse_args()
    a, b = (int(x) for x in args.seeds.split("-"))
    lines = ["# sampled reads, counted, against the thinning model's expectation from the full histogram: genome %d, "
             "L = %d, c = %g, e = %g, factor %g, k = %d canonical; bins with an expected count >= %d"
             % (GENOME_LEN, READ_LEN, COVERAGE, ERROR_RATE, FACTOR, K, MIN_EXPECTED),
             "# %-4s %9s %12s %14s %9s" % ("seed", "abundance", "observed", "expected", "z")]
    worst_all = 0.0
    for seed in range(a, b + 1):
        g = sim.random_genome(GENOME_LEN, seed)
        reads = sim.simulate_reads(g, READ_LEN, coverage=COVERAGE, error_rate=ERROR_RATE, seed=seed)
        full = histogram_of(reads)
        observed = histogram_of(sample.sample_reads(reads, FACTOR, seed=seed))
        expected = hist_steps.expected_sampled(full, FACTOR)
        worst = 0.0
        for j in sorted(expected):
            if expected[j] >= MIN_EXPECTED:
                z = (observed.get(j, 0) - expected[j]) / math.sqrt(expected[j])
                worst = max(worst, abs(z))
                lines.append("  %-4d %9d %12d %14.2f %9.2f" % (seed, j, observed.get(j, 0), expected[j], z))
        lines.append("# seed %d: largest |z| %.2f" % (seed, worst))
        worst_all = max(worst_all, worst)
    lines.append("# largest |z| over the seeds %.2f" % worst_all)
    text = "\n".join(lines) + "\n"
    print("\n".join(l for l in lines if l.startswith("#")))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
