"""The Poisson bootstrap over reads (covest_amd/read_bootstrap.py) beside the project's other
read-level answers, on the simulated genomes and read sets of tools/jackknife_recovery.py; nothing in the output is a
pass mark.

  basic    one random genome of 1 Mbp, 100-base reads at coverage 10, error rate 0.01, k = 21 forward strand, basic model
  repeats  repeat_genome and the repeats model at the settings of tests/repeat_recovery.py
For each: S read sets with simulator seeds 1 .. S, each estimated; the empirical standard deviation of every quantity over
them; on EVERY set the read bootstrap at B replicates and the delete-a-group jackknife at G groups (both seeded with the
set's number), and how often the bootstrap's percentile interval and the jackknife's t interval cover the truth (the
simulator's coverage and genome length, the realised substitution rate, the genome's own (q1, q2, q)); on the first four
sets also the linearised delete-one error (covest_amd/influence.py) and the model's Wald error.  Standard errors are
medians over the sets they were computed on.

And the cost, 6 * 10^6 reads of 100 bases (a 20 Mbp genome at coverage 30), k = 21 canonical, the table reserved once: B
= 64 replicate histograms -- draw, clear, add_weighted_device, histogram, each -- beside 64 x the median of one unweighted
clear + add_device + histogram of the same reads; host wall clock around calls that wait for the device (histogram
does).  `--only unweighted` runs that part alone: it uses nothing the parent of the weighted add lacks, so the same file
measures the parent's number on the parent's library.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/read_bootstrap_recovery.py [--sets 16] [--replicates 64] [--groups 32] [--out profiles/read_bootstrap_recovery.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from covest_amd import simulate as sim  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402


def covers(interval, truth):
    return interval is not None and truth is not None and interval[0] <= truth <= interval[1]


def median_or_none(values):
    values = [v for v in values if v is not None]
    return statistics.median(values) if values else None


def show(v, fmt="%.4g"):
    return fmt % v if v is not None else "none"


def recovery(name, genome, settings, model_name, truth_q, sets, replicates, groups, lines):
    from covest_amd import influence, jackknife
    from covest_amd.information import genome_size_se
    from covest_amd.read_bootstrap import read_bootstrap
    from jackknife_recovery import fit
    k, L = settings["k"], settings["read_len"]
    names = None
    est_rows, boot, jack, lin, wald, hit_boot, hit_jack, notes = [], [], [], [], [], [], [], []
    for seed in range(1, sets + 1):
        t0 = time.perf_counter()
        reads = sim.simulate_reads(genome, L, coverage=settings["coverage"], error_rate=settings["error_rate"], seed=seed,
                                   both_strands=False)
        model, est, ok, hist_orig, trim = fit(reads, k, model_name)
        names = list(model.params) + ["genome_size"]
        occurrences = sum(i * n for i, n in hist_orig.items())
        truth = dict(truth_q, coverage=reads.true_coverage, genome_size=float(len(genome)),
                     error_rate=reads.substitutions(genome) / (reads.n_reads * L))
        est_rows.append(est + [occurrences / model.correct_c(est[0]), ok])
        b = read_bootstrap(model, est, reads, replicates=replicates, seed=seed, trim=trim)
        j = jackknife.read_jackknife(model, est, reads, groups=groups, seed=seed, trim=trim)
        boot.append(b)
        jack.append(j)
        hit_boot.append([covers(b["intervals"][q], truth.get(q)) for q in names])
        hit_jack.append([covers(j["intervals"][q], truth.get(q)) for q in names])
        if seed <= 4:
            counts = reads.add_to(KmerCounts(k, canonical=False))
            infl = influence.read_influence(model, est, counts, reads)
            counts.close()
            summary = infl.summary()
            size = genome_size_se(model, hist_orig, infl.info)
            lin.append(summary["standard_errors"])
            wald.append(dict(infl.info["standard_errors"], genome_size=size["genome_size_se"]))
        notes.append("  %-8s set %2d: bootstrap used %d of %d (reads drawn %d .. %d of %d), keys added %d; jackknife used %d of %d; "
                     "%.1f s" % (name, seed, b["used"], replicates, min(b["reads_drawn"]), max(b["reads_drawn"]), reads.n_reads,
                                 b["keys_added"], j["used"], groups, time.perf_counter() - t0))
        model.close()
    lines.extend(notes)
    good = np.array([r[:-1] for r in est_rows if r[-1]], dtype=np.float64)
    sd = good.std(axis=0, ddof=1)
    lines.append("# %s: %d read sets (%d estimated with success); B = %d, G = %d; standard errors: medians over the sets "
                 "(linearised and Wald: the first four); bias: the bootstrap's mean - full, median; covers: sets whose interval "
                 "holds the truth" % (name, sets, len(good), replicates, groups))
    lines.append("# %-8s %-12s %13s %12s %12s %12s %12s %12s %12s %9s %9s %14s %14s" % (
        "case", "quantity", "mean", "empirical sd", "bootstrap se", "jackknife se", "linearised", "Wald se", "boot bias",
        "boot/emp", "jack/emp", "boot covers", "jack covers"))
    for d, q in enumerate(names):
        bs = median_or_none([b["standard_errors"][q] for b in boot])
        bias = median_or_none([b["bias"][q] for b in boot])
        js = median_or_none([j["standard_errors"][q] for j in jack])
        ls = median_or_none([s.get(q) for s in lin])
        ws = median_or_none([w.get(q) for w in wald])
        known = q in ("coverage", "error_rate", "genome_size") or truth_q.get(q) is not None
        lines.append("  %-8s %-12s %13.8g %12.4g %12s %12s %12s %12s %12s %9s %9s %14s %14s" % (
            name, q, good[:, d].mean(), sd[d], show(bs), show(js), show(ls), show(ws), show(bias, "%.3g"),
            show(bs / sd[d] if bs is not None and sd[d] > 0 else None, "%.3f"),
            show(js / sd[d] if js is not None and sd[d] > 0 else None, "%.3f"),
            "%d of %d" % (sum(h[d] for h in hit_boot), sets) if known else "none",
            "%d of %d" % (sum(h[d] for h in hit_jack), sets) if known else "none"))
    lines.append("#   share of bootstrap refits that ended on a bound, median over the sets: %s" % " ".join(
        "%s %s" % (q, show(median_or_none([b["bound_share"][q] for b in boot]), "%.3f")) for q in names))


# ---- the cost ----------------------------------------------------------------------------------------------------------------
RATE = dict(genome_len=20_000_000, read_len=100, n_reads=6_000_000, k=21, seed=20261021)


def resident_reads():
    dev = torch.device("cuda", 0)
    d_genome = torch.empty(RATE["genome_len"], dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), RATE["genome_len"], RATE["seed"])
    d_reads = torch.empty(RATE["n_reads"] * RATE["read_len"], dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), RATE["genome_len"], RATE["read_len"], RATE["n_reads"], d_reads.data_ptr(),
                              error_rate=0.01, seed=RATE["seed"])
    counts = KmerCounts(RATE["k"], canonical=True)
    counts.add_device(d_reads.data_ptr(), RATE["n_reads"], RATE["read_len"])  # (reserve: the table for the whole set, once)
    counts.histogram()
    return d_reads, counts


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def unweighted(reps, lines, d_reads=None, counts=None):
    """One unweighted clear + add_device + histogram of the resident reads, `reps` times after a discarded one."""
    own = counts is None
    if own:
        d_reads, counts = resident_reads()
    n, L = RATE["n_reads"], RATE["read_len"]

    def one():
        counts.clear()
        counts.add_device(d_reads.data_ptr(), n, L, reserve=False)
        counts.histogram()
    one()
    ms = [wall_ms(one) for _ in range(reps)]
    lines.append("# cost: %d reads of %d bases, k = %d canonical, %d slots; host wall clock; %s" % (
        n, L, RATE["k"], counts.slots, torch.cuda.get_device_name(0)))
    lines.append("  unweighted clear + add_device + histogram: median %.2f ms, least %.2f, most %.2f, of %d; 64 x median %.1f ms; "
                 "all: %s" % (statistics.median(ms), min(ms), max(ms), reps, 64 * statistics.median(ms),
                              " ".join("%.2f" % v for v in ms)))
    if own:
        counts.close()
    return statistics.median(ms), max(ms) - min(ms)


def cost(reps, replicates, lines):
    from covest_amd.read_bootstrap import bootstrap_weights_device
    d_reads, counts = resident_reads()
    n, L = RATE["n_reads"], RATE["read_len"]
    plain, spread = unweighted(reps, lines, d_reads, counts)
    d_w = torch.empty(n, dtype=torch.int32, device=torch.device("cuda", 0))

    def replicate(b):
        bootstrap_weights_device(d_w.data_ptr(), n, b, seed=RATE["seed"])
        counts.clear()
        counts.add_weighted_device(d_reads.data_ptr(), n, L, d_w.data_ptr(), reserve=False)
        counts.histogram()
    replicate(replicates)  # (discarded)
    ms = [wall_ms(lambda b=b: replicate(b)) for b in range(replicates)]
    lines.append("  replicate (draw + clear + add_weighted_device + histogram): median %.2f ms, least %.2f, most %.2f, of %d; "
                 "all %d: %.1f ms" % (statistics.median(ms), min(ms), max(ms), replicates, replicates, sum(ms)))
    draw = [wall_ms(lambda: bootstrap_weights_device(d_w.data_ptr(), n, 1, seed=RATE["seed"])) for _ in range(reps)]
    lines.append("  the draw alone (%d weights): median %.3f ms" % (n, statistics.median(draw)))
    lines.append("  replicate / unweighted, medians: %.3f (the unweighted count's least-to-most spread: %.1f %% of its median)" % (
        statistics.median(ms) / plain, 100.0 * spread / plain))
    counts.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--replicates", type=int, default=64)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip", default="", help="comma-separated: basic, repeats, cost")
    ap.add_argument("--only", default="", help="unweighted: the unweighted count's time alone")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "read_bootstrap_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("read_bootstrap_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    skip = set(args.skip.split(","))
    lines = []

    def write():  # after every part: a run that is cut short leaves what it had
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if args.only == "unweighted":
        unweighted(args.reps, lines)
        write()
        print("\n".join(lines))
        return
    from jackknife_recovery import BASIC
    from repeat_recovery import LOOP
    lines.append("# the Poisson bootstrap over reads at B = %d beside the delete-a-group jackknife at G = %d, the linearised "
                 "delete-one error, the Wald error and the spread over independent read sets of ONE genome" % (args.replicates, args.groups))
    if "cost" not in skip:
        cost(args.reps, args.replicates, lines)
        write()
    if "basic" not in skip:
        lines.append("# basic: random genome %(genome_len)d, L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, k = %(k)d "
                     "forward strand, basic model" % BASIC)
        recovery("basic", sim.random_genome(BASIC["genome_len"], 1), BASIC, "basic", {}, args.sets, args.replicates, args.groups, lines)
        write()
    if "repeats" not in skip:
        lines.append("# repeats: repeat genome %(genome_len)d, unit_len %(unit_len)d, (q1, q2, q) = (%(q1)g, %(q2)g, %(q)g), "
                     "L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, k = %(k)d forward strand, repeats model" % LOOP)
        g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], 1,
                              divergence=LOOP["divergence"])
        q1, q2, q = sim.spectrum_to_q(sim.genome_spectrum(g, LOOP["k"], canonical=False))
        recovery("repeats", g.bases, LOOP, "repeats", dict(q1=q1, q2=q2, q=q), args.sets, args.replicates, args.groups, lines)
        write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
