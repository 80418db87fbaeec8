"""How well the posterior classes of a fitted model match the truth, where the truth is the join of the reads' k-mer table
with the genome's own (covest_amd.copy_spectrum), and what the join costs.

  recovery  tests/copy_spectrum_recovery.py for seeds 1..8 and both models, at the settings of tests/repeat_recovery.py:
            the modelled and the measured error cutoff, the expected and the observed numbers of erroneous, 1-copy,
            2-copy and >= 3-copy k-mers, (q1, q2, q) of the estimate beside spectrum_to_q of the measured spectrum, and
            per copy number the measured abundance profile N[a][o] / N_o beside the model's truncated Poisson at o times
            the error-free k-mer coverage (mean, variance, total variation distance).  The caps of
            tests/test_gpu_copy_spectrum_recovery.py are twice the worst gap of the eight seeds, per model.
  cost      6 * 10^6 reads of 100 bases (a 20 Mbp genome at coverage 30, error rate 0.01), k = 21 canonical, joined with
            the genome's table, unclipped: HIP events around KmerCounts.histogram() of both tables (existing code, the
            yardstick), around join_histogram (the host form, its copy back included) and around join_histogram_device
            alone, each the median of `--reps` runs after a discarded one, in one process.  The library is the one
            COVEST_AMD_LIB names, so a variant build is timed by a second run with `--label` and `--append`.

    python tools/copy_spectrum_recovery.py [--only recovery|cost] [--label TEXT] [--append] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch  # first: ONE HIP runtime per process

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from covest_amd import simulate as sim  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402

GAPS = ("error_cutoff", "erroneous", "copies_1", "copies_2", "copies_ge_3")
ERROR_FREE = ("copies_1", "copies_2", "copies_ge_3")


def show(v, fmt="%.4g"):
    return "none" if v is None else fmt % v


def recovery(seeds, lines):
    from copy_spectrum_recovery import MODELS, recover
    from repeat_recovery import LOOP
    lines.append("# posterior classes against the joined truth: genome %(genome_len)d, unit_len %(unit_len)d, (q1, q2, q) = "
                 "(%(q1)g, %(q2)g, %(q)g), divergence %(divergence)g, L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, "
                 "k = %(k)d forward strand; the model fitted to the histogram of the joined counts, no sample factor" % LOOP)
    lines.append("# gap: |model - measured| for the error cutoff, |expected - observed| / observed for the numbers of k-mers")
    worst = {}
    for model in MODELS:
        for seed in seeds:
            r = recover(seed, model)
            lines.append("  %-7s seed %d estimate %s" % (model, seed, " ".join("%.6g" % v for v in r["estimate"])))
            lines.append("    error cutoff: model %s measured %s gap %s" % (show(r["cutoff"][0], "%d"), show(r["cutoff"][1], "%d"),
                                                                           show(r["gaps"]["error_cutoff"])))
            for name in GAPS[1:]:
                lines.append("    %-12s expected %14.2f observed %10d gap %.5f" % (name, r["expected"][name], r["observed"][name],
                                                                                  r["gaps"][name]))
            lines.append("    over the keys with E_0 >= 0.99 alone (%s):" % ("none" if r["copy_keys"] is None else "%d .. %d" % r["copy_keys"]))
            for name in ERROR_FREE:
                lines.append("    %-12s expected %14.2f observed %10d gap %.5f" % (name, r["copy_expected"][name], r["copy_observed"][name],
                                                                                  r["gaps"]["error_free_" + name]))
            est_q, true_q = r["q"]
            lines.append("    q1 q2 q: estimate %s measured %s" % (
                "none (basic model)" if est_q is None else " ".join("%.5f" % v for v in est_q), " ".join(show(v, "%.5f") for v in true_q)))
            for o, (seen, m_mean, m_var, t_mean, t_var, tv) in sorted(r["profiles"].items()):
                lines.append("    copies %d: %8d k-mers seen; abundance mean %.4f variance %.4f measured, mean %.4f variance %.4f "
                             "modelled; total variation %.5f" % (o, seen, m_mean, m_var, t_mean, t_var, tv))
            for name in GAPS + tuple("error_free_" + n for n in ERROR_FREE):
                worst[(model, name)] = max(worst.get((model, name), 0.0), r["gaps"][name])
    for (model, name), gap in worst.items():
        lines.append("# largest gap, %-7s %-22s %10.5f   twice: %10.5f" % (model, name, gap, 2 * gap))


# ---- the cost ----------------------------------------------------------------------------------------------------------------
RATE = dict(genome_len=20_000_000, read_len=100, n_reads=6_000_000, k=21, seed=20261021)


def event_ms(fn):
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    begin.record()
    fn()
    end.record()
    end.synchronize()
    return begin.elapsed_time(end)


def cost(reps, label, lines):
    dev = torch.device("cuda", 0)
    d_genome = torch.empty(RATE["genome_len"], dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), RATE["genome_len"], RATE["seed"])
    d_reads = torch.empty(RATE["n_reads"] * RATE["read_len"], dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), RATE["genome_len"], RATE["read_len"], RATE["n_reads"], d_reads.data_ptr(),
                              error_rate=0.01, seed=RATE["seed"])
    counts = KmerCounts(RATE["k"], canonical=True)
    counts.add_device(d_reads.data_ptr(), RATE["n_reads"], RATE["read_len"])  # (reserve: the table for the whole set, once)
    truth = sim.genome_counts(d_genome.cpu().numpy(), RATE["k"], canonical=True)
    del d_reads
    rows, (cols, in_genome) = counts.stats()[0], truth.stats()
    stream = torch.cuda.current_stream().cuda_stream
    d_out = torch.empty(rows * cols, dtype=torch.int64, device=dev)

    def scans():
        counts.histogram()
        truth.histogram()

    def timed(fn):
        fn()  # (discarded: code objects, the first scratch block)
        ms = [event_ms(fn) for _ in range(reps)]
        return statistics.median(ms), min(ms), max(ms)
    matrix = counts.join_histogram(truth, rows, cols)
    hist = counts.histogram()
    assert matrix[1:].sum(axis=1).tolist() == hist[1:] and int(matrix.sum()) == len(counts) + int(matrix[0].sum())
    scan = timed(scans)
    host = timed(lambda: counts.join_histogram(truth, rows, cols))
    device = timed(lambda: counts.join_histogram_device(truth, rows, cols, d_out.data_ptr(), stream=stream))
    assert (d_out.cpu().numpy().reshape(rows, cols) == matrix).all()
    lines.append("# cost (%s): %d reads of %d bases, k = %d canonical; reads' table %d slots, %d keys; genome's table %d slots, "
                 "%d keys; matrix %d x %d; HIP events, median (least, most) of %d after a discarded run; %s" % (
                     label, RATE["n_reads"], RATE["read_len"], RATE["k"], counts.slots, len(counts), truth.slots, in_genome,
                     rows, cols, reps, torch.cuda.get_device_name(0)))
    lines.append("  histogram() of both tables (the yardstick): %8.3f ms (%.3f, %.3f)" % scan)
    lines.append("  join_histogram, host form:                  %8.3f ms (%.3f, %.3f)   %.3f of the yardstick" % (host + (host[0] / scan[0],)))
    lines.append("  join_histogram_device alone:                %8.3f ms (%.3f, %.3f)   %.3f of the yardstick" % (device + (device[0] / scan[0],)))
    lines.append("  k-mers of the reads outside the genome %d, inside %d; of the genome unseen %d" % (
        int(matrix[1:, 0].sum()), int(matrix[1:, 1:].sum()), int(matrix[0].sum())))
    counts.close()
    truth.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="1-8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="", help="recovery or cost")
    ap.add_argument("--label", default="as built")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "copy_spectrum_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("copy_spectrum_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    a, b = (int(x) for x in args.seeds.split("-"))
    lines = []

    def write():  # after every part: a run that is cut short leaves what it had
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")

    if args.only in ("", "recovery"):
        recovery(range(a, b + 1), lines)
    if args.only in ("", "cost"):
        cost(args.reps, args.label, lines)
    write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
