"""Which reads carry errors, against the truth the simulator knows; nothing in the output is a
pass mark.

  genome (random, --genome-len bases) -> simulate_reads_device at --coverage and --error-rate -> canonical k-mers into the
  table (add_device) -> histogram -> basic model fitted -> posterior error cutoff at --level -> lookup_device -> the flags
  against the reads' realised substitutions (the same reads simulated at error rate 0 are their error-free twins).

Printed: sensitivity and specificity of "the read has a k-mer below the cutoff", the share of the reads with exactly one
substitution whose base locate_single_errors names, the flagged share beside the model's predicted share -- and the
lookup's windows/s beside add_device's k-mers/s on the same resident reads in the same run, each the median of --reps
timings by device events after a discarded warm-up (the add into a cleared table every time).

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/read_error_recovery.py [--genome-len 20000000] [--coverage 30] [--k 21] [--out profiles/read_error_recovery.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from covest_amd import constants, simulate as sim  # noqa: E402
from covest_amd.estimator import CoverageEstimator  # noqa: E402
from covest_amd.hist_steps import process_histogram  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402
from covest_amd.models import select_model  # noqa: E402
from covest_amd.posterior import posterior_classes  # noqa: E402
from covest_amd.read_errors import ReadErrorScores, abundance_weights  # noqa: E402


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def signed(column):
    out = column.astype(np.int64)
    out[column == 0xFFFFFFFF] = -1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-len", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--level", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "read_error_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("read_error_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    G, L, k = args.genome_len, args.read_len, args.k
    n = int(round(args.coverage * G / L))
    n_windows = n * (L - k + 1)
    lines = ["# read errors against the simulator's truth: random genome %d, %d reads of %d bases (coverage %g), e = %g, k = %d "
             "canonical, seed %d; %s" % (G, n, L, args.coverage, args.error_rate, k, args.seed, torch.cuda.get_device_name(0))]

    d_genome = torch.empty(G, dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), G, args.seed, stream=stream)
    d_reads = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_clean = torch.empty(n * L, dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_reads.data_ptr(), error_rate=args.error_rate, seed=args.seed,
                              stream=stream)
    sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_clean.data_ptr(), error_rate=0.0, seed=args.seed, stream=stream)
    hit = (d_reads != d_clean).view(n, L)
    per_read = hit.sum(dim=1)
    wrong = (per_read > 0).cpu().numpy()
    single = (per_read == 1).cpu().numpy()
    truth_at = hit.to(torch.int32).argmax(dim=1).cpu().numpy()
    realised = float(per_read.sum().item()) / (n * L)
    del d_clean, hit, per_read
    torch.cuda.empty_cache()

    # ---- the table: counted once untimed (it grows to its size here), then cleared and counted again --reps times ---------
    counts = KmerCounts(k, canonical=True)
    counts.add_device(d_reads.data_ptr(), n, L, stream=stream)
    torch.cuda.synchronize()
    add_ms = []
    for _ in range(args.reps):
        counts.clear(stream)
        add_ms.append(timed_ms(lambda: counts.add_device(d_reads.data_ptr(), n, L, stream=stream, reserve=False)))
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    distinct = len(counts)
    lines.append("# table: %d slots of 16 bytes (%.2f GB), %d distinct k-mers" % (counts.slots, counts.slots * 16 / 1e9, distinct))

    # ---- histogram -> fit -> posterior cutoff ---------------------------------------------------------------------------
    # (sample factor 1: the table holds the abundances of the whole read set, so the model is fitted to them as they are)
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, k, L, sample_factor=1)
    model = select_model("basic")(k, L, hist, tail, max_error=constants.MAX_ERRORS)
    estimate, success = CoverageEstimator(model).compute_coverage([guess_c, guess_e])
    estimate = [float(v) for v in estimate]
    posterior = posterior_classes(model, estimate)
    cutoff = posterior.error_cutoff(args.level)
    lines.append("# fit: sample factor %d, coverage %.4f (per base %.4f), error rate %.5f (realised %.5f), success %s; "
                 "error cutoff at level %g: %s" % (sample_factor, estimate[0], n * L / G, estimate[1], realised, success,
                                                   args.level, cutoff))
    if cutoff is None:
        raise SystemExit("the posterior classes give no error cutoff")
    weights = abundance_weights(posterior, "erroneous")
    d_weights = torch.from_numpy(weights).to(dev)

    # ---- the lookup: all three outputs, and the summary alone ------------------------------------------------------------
    d_abundance = torch.empty(n * L, dtype=torch.int32, device=dev)
    d_summary = torch.empty(4 * n, dtype=torch.int32, device=dev)
    d_score = torch.empty(n, dtype=torch.float64, device=dev)

    def lookup_all():
        counts.lookup_device(d_reads.data_ptr(), n, L, cutoff=cutoff, d_weights_ptr=d_weights.data_ptr(), n_weights=weights.size,
                             d_abundance_ptr=d_abundance.data_ptr(), d_summary_ptr=d_summary.data_ptr(),
                             d_score_ptr=d_score.data_ptr(), stream=stream)

    def lookup_summary():
        counts.lookup_device(d_reads.data_ptr(), n, L, cutoff=cutoff, d_summary_ptr=d_summary.data_ptr(), stream=stream)

    lookup_ms = {}
    for name, fn in (("abundance + summary + score", lookup_all), ("summary alone", lookup_summary)):
        fn()  # warm-up, discarded
        torch.cuda.synchronize()
        lookup_ms[name] = [timed_ms(fn) for _ in range(args.reps)]
    lookup_all()
    torch.cuda.synchronize()
    summary = d_summary.cpu().numpy().view(np.uint32).reshape(n, 4)
    score = d_score.cpu().numpy()

    # ---- against the truth ----------------------------------------------------------------------------------------------
    scores = ReadErrorScores(k, np.full(n, L), *(signed(summary[:, j]) for j in range(4)), score, cutoff, args.level,
                             estimate[1], weights=weights)
    flagged = scores.flagged
    missed, false = int((wrong & ~flagged).sum()), int((~wrong & flagged).sum())
    n_wrong, n_clean = int(wrong.sum()), int((~wrong).sum())
    located = scores.locate_single_errors()
    right = int((single & (located == truth_at)).sum())
    undecided = int((single & (located < 0)).sum())
    n_single = int(single.sum())
    lines.append("  reads with a substitution %d of %d, flagged %d, missed %d, falsely flagged %d" % (n_wrong, n, int(flagged.sum()),
                                                                                                  missed, false))
    lines.append("  sensitivity %.5f  specificity %.5f" % (1 - missed / max(n_wrong, 1), 1 - false / max(n_clean, 1)))
    lines.append("  reads with exactly one substitution %d: located right %d (%.5f), wrong %d, undecided %d" % (
        n_single, right, right / max(n_single, 1), n_single - right - undecided, undecided))
    lines.append("  flagged share %.5f  predicted share 1 - (1 - e)^L %.5f (the model's share of reads with a wrong base, not the "
                 "detector's expectation)  true share %.5f" % (scores.flagged_share, scores.predicted_share, n_wrong / n))
    lines.append("  mean expected erroneous k-mers a read %.4f" % float(score.mean()))
    lines.append("# rates: median of %d by device events after a discarded warm-up; %d windows" % (args.reps, n_windows))
    lines.append("# %-32s %10s %14s" % ("route", "ms", "1e9 windows/s"))
    t = statistics.median(add_ms)
    lines.append("  %-32s %10.3f %14.3f" % ("add_device (cleared table)", t, n_windows / (t * 1e-3) / 1e9))
    for name, ms in lookup_ms.items():
        t = statistics.median(ms)
        lines.append("  %-32s %10.3f %14.3f" % ("lookup_device, " + name, t, n_windows / (t * 1e-3) / 1e9))
    lines.append("#   all timings, ms: add %s" % " ".join("%.2f" % v for v in add_ms))
    for name, ms in lookup_ms.items():
        lines.append("#   all timings, ms: lookup, %s: %s" % (name, " ".join("%.2f" % v for v in ms)))
    counts.close()
    model.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
