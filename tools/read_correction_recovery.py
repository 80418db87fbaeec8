"""Isolated substitutions corrected from the k-mer table, against the truth the simulator knows, and the loop closed:
reads -> count -> fit -> correct -> recount -> refit; nothing in the output is a pass mark.

  genome (random, --genome-len bases) -> simulate_reads_device at --coverage and --error-rate -> canonical k-mers into the
  table (add_device) -> histogram -> basic model fitted at sample factor 1 -> posterior error cutoff at --level ->
  correct_device into a second buffer -> the corrected reads against the same reads simulated at error rate 0 (their
  error-free twins) -> the corrected reads counted into a fresh counter -> histogram -> the model fitted again.

Printed: wrong bases before and after and the corrections to a base other than the true one, the four run totals, fitted
coverage and error rate before and after -- and correct_device's time beside lookup_device's (summary alone) and
add_device's on the same resident reads and table in the same run, each the median of --reps timings by device events
after a discarded warm-up (the add into a cleared table every time).

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/read_correction_recovery.py [--genome-len 20000000] [--coverage 30] [--k 21] [--out profiles/read_correction_recovery.txt]
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


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fitted(counts, k, read_len):
    """(histogram, estimate [coverage, error rate], success, model) of the basic model on the counter's histogram at
    sample factor 1: the table holds the abundances of the whole read set, so the model is fitted to them as they are."""
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    hist, tail, sample_factor, guess_c, guess_e = process_histogram(hist_orig, k, read_len, sample_factor=1)
    assert sample_factor == 1
    model = select_model("basic")(k, read_len, hist, tail, max_error=constants.MAX_ERRORS)
    estimate, success = CoverageEstimator(model).compute_coverage([guess_c, guess_e])
    return hist_orig, [float(v) for v in estimate], success, model


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "read_correction_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("read_correction_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    G, L, k = args.genome_len, args.read_len, args.k
    n = int(round(args.coverage * G / L))
    n_windows = n * (L - k + 1)
    lines = ["# isolated substitutions corrected from the k-mer table, against the simulator's truth: random genome %d, %d "
             "reads of %d bases (coverage %g), e = %g, k = %d canonical, seed %d; %s"
             % (G, n, L, args.coverage, args.error_rate, k, args.seed, torch.cuda.get_device_name(0))]

    d_genome = torch.empty(G, dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), G, args.seed, stream=stream)
    d_reads = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_clean = torch.empty(n * L, dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_reads.data_ptr(), error_rate=args.error_rate, seed=args.seed,
                              stream=stream)
    sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_clean.data_ptr(), error_rate=0.0, seed=args.seed, stream=stream)
    del d_genome

    # ---- the table: counted once untimed (it grows to its size here), then cleared and counted again --reps times ---------
    counts = KmerCounts(k, canonical=True)
    counts.add_device(d_reads.data_ptr(), n, L, stream=stream)
    torch.cuda.synchronize()
    add_ms = []
    for _ in range(args.reps):
        counts.clear(stream)
        add_ms.append(timed_ms(lambda: counts.add_device(d_reads.data_ptr(), n, L, stream=stream, reserve=False)))
    hist_before, before, success, model = fitted(counts, k, L)
    lines.append("# table: %d slots of 16 bytes (%.2f GB), %d distinct k-mers, %d of them counted once"
                 % (counts.slots, counts.slots * 16 / 1e9, len(counts), hist_before.get(1, 0)))
    cutoff = posterior_classes(model, before).error_cutoff(args.level)
    model.close()
    lines.append("# fit before: coverage %.4f (per base %.4f), error rate %.5f, success %s; error cutoff at level %g: %s"
                 % (before[0], n * L / G, before[1], success, args.level, cutoff))
    if cutoff is None:
        raise SystemExit("the posterior classes give no error cutoff")

    # ---- the correction beside the lookup's summary: the same reads, the same table ---------------------------------------
    d_out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_fix = torch.empty(4 * n, dtype=torch.int32, device=dev)
    d_summary = torch.empty(4 * n, dtype=torch.int32, device=dev)

    def correct():
        counts.correct_device(d_reads.data_ptr(), n, L, d_out.data_ptr(), cutoff=cutoff, d_fix_ptr=d_fix.data_ptr(), stream=stream)

    def lookup_summary():
        counts.lookup_device(d_reads.data_ptr(), n, L, cutoff=cutoff, d_summary_ptr=d_summary.data_ptr(), stream=stream)

    ms = {}
    for name, fn in (("lookup_device, summary alone", lookup_summary), ("correct_device", correct)):
        fn()  # warm-up, discarded
        torch.cuda.synchronize()
        ms[name] = [timed_ms(fn) for _ in range(args.reps)]
    del d_summary
    counts.close()

    # ---- against the truth ----------------------------------------------------------------------------------------------
    wrong_before, wrong_after, changed = d_reads != d_clean, d_out != d_clean, d_out != d_reads
    n_before, n_after = int(wrong_before.sum().item()), int(wrong_after.sum().item())
    miscorrected = int((changed & wrong_after).sum().item())
    reads_before = int(wrong_before.view(n, L).any(dim=1).sum().item())
    reads_after = int(wrong_after.view(n, L).any(dim=1).sum().item())
    worse = int((wrong_after.view(n, L).sum(dim=1) > wrong_before.view(n, L).sum(dim=1)).sum().item())
    totals = d_fix.cpu().numpy().view(np.uint32).reshape(n, 4).astype(np.int64).sum(axis=0)
    n_changed = int(changed.sum().item())
    del wrong_before, wrong_after, changed, d_clean, d_reads
    torch.cuda.empty_cache()
    lines.append("  runs of weak windows %d: corrected %d (%.5f), ambiguous %d, unfixable %d; bytes changed %d"
                 % (totals[0], totals[1], totals[1] / max(int(totals[0]), 1), totals[2], totals[3], n_changed))
    lines.append("  wrong bases %d -> %d; corrections to a base other than the true one %d" % (n_before, n_after, miscorrected))
    lines.append("  reads with a wrong base %d -> %d of %d; reads with more wrong bases after than before %d"
                 % (reads_before, reads_after, n, worse))

    # ---- recount the corrected reads into a fresh counter, refit ----------------------------------------------------------
    recount = KmerCounts(k, canonical=True)
    recount.add_device(d_out.data_ptr(), n, L, stream=stream)
    torch.cuda.synchronize()
    hist_after, after, success, model = fitted(recount, k, L)
    cutoff_after = posterior_classes(model, after).error_cutoff(args.level)
    model.close()
    lines.append("# recount: %d distinct k-mers, %d of them counted once" % (len(recount), hist_after.get(1, 0)))
    lines.append("# fit after: coverage %.4f, error rate %.5f, success %s; error cutoff at level %g: %s"
                 % (after[0], after[1], success, args.level, cutoff_after))
    lines.append("  fitted coverage %.4f -> %.4f; fitted error rate %.5f -> %.5f (wrong bases a base: %.5f -> %.5f)"
                 % (before[0], after[0], before[1], after[1], n_before / (n * L), n_after / (n * L)))
    recount.close()

    lines.append("# times: median of %d by device events after a discarded warm-up; %d windows" % (args.reps, n_windows))
    lines.append("# %-32s %10s %14s" % ("route", "ms", "1e9 windows/s"))
    rows = [("add_device (cleared table)", add_ms)] + list(ms.items())
    for name, values in rows:
        t = statistics.median(values)
        lines.append("  %-32s %10.3f %14.3f" % (name, t, n_windows / (t * 1e-3) / 1e9))
    lines.append("  correct_device / lookup_device   %10.3f" % (statistics.median(ms["correct_device"]) /
                                                                statistics.median(ms["lookup_device, summary alone"])))
    for name, values in rows:
        lines.append("#   all timings, ms: %s: %s" % (name, " ".join("%.2f" % v for v in values)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
