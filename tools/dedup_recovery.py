"""The duplicate remover (covest_amd/dedup.py): what it costs beside a pure compaction and beside
the k-mer count, and what it does to the estimates of read sets that carry copies; nothing in the output is a pass mark.

  cost      6 * 10^6 reads of 100 bases resident in HBM (a 20 Mbp genome at coverage 30, error rate 0.01); every read
            given one extra copy with probability 0 or 0.3 (numpy on the host, the copies shuffled in, the set cut back
            to 6 * 10^6 reads); the median of 7 runs of dedup_reads_device, forward and with the reverse complement;
            beside it, in the same run, sample_reads_device at factor 1 (a pure compaction of the same bytes) and an
            unweighted clear + add_device + histogram at k = 21.  Host wall clock around calls that wait for the device.
  estimate  one random genome of 1 Mbp, 100-base reads at coverage 10, error rate 0.01, both strands; every read given
            one extra copy with probability 0, 0.1 or 0.3, the copies shuffled in; k = 21 canonical; basic model and
            repeats model; coverage, error rate and genome size of the raw and of the deduplicated reads (forward only)
            against the simulator's truth.  At probability 0: the share of reads the call drops although nobody copied
            them (chance coincidences of start, strand and errors, of the order of c / 2L per read), and the shift of
            the coverage estimate that causes.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/dedup_recovery.py [--sets 3] [--out profiles/dedup_recovery.txt]
"""
import argparse
import ctypes
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
from covest_amd import constants, simulate as sim  # noqa: E402
from covest_amd.dedup import dedup_reads, dedup_reads_device  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402
from covest_amd.sample import sample_reads_device  # noqa: E402

RATE = dict(genome_len=20_000_000, read_len=100, n_reads=6_000_000, k=21, seed=20261021)
BASIC = dict(genome_len=1_000_000, read_len=100, coverage=10, error_rate=0.01, k=21)


def with_copies(rows, p, rng):
    """`rows` ((n, L) uint8) with one extra copy of every read with probability p, the copies shuffled in."""
    if p == 0:
        return rows
    extra = rows[rng.random(rows.shape[0]) < p]
    both = np.concatenate([rows, extra])
    return both[rng.permutation(both.shape[0])]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, reps):
    fn()  # (discarded: code objects, the first scratch block)
    ms = [wall_ms(fn) for _ in range(reps)]
    return statistics.median(ms), ms


def cost(reps, lines):
    dev = torch.device("cuda", 0)
    n, L, k = RATE["n_reads"], RATE["read_len"], RATE["k"]
    d_genome = torch.empty(RATE["genome_len"], dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), RATE["genome_len"], RATE["seed"])
    d_plain = torch.empty(n * L, dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), RATE["genome_len"], L, n, d_plain.data_ptr(), error_rate=0.01, seed=RATE["seed"])
    rows = d_plain.cpu().numpy().reshape(n, L)
    rng = np.random.default_rng(RATE["seed"])
    d_out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_kept = torch.empty(n, dtype=torch.int64, device=dev)
    d_copies = torch.empty(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(3, dtype=torch.int64, device=dev)
    lines.append("# cost: %d reads of %d bases resident in HBM, the median of %d runs after a discarded one; host wall clock; %s"
                 % (n, L, reps, torch.cuda.get_device_name(0)))
    for share in (0.0, 0.3):
        d_reads = d_plain if share == 0 else torch.from_numpy(np.ascontiguousarray(with_copies(rows, share, rng)[:n])).to(dev)
        medians = {}
        for rc in (False, True):
            name = "dedup_reads_device, %s" % ("reverse complement" if rc else "forward")
            medians[rc], ms = timed(lambda: dedup_reads_device(
                d_reads.data_ptr(), n, d_out.data_ptr(), d_counts.data_ptr(), reverse_complement=rc, seed=1, read_len=L,
                kept_ptr=d_kept.data_ptr(), copies_ptr=d_copies.data_ptr()), reps)
            kept, bases, collided = d_counts.cpu().tolist()
            lines.append("  copies with probability %.1f: %-44s median %7.2f ms (all: %s); kept %d of %d, dropped share %.4f, "
                         "collided %d" % (share, name, medians[rc], " ".join("%.2f" % v for v in ms), kept, n, 1 - kept / n, collided))
        compaction, ms = timed(lambda: sample_reads_device(d_reads.data_ptr(), n, d_out.data_ptr(), d_counts.data_ptr(), 1,
                                                           seed=1, read_len=L, kept_ptr=d_kept.data_ptr()), reps)
        lines.append("  copies with probability %.1f: %-44s median %7.2f ms (all: %s)" % (
            share, "sample_reads_device at factor 1", compaction, " ".join("%.2f" % v for v in ms)))
        counts = KmerCounts(k, canonical=True)
        counts.add_device(d_reads.data_ptr(), n, L)  # (reserve: the table for the whole set, once)
        counts.histogram()

        def count():
            counts.clear()
            counts.add_device(d_reads.data_ptr(), n, L, reserve=False)
            counts.histogram()
        counting, ms = timed(count, reps)
        counts.close()
        lines.append("  copies with probability %.1f: %-44s median %7.2f ms (all: %s)" % (
            share, "clear + add_device + histogram, k = %d" % k, counting, " ".join("%.2f" % v for v in ms)))
        for rc in (False, True):
            lines.append("  copies with probability %.1f: dedup (%s) / compaction %.2f, dedup / count %.3f" % (
                share, "reverse complement" if rc else "forward", medians[rc] / compaction, medians[rc] / counting))
        del d_reads


def fit(rows, k, model_name):
    """(estimate, success, genome size) of one read set ((n, L) uint8): canonical k-mers, sample factor 1, the cut of
    process_histogram (none up to abundance MAX_NOTRIM), as tools/jackknife_recovery.py fits."""
    from covest_amd.estimator import CoverageEstimator
    from covest_amd.hist_steps import MAX_NOTRIM, compute_coverage_apx, get_trim, trim_hist
    from covest_amd.models import select_model
    n, L = rows.shape
    blob = np.ascontiguousarray(rows).reshape(-1)
    offsets = np.arange(n + 1, dtype=np.int64) * L
    counts = KmerCounts(k, canonical=True)
    counts.add_packed(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                      n, blob.size)
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    trim = get_trim(hist_orig, ignore_last=True) if max(hist_orig) > MAX_NOTRIM else None
    hist, tail = trim_hist(hist_orig, trim) if trim is not None else (hist_orig, 0)
    model = select_model(model_name)(k, L, hist, tail, max_error=constants.MAX_ERRORS, max_cov=None,
                                     min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
    guess = list(model.defaults)
    c, e = compute_coverage_apx(hist_orig, k, L)
    if not (c == 0 and e == 1):
        guess[:2] = c, e
    est, ok = CoverageEstimator(model).compute_coverage(guess)
    occurrences = sum(i * v for i, v in hist_orig.items())
    size = occurrences / model.correct_c(est[0])
    model.close()
    return [float(v) for v in est], bool(ok), float(size)


def estimates(sets, lines):
    k, L = BASIC["k"], BASIC["read_len"]
    genome = sim.random_genome(BASIC["genome_len"], 1)
    lines.append("# estimate: random genome %(genome_len)d, L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, both strands, "
                 "k = %(k)d canonical; raw reads and dedup_reads(reads) (forward only) against the simulator's truth" % BASIC)
    lines.append("# %-4s %-5s %-8s %-6s %9s %9s %12s %12s %12s %10s %10s %10s %7s" % (
        "set", "p", "model", "reads", "n reads", "dropped", "coverage", "error rate", "genome size", "c / truth", "e / truth",
        "G / truth", "success"))
    for seed in range(1, sets + 1):
        reads = sim.simulate_reads(genome, L, coverage=BASIC["coverage"], error_rate=BASIC["error_rate"], seed=seed)
        truth_c, truth_e = reads.true_coverage, reads.substitutions(genome) / (reads.n_reads * L)
        rng = np.random.default_rng(seed)
        for p in (0.0, 0.1, 0.3):
            raw = with_copies(reads.bases, p, rng)
            t0 = time.perf_counter()
            unique = dedup_reads(raw)
            dedup_s = time.perf_counter() - t0
            dropped = raw.shape[0] - unique.n_reads
            for model_name in ("basic", "repeats"):
                row = {}
                for label, rows in (("raw", raw), ("dedup", unique.bases)):
                    est, ok, size = fit(rows, k, model_name)
                    row[label] = est
                    lines.append("  %-4d %-5.1f %-8s %-6s %9d %9d %12.6f %12.6f %12.0f %10.4f %10.4f %10.4f %7s" % (
                        seed, p, model_name, label, rows.shape[0], dropped if label == "dedup" else 0, est[0], est[1], size,
                        est[0] / truth_c, est[1] / truth_e, size / len(genome), ok))
                if p == 0:
                    lines.append("#   set %d, %s, nobody copied a read: %d of %d reads dropped (share %.5f; c / 2L = %.5f); coverage "
                                 "%.6f -> %.6f, a shift of %+.4f %%" % (
                                     seed, model_name, dropped, raw.shape[0], dropped / raw.shape[0], truth_c / (2 * L),
                                     row["raw"][0], row["dedup"][0], 100.0 * (row["dedup"][0] / row["raw"][0] - 1)))
            lines.append("#   set %d, p = %.1f: truth c %.6f, e %.6f; copies %s; rounds %d, collided %d; dedup_reads (host form, "
                         "copies included) %.2f s" % (seed, p, truth_c, truth_e, unique.copies_histogram(), unique.rounds,
                                                     unique.collided, dedup_s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", default="", help="comma-separated: cost, estimate")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dedup_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dedup_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    skip = set(args.skip.split(","))
    lines = ["# duplicate reads removed on the device: the cost beside a compaction and a k-mer count, and the estimates of "
             "read sets with copies, raw and deduplicated"]

    def write():  # after every part: a run that is cut short leaves what it had
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if "cost" not in skip:
        cost(args.reps, lines)
        write()
    if "estimate" not in skip:
        estimates(args.sets, lines)
        write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
