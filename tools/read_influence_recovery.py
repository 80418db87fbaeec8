"""The linearised delete-one jackknife (covest_amd/influence.py) beside what section 6aa measured;
nothing in the output is a pass mark.

  On the two cases of tools/jackknife_recovery.py (basic, repeats), read sets 1 .. 4: the linearised standard errors
  beside read_jackknife's at G groups, the model's Wald error and the empirical standard deviation over independent read
  sets that profiles/jackknife_recovery.txt records (read from that file; "none" where it is not there).
  And the direct test of section 6aa's supposition about the basic model: per parameter, the correlation over the G groups
  between A^-1 sum_{r in g} Delta_r (groups from sample.read_groups) and the actual leave-out shift of the refit,
  estimates[g] - full_estimate, with the ratio of their root mean squares.

  The rates: 6 * 10^6 reads of 100 bases (a 20 Mbp genome at coverage 30), k = 21 canonical, the 2^30-slot table; at P = 2
  and P = 5 table columns, read_influence_device + the two moments calls against P calls of lookup_device with a score
  -- the only route the parent commit has, and it gives the m = 1 part alone.  Medians of --reps by device events after
  a discarded warm-up.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/read_influence_recovery.py [--groups 32] [--out profiles/read_influence_recovery.txt]
"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from covest_amd import influence, jackknife, sample, simulate as sim  # noqa: E402
from covest_amd.information import genome_size_se  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402
from jackknife_recovery import BASIC, QUANTITIES, fit, timed_ms  # noqa: E402
from repeat_recovery import LOOP  # noqa: E402


def empirical_sd(name):
    """{quantity: the empirical sd} of case `name` as profiles/jackknife_recovery.txt records it."""
    out = {}
    try:
        with open(os.path.join(REPO, "profiles", "jackknife_recovery.txt")) as f:
            for line in f:
                m = re.match(r"  (\w+) +(\w+) +(\S+) +(\S+) ", line)
                if m and m.group(1) == name and m.group(2) in QUANTITIES:
                    out[m.group(2)] = float(m.group(4))
    except OSError:
        pass
    return out


def recovery(name, genome, settings, model_name, groups, lines):
    k, L = settings["k"], settings["read_len"]
    emp = empirical_sd(name)
    lines.append("# %s: standard errors from ONE read set; empirical sd over independent sets from profiles/jackknife_recovery.txt"
                 % name)
    lines.append("# %-8s %3s %-12s %12s %12s %12s %12s %10s %10s" % ("case", "set", "quantity", "linearised", "jackknife G",
                                                                   "Wald", "empirical sd", "lin/jack", "lin/emp"))
    for seed in range(1, 5):
        reads = sim.simulate_reads(genome, L, coverage=settings["coverage"], error_rate=settings["error_rate"], seed=seed,
                                   both_strands=False)
        model, est, ok, hist_orig, trim = fit(reads, k, model_name)
        counts = reads.add_to(KmerCounts(k, canonical=False))
        infl = influence.read_influence(model, est, counts, reads)
        counts.close()
        summary = infl.summary()
        jack = jackknife.read_jackknife(model, est, reads, groups=groups, seed=seed, trim=trim)
        size = genome_size_se(model, hist_orig, infl.info)
        wald = dict(infl.info["standard_errors"], genome_size=size["genome_size_se"])
        if summary["reason"] is not None:
            lines.append("  %-8s %3d no linearised error: %s" % (name, seed, summary["reason"]))
            model.close()
            continue
        for q in list(model.params) + ["genome_size"]:
            lin, jk, w, e = summary["standard_errors"][q], jack["standard_errors"][q], wald.get(q), emp.get(q)
            lines.append("  %-8s %3d %-12s %12s %12s %12s %12s %10s %10s" % (
                name, seed, q, *("%.4g" % v if v is not None else "none" for v in (lin, jk, w, e)),
                "%.3f" % (lin / jk) if lin is not None and jk else "none", "%.3f" % (lin / e) if lin is not None and e else "none"))
        # the groups' summed linear shifts against the refits' actual ones (the parameters as refitted: nothing rescaled)
        P = len(model.params)
        group = sample.read_groups(reads.n_reads, groups, seed=seed, first_read=int(reads.first_read))
        shifts = infl.shifts()[:, :P] - (infl.rows[:, P:] * (est[0] / infl.occurrences_full)) * (np.arange(P) == 0)
        predicted = np.array([shifts[group == g].sum(axis=0) for g in range(groups)])
        actual = np.asarray(jack["estimates"]) - np.asarray(jack["full_estimate"])[None, :]
        good = np.asarray(jack["success"], dtype=bool)
        for d, q in enumerate(model.params):
            a, p = actual[good, d], predicted[good, d]
            if a.std() == 0 or p.std() == 0:
                lines.append("  %-8s %3d groups  %-12s no spread" % (name, seed, q))
                continue
            lines.append("  %-8s %3d groups  %-12s correlation %.4f rms predicted / rms actual %.3f (%d groups)" % (
                name, seed, q, float(np.corrcoef(a, p)[0, 1]), float(np.sqrt((p ** 2).mean() / (a ** 2).mean())), int(good.sum())))
        model.close()


def rates(reps, lines):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    G, L, k, n = 20_000_000, 100, 21, 6_000_000
    d_genome = torch.empty(G, dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), G, 20261020, stream=stream)
    d_reads = torch.empty(n * L, dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), G, L, n, d_reads.data_ptr(), error_rate=0.01, seed=20261020, stream=stream)
    counts = KmerCounts(k, canonical=True)
    counts.add_device(d_reads.data_ptr(), n, L, stream=stream)
    torch.cuda.synchronize()
    lines.append("# rates: %d reads of %d bases, k = %d canonical, %d slots; median of %d by device events after a discarded "
                 "warm-up; %s" % (n, L, k, counts.slots, reps, torch.cuda.get_device_name(0)))
    lines.append("# %-44s %10s" % ("route", "ms"))
    rng = np.random.default_rng(1)
    for P in (2, 5):
        table = torch.from_numpy(rng.normal(size=(64, P))).to(dev)
        columns = [table[:, j].contiguous() for j in range(P)]
        rows = torch.empty(n * (P + 1), dtype=torch.float64, device=dev)
        scores = torch.empty((P, n), dtype=torch.float64, device=dev)
        centre = torch.zeros(P + 1, dtype=torch.float64, device=dev)
        total = torch.empty(P + 1, dtype=torch.float64, device=dev)
        cross = torch.empty((P + 1) * (P + 2) // 2, dtype=torch.float64, device=dev)

        def influence_route():
            counts.read_influence_device(d_reads.data_ptr(), n, L, table.data_ptr(), 64, P, rows.data_ptr(), stream=stream)
            influence.rows_moments_device(rows.data_ptr(), n, P + 1, centre.data_ptr(), total.data_ptr(), cross.data_ptr(), stream)
            influence.rows_moments_device(rows.data_ptr(), n, P + 1, centre.data_ptr(), total.data_ptr(), cross.data_ptr(), stream)

        def influence_alone():
            counts.read_influence_device(d_reads.data_ptr(), n, L, table.data_ptr(), 64, P, rows.data_ptr(), stream=stream)

        def lookup_route():
            for j in range(P):
                counts.lookup_device(d_reads.data_ptr(), n, L, d_weights_ptr=columns[j].data_ptr(), n_weights=64,
                                     d_score_ptr=scores[j].data_ptr(), stream=stream)

        ms = {}
        for name, fn in (("read_influence_device + 2 x moments", influence_route), ("read_influence_device alone", influence_alone),
                         ("%d x lookup_device with a score (m = 1 part)" % P, lookup_route)):
            fn()
            torch.cuda.synchronize()
            ms[name] = [timed_ms(fn) for _ in range(reps)]
            lines.append("  P = %d %-38s %10.3f   all: %s" % (P, name, statistics.median(ms[name]),
                                                               " ".join("%.2f" % v for v in ms[name])))
        names = list(ms)
        lines.append("  P = %d ratio influence + moments / %d lookups: %.3f" % (
            P, P, statistics.median(ms[names[0]]) / statistics.median(ms[names[2]])))
    counts.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated: basic, repeats, rates")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "read_influence_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("read_influence_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    skip = set(args.skip.split(","))
    lines = ["# the linearised delete-one-read jackknife beside the delete-a-group jackknife at G = %d, the Wald error and the "
             "empirical spread of section 6aa" % args.groups]

    def write():  # after every part: a run that is cut short leaves what it had
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    if "rates" not in skip:
        rates(args.reps, lines)
        write()
    if "basic" not in skip:
        recovery("basic", sim.random_genome(BASIC["genome_len"], 1), BASIC, "basic", args.groups, lines)
        write()
    if "repeats" not in skip:
        g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], 1,
                              divergence=LOOP["divergence"])
        recovery("repeats", g.bases, LOOP, "repeats", args.groups, lines)
        write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
