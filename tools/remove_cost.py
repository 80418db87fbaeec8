"""What taking counts back out of the k-mer table costs -> profiles/remove_cost.txt.

    python tools/remove_cost.py [--reps 7] [--out profiles/remove_cost.txt]

1. remove_device against add_device: 6 * 10^6 reads of 100 bases (a 20 Mbp genome at coverage 30, 1 % errors), k = 21
   canonical -- section 6ak's workload --, resident in HBM, the table reserved once and holding the reads.  A round adds
   the reads a second time and takes them out again; HIP events around each call, median of `reps` rounds after a
   discarded one, one process.  The yardstick is the add of the same round.
2. leave_group_out_histograms by both routes: 10^6 random reads of 100 bases (10^8 bases: the workload behind the
   281.3 ms of profiles/jackknife_recovery.txt), k = 21, G = 32, host reads in and histograms out, median of `reps` after
   a discarded run, the routes alternating.  And how the remove route splits: its 32 x (uncount + count) alone under HIP
   events, and its 33 histogram scans alone by the host's clock (each waits for the device).

Run in a fresh process; torch is imported first (one HIP runtime a process).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from covest_amd import jackknife, simulate as sim  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402
from covest_amd.read_sets import ResidentReads  # noqa: E402

RATE = dict(genome_len=20_000_000, read_len=100, n_reads=6_000_000, k=21, seed=20261021)
SEED = 7


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(t):
    return "median %.3f ms, least %.3f, most %.3f, of %d" % (statistics.median(t), min(t), max(t), len(t))


def add_against_remove(reps, lines):
    dev = torch.device("cuda", 0)
    n, L, k = RATE["n_reads"], RATE["read_len"], RATE["k"]
    d_genome = torch.empty(RATE["genome_len"], dtype=torch.uint8, device=dev)
    sim.random_genome_device(d_genome.data_ptr(), RATE["genome_len"], RATE["seed"])
    d_reads = torch.empty(n * L, dtype=torch.uint8, device=dev)
    sim.simulate_reads_device(d_genome.data_ptr(), RATE["genome_len"], L, n, d_reads.data_ptr(), error_rate=0.01, seed=RATE["seed"])
    counts = KmerCounts(k, canonical=True)
    counts.add_device(d_reads.data_ptr(), n, L)  # (reserve: the table for the whole set, once)
    before = counts.stats()
    held, occupied = counts.occupancy()
    add, sub = [], []
    for i in range(reps + 1):
        a = timed_ms(lambda: counts.add_device(d_reads.data_ptr(), n, L, reserve=False))
        s = timed_ms(lambda: counts.remove_device(d_reads.data_ptr(), n, L))
        if i:  # (the first round is discarded)
            add.append(a)
            sub.append(s)
    assert counts.stats() == before and counts.occupancy() == (held, occupied)
    windows = n * (L - k + 1)
    lines.append("# 1. remove_device against add_device: %d reads of %d bases, k = %d canonical, %d windows a call; the table holds "
                 "the reads (%d keys in %d slots) and a round adds them again and takes them out; HIP events; %s"
                 % (n, L, k, windows, held, counts.slots, torch.cuda.get_device_name(0)))
    lines.append("  add_device     %s; %.2f windows/ns" % (spread(add), windows / (statistics.median(add) * 1e6)))
    lines.append("  remove_device  %s; %.2f windows/ns" % (spread(sub), windows / (statistics.median(sub) * 1e6)))
    lines.append("  remove / add   %.3f (medians); per round least %.3f, most %.3f"
                 % (statistics.median(sub) / statistics.median(add), min(s / a for s, a in zip(sub, add)),
                    max(s / a for s, a in zip(sub, add))))
    counts.close()
    del d_reads, d_genome
    torch.cuda.empty_cache()


def routes(reps, lines):
    n, L, k, groups = 10 ** 6, 100, 21, 32
    host = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, L))
    ms = {"recount": [], "remove": []}
    same = None
    for i in range(reps + 1):
        for route in ("recount", "remove"):
            got = []
            t = timed_ms(lambda: got.append(jackknife.leave_group_out_histograms(host, k, groups, seed=SEED, route=route)))
            if i:
                ms[route].append(t)
            elif route == "recount":
                same = got[0]
            else:
                assert got[0] == same, "the routes differ"
    lines.append("# 2. leave_group_out_histograms, %d bases of %d-base reads, k = %d, G = %d, host reads in, histograms out "
                 "(profiles/jackknife_recovery.txt has 281.3 ms for the recount route: for orientation only)" % (n * L, L, k, groups))
    lines.append("  route recount (upload, split, %d counts, %d clears)   %s" % (groups + 1, groups, spread(ms["recount"])))
    lines.append("  route remove  (upload, split, 1 count, %d x un/recount) %s" % (groups, spread(ms["remove"])))
    lines.append("  remove / recount %.3f (medians)" % (statistics.median(ms["remove"]) / statistics.median(ms["recount"])))
    # how the remove route splits: equal groups of consecutive ranks stand in for the split's (same sizes but for chance)
    with ResidentReads(host, k, False, -1, "remove_cost", "nothing else") as rs:
        rs.open_counter()
        rs.count(rs.d_in, None, 0, n)
        rs.histogram()
        cuts = [g * n // groups for g in range(groups + 1)]

        def un_and_recount():
            for g in range(groups):
                rs.uncount(rs.d_in, None, cuts[g], cuts[g + 1])
                rs.count(rs.d_in, None, cuts[g], cuts[g + 1])

        def scans():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(groups + 1):
                rs.histogram()
            return (time.perf_counter() - t0) * 1e3

        first = [timed_ms(lambda: rs.count(rs.d_in, None, 0, n)), timed_ms(lambda: rs.uncount(rs.d_in, None, 0, n))]
        un_and_recount()
        scans()
        moved = [timed_ms(un_and_recount) for _ in range(reps)]
        scanned = [scans() for _ in range(reps)]
        lines.append("  of the remove route: %d x (uncount + count) of a group  %s" % (groups, spread(moved)))
        lines.append("  of the remove route: %d histogram() calls (two scans each, %d slots; host clock)  %s"
                     % (groups + 1, rs.counts.slots, spread(scanned)))
        lines.append("  for scale: one count of all reads %.3f ms, one uncount of all reads %.3f ms" % (first[0], first[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "remove_cost.txt"))
    args = ap.parse_args()
    lines = ["# what a removal costs: HIP events, medians of %d after a discarded run, one process" % args.reps]
    add_against_remove(args.reps, lines)
    routes(args.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
