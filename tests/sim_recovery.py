"""One whole estimate from simulated reads against the exact truth (TEST INFRASTRUCTURE ONLY; not collected):
genome -> reads (covest_amd.simulate) -> canonical 21-mer histogram -> tests/flow_helper.estimate, basic model.
tools/simulate_recovery.py records it for a range of seeds."""
LOOP = dict(genome_len=200_000, read_len=100, coverage=20, error_rate=0.02, k=21)


def recover(seed):
    """{quantity: (truth, estimate, relative deviation)}: c = n_reads L / genome_len, e = realised substitutions /
    (n_reads L), genome size 200 000 (from the histogram, and from reads_size = n_reads L)."""
    from flow_helper import estimate
    from covest_amd import kmer_hist as kh, simulate as sim
    g = sim.random_genome(LOOP["genome_len"], seed)
    reads = sim.simulate_reads(g, LOOP["read_len"], coverage=LOOP["coverage"], error_rate=LOOP["error_rate"], seed=seed)
    counts = reads.add_to(kh.KmerCounts(LOOP["k"], canonical=True))
    hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    reads_size = reads.n_reads * reads.read_length
    rec = estimate(hist, kmer_size=LOOP["k"], read_length=LOOP["read_len"], model="basic", reads_size=reads_size)
    truth = {"coverage": reads.true_coverage, "error_rate": reads.substitutions(g) / reads_size,
             "genome_size": LOOP["genome_len"], "genome_size_reads": LOOP["genome_len"]}
    return {q: (t, rec[q], abs(rec[q] - t) / t) for q, t in truth.items()}
