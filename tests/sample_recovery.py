"""One whole estimate from simulated reads that went through the sampler, against the sample's own truth (TEST
INFRASTRUCTURE ONLY; not collected): the loop of tests/sim_recovery.py at twice its coverage with the sampler at factor 2
in between.  tools/sample_recovery.py records it for a range of seeds."""
COVERAGE, FACTOR = 40, 2


def recover(seed, coverage=COVERAGE, factor=FACTOR):
    """The loop of tests/sim_recovery.py with the sampler in between: {quantity: (truth, estimate, relative deviation)},
    the truth being the sample's: c = n_kept L / genome_len, e = substitutions among the kept reads / (n_kept L)."""
    from flow_helper import estimate
    from sim_recovery import LOOP
    from covest_amd import kmer_hist as kh, sample, simulate as sim
    g = sim.random_genome(LOOP["genome_len"], seed)
    reads = sim.simulate_reads(g, LOOP["read_len"], coverage=coverage, error_rate=LOOP["error_rate"], seed=seed)
    half = sample.sample_reads(reads, factor, seed=seed)
    counts = half.add_to(kh.KmerCounts(LOOP["k"], canonical=True))
    hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    reads_size = half.n_bases
    rec = estimate(hist, kmer_size=LOOP["k"], read_length=LOOP["read_len"], model="basic", reads_size=reads_size)
    truth = {"coverage": reads_size / LOOP["genome_len"], "error_rate": half.substitutions(g) / reads_size,
             "genome_size": LOOP["genome_len"], "genome_size_reads": LOOP["genome_len"]}
    return {q: (t, rec[q], abs(rec[q] - t) / t) for q, t in truth.items()}
