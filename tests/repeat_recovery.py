"""One whole estimate of the REPEAT model from simulated reads against a measured truth (TEST INFRASTRUCTURE ONLY; not
collected): repeat genome -> reads (covest_amd.simulate) -> forward-strand 21-mer histogram -> tests/flow_helper.estimate,
repeats model.  tools/repeat_recovery.py records it for a range of seeds."""
LOOP = dict(genome_len=300_000, unit_len=250, q1=0.7, q2=0.5, q=0.5, divergence=0.0, read_len=100, coverage=20,
            error_rate=0.01, k=21)
RELATIVE = ("coverage", "error_rate", "genome_size", "genome_size_reads")  # the others: absolute deviations


def recover(seed):
    """{quantity: (truth, estimate, deviation)}: c = n_reads L / genome_len, e = realised substitutions / (n_reads L),
    genome size 300 000 (from the histogram, and from reads_size = n_reads L) -- relative deviations --, and (q1, q2, q)
    = spectrum_to_q of the genome's own forward-strand 21-mer spectrum -- absolute deviations.  The reads come from the
    forward strand only, as the k-mers are counted."""
    from flow_helper import estimate
    from covest_amd import kmer_hist as kh, simulate as sim
    g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], seed,
                          divergence=LOOP["divergence"])
    reads = sim.simulate_reads(g.bases, LOOP["read_len"], coverage=LOOP["coverage"], error_rate=LOOP["error_rate"], seed=seed,
                               both_strands=False)
    counts = reads.add_to(kh.KmerCounts(LOOP["k"], canonical=False))
    hist = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    reads_size = reads.n_reads * reads.read_length
    rec = estimate(hist, kmer_size=LOOP["k"], read_length=LOOP["read_len"], model="repeats", reads_size=reads_size)
    q1, q2, q = sim.spectrum_to_q(sim.genome_spectrum(g, LOOP["k"], canonical=False))
    truth = {"coverage": reads.true_coverage, "error_rate": reads.substitutions(g.bases) / reads_size,
             "genome_size": LOOP["genome_len"], "genome_size_reads": LOOP["genome_len"], "q1": q1, "q2": q2, "q": q}
    return {name: (t, rec[name], abs(rec[name] - t) / (t if name in RELATIVE else 1.0)) for name, t in truth.items()}
