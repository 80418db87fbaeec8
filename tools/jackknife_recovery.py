"""What nobody had measured: the spread of the estimate over INDEPENDENT read sets of one genome, beside the two standard
errors the project can state from one read set -- the delete-a-group jackknife over reads (covest_amd/jackknife.py) and
the model's own Wald error (covest_amd/information.py).  Nothing in the output is a pass mark.

  basic    one random genome of 1 Mbp, 100-base reads at coverage 10, error rate 0.01, k = 21 forward strand, basic model
  repeats  repeat_genome and the repeats model at the settings of tests/repeat_recovery.py
For each: S read sets with simulator seeds 1 .. S, each estimated; the empirical standard deviation of coverage, error
rate and genome size over them; on the first four sets the jackknife standard errors at G groups and the Wald standard
errors; the ratios jackknife / empirical and Wald / empirical (medians over the four sets).  For the basic case also
the jackknife errors of sets 1 and 2 at G = 4 .. 256 on both refit routes.

And the rates, median of N by HIP events after a spin-up: the split alone at G = 2, 32, 256 on 10^9 bases of 100-base
reads beside covest_sample_reads_device at factor 1 (which moves the same bytes) and a device memcpy; and one whole
leave_group_out_histograms (upload, split, G + 1 counts) on 10^8 bases.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/jackknife_recovery.py [--sets 32] [--groups 32] [--out profiles/jackknife_recovery.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from covest_amd import _capi, constants, jackknife, sample, simulate as sim  # noqa: E402
from covest_amd.estimator import CoverageEstimator  # noqa: E402
from covest_amd.hist_steps import MAX_NOTRIM, compute_coverage_apx, get_trim, trim_hist  # noqa: E402
from covest_amd.information import genome_size_se, observed_information  # noqa: E402
from covest_amd.kmer_hist import KmerCounts  # noqa: E402
from covest_amd.models import select_model  # noqa: E402
from repeat_recovery import LOOP  # noqa: E402

BASIC = dict(genome_len=1_000_000, read_len=100, coverage=10, error_rate=0.01, k=21)
QUANTITIES = ("coverage", "error_rate", "genome_size")
READ_LEN, SEED = 100, 20241019


def fit(reads, k, model_name):
    """(model, estimate, success, hist_orig, trim) of one read set: forward-strand k-mers, sample factor 1, the cut of
    process_histogram (none up to abundance MAX_NOTRIM)."""
    counts = reads.add_to(KmerCounts(k, canonical=False))
    hist_orig = {i: v for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    trim = get_trim(hist_orig, ignore_last=True) if max(hist_orig) > MAX_NOTRIM else None
    hist, tail = trim_hist(hist_orig, trim) if trim is not None else (hist_orig, 0)
    model = select_model(model_name)(k, reads.read_length, hist, tail, max_error=constants.MAX_ERRORS, max_cov=None,
                                     min_single_copy_ratio=constants.DEFAULT_MIN_SINGLECOPY_RATIO)
    guess = list(model.defaults)
    c, e = compute_coverage_apx(hist_orig, k, reads.read_length)
    if not (c == 0 and e == 1):
        guess[:2] = c, e
    est, ok = CoverageEstimator(model).compute_coverage(guess)
    return model, [float(v) for v in est], bool(ok), hist_orig, trim


def recovery(name, genome, settings, model_name, sets, groups, lines):
    k, L = settings["k"], settings["read_len"]
    rows, jack, wald = [], [], []
    for seed in range(1, sets + 1):
        reads = sim.simulate_reads(genome, L, coverage=settings["coverage"], error_rate=settings["error_rate"], seed=seed,
                                   both_strands=False)
        model, est, ok, hist_orig, trim = fit(reads, k, model_name)
        occurrences = sum(i * n for i, n in hist_orig.items())
        rows.append((est[0], est[1], occurrences / model.correct_c(est[0]), ok))
        if seed <= 4:
            out = jackknife.read_jackknife(model, est, reads, groups=groups, seed=seed, trim=trim)
            info = observed_information(model, est)
            size = genome_size_se(model, hist_orig, info)
            jack.append([out["standard_errors"][q] for q in QUANTITIES])
            wald.append([info["standard_errors"]["coverage"], info["standard_errors"]["error_rate"], size["genome_size_se"]])
            lines.append("  %-8s set %d: jackknife used %d of %d, keys added %d, full - given %s" % (
                name, seed, out["used"], groups, out["keys_added"], " ".join("%.2e" % d for d in out["full_minus_given"])))
        model.close()
    good = np.array([r[:3] for r in rows if r[3]], dtype=np.float64)
    sd = good.std(axis=0, ddof=1)
    lines.append("# %s: %d read sets (%d estimated with success), empirical mean and standard deviation" % (name, sets, len(good)))
    lines.append("# %-8s %-12s %14s %12s %12s %12s %10s %10s" % ("case", "quantity", "mean", "empirical sd", "jackknife se",
                                                              "Wald se", "jack/emp", "Wald/emp"))
    for d, q in enumerate(QUANTITIES):
        js = [row[d] for row in jack if row[d] is not None]
        ws = [row[d] for row in wald if row[d] is not None]
        j = statistics.median(js) if js else float("nan")
        w = statistics.median(ws) if ws else float("nan")
        lines.append("  %-8s %-12s %14.8g %12.4g %12.4g %12.4g %10.3f %10.3f" % (name, q, good[:, d].mean(), sd[d], j, w,
                                                                                 j / sd[d], w / sd[d]))
        for s, (jr, wr) in enumerate(zip(jack, wald)):
            lines.append("#   set %d %-12s jackknife %s Wald %s" % (s + 1, q, "%.4g" % jr[d] if jr[d] is not None else "none",
                                                                    "%.4g" % wr[d] if wr[d] is not None else "none"))


def sweep(lines):
    """The basic case's jackknife errors on sets 1 and 2 at G = 4 .. 256 and on both refit routes: whether the error
    depends on the number of groups or on where the refits stop."""
    lines.append("# sweep: the basic case, jackknife standard errors by number of groups and refit route")
    genome = sim.random_genome(BASIC["genome_len"], 1)
    for seed in (1, 2):
        reads = sim.simulate_reads(genome, BASIC["read_len"], coverage=BASIC["coverage"], error_rate=BASIC["error_rate"],
                                   seed=seed, both_strands=False)
        model, est, ok, hist_orig, trim = fit(reads, BASIC["k"], "basic")
        for groups in (4, 8, 32, 128, 256):
            for refit in jackknife.REFITS:
                out = jackknife.read_jackknife(model, est, reads, groups=groups, seed=seed, trim=trim, refit=refit)
                lines.append("  sweep    set %d G %3d %-18s coverage %.5f error_rate %.3e genome_size %.1f used %d" % (
                    seed, groups, refit, out["standard_errors"]["coverage"], out["standard_errors"]["error_rate"],
                    out["standard_errors"]["genome_size"], out["used"]))
        model.close()


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rates(reps, lines):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    hip = ctypes.CDLL(_capi.hip_runtimes_mapped()[0])  # the runtime torch brought: already mapped
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    n_bases = 10 ** 9
    n_reads = n_bases // READ_LEN
    reads = torch.randint(65, 85, (n_reads, READ_LEN), dtype=torch.uint8, device=dev)
    out = torch.empty(n_bases, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    first = torch.zeros(257, dtype=torch.int64, device=dev)

    def split(groups):
        return lambda: sample.split_reads_device(reads.data_ptr(), n_reads, out.data_ptr(), first.data_ptr(), groups, seed=SEED,
                                                 read_len=READ_LEN, stream=stream)

    def sampler():
        sample.sample_reads_device(reads.data_ptr(), n_reads, out.data_ptr(), counts.data_ptr(), 1, seed=SEED,
                                   read_len=READ_LEN, stream=stream)

    def memcpy():
        if hip.hipMemcpyAsync(out.data_ptr(), reads.data_ptr(), n_bases, 3, stream) != 0:
            raise SystemExit("hipMemcpyAsync failed")

    routes = [("split G=2", split(2)), ("split G=32", split(32)), ("split G=256", split(256)), ("sampler factor 1", sampler),
              ("memcpy", memcpy)]
    for _, fn in routes:  # spin-up: code objects loaded, scratch in place, clocks up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in routes}
    for _ in range(reps):
        for name, fn in routes:
            ms[name].append(timed_ms(fn))
    rate = {name: n_bases / (statistics.median(t) * 1e-3) / 1e9 for name, t in ms.items()}
    lines.append("# rates: GB/s of bases moved, median of %d; %d bases of %d-base reads; %s" % (reps, n_bases, READ_LEN,
                                                                                              torch.cuda.get_device_name(0)))
    lines.append("# %-18s %10s %10s %16s %10s %10s" % ("route", "ms", "GB/s", "of the sampler's", "least ms", "most ms"))
    for name, _ in routes:
        lines.append("  %-18s %10.3f %10.1f %16.3f %10.3f %10.3f" % (name, statistics.median(ms[name]), rate[name],
                                                                     rate[name] / rate["sampler factor 1"], min(ms[name]),
                                                                     max(ms[name])))
    del reads, out
    torch.cuda.empty_cache()
    # one whole leave_group_out_histograms: host reads in, histograms out
    n = 10 ** 6
    host = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, READ_LEN))
    for groups in (32,):
        jackknife.leave_group_out_histograms(host, 21, groups, seed=SEED)
        t = [timed_ms(lambda: jackknife.leave_group_out_histograms(host, 21, groups, seed=SEED)) for _ in range(reps)]
        lines.append("  leave_group_out_histograms, %d bases, k = 21, G = %d (upload, split, %d counts): %.1f ms, median of %d" % (
            n * READ_LEN, groups, groups + 1, statistics.median(t), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip", default="", help="comma-separated: basic, repeats, sweep, rates")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jackknife_recovery.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jackknife_recovery.py needs a HIP device")
    torch.cuda.set_device(0)
    skip = set(args.skip.split(","))

    def write():  # after every part: a run that is cut short leaves what it had
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    lines = ["# the estimate's spread over independent read sets of ONE genome, the delete-a-group jackknife over reads at "
             "G = %d and the model's Wald error; ratios are medians over the first four sets" % args.groups]
    if "basic" not in skip:
        lines.append("# basic: random genome %(genome_len)d, L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, k = %(k)d "
                     "forward strand, basic model" % BASIC)
        recovery("basic", sim.random_genome(BASIC["genome_len"], 1), BASIC, "basic", args.sets, args.groups, lines)
        write()
    if "repeats" not in skip:
        lines.append("# repeats: repeat genome %(genome_len)d, unit_len %(unit_len)d, (q1, q2, q) = (%(q1)g, %(q2)g, %(q)g), "
                     "L = %(read_len)d, c = %(coverage)g, e = %(error_rate)g, k = %(k)d forward strand, repeats model" % LOOP)
        g = sim.repeat_genome(LOOP["genome_len"], LOOP["unit_len"], LOOP["q1"], LOOP["q2"], LOOP["q"], 1,
                              divergence=LOOP["divergence"])
        recovery("repeats", g.bases, LOOP, "repeats", args.sets, args.groups, lines)
        write()
    if "sweep" not in skip:
        sweep(lines)
        write()
    if "rates" not in skip:
        rates(args.reps, lines)
    write()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
