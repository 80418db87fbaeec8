"""The per-read k-mer lookup restated in plain Python over tests/kmer_reference.py (TEST INFRASTRUCTURE ONLY; not
collected).  Written from the definition in include/covest_amd.h and csrc/kmer_lookup.h, not from the kernel:

  * the table is kmer_reference.count's {key: occurrences}; a window's key is kmer_reference._key of its digits;
  * abundance: per base of a read, min(count, 0xFFFFFFFE) where a window starts, 0xFFFFFFFF at the last k - 1 bases
    (all of a read shorter than k: such a read has no window, the key the counter counts for it is not looked up);
  * summary: (min abundance, windows below the cutoff, the first and the last of them), 0xFFFFFFFF for "none";
  * score: lane l of 64 adds weights[min(count, n_weights - 1)] of windows l, l + 64, ... in ascending order onto
    +0.0; the 64 partials are folded by the xor butterfly off = 32, 16, ..., 1, p <- p + p[l xor off]; lane 0's value.
"""
import functools

import numpy as np

import kmer_reference as kr

NONE = 0xFFFFFFFF
LANES = 64


def window_counts(read, counts, k, canonical):
    """The table's (unclipped) count per window of one read: [] for a read shorter than k."""
    d = kr._digits(read)
    return [counts.get(kr._key(d[s:s + k], k, canonical), 0) for s in range(len(d) - k + 1)]


def butterfly_sum(values):
    """The score's sum in the kernel's order, in IEEE doubles (Python floats)."""
    p = [0.0] * LANES
    for s, v in enumerate(values):
        p[s % LANES] = p[s % LANES] + float(v)
    off = LANES // 2
    while off >= 1:
        p = [p[lane] + p[lane ^ off] for lane in range(LANES)]
        off //= 2
    return p[0]


def summary_of(found, cutoff):
    """(min_abundance, weak, first_weak, last_weak) of one read's (clipped) abundances."""
    if not found:
        return (NONE, 0, NONE, NONE)
    weak = [s for s, a in enumerate(found) if a < cutoff]
    return (min(found), len(weak), weak[0] if weak else NONE, weak[-1] if weak else NONE)


def lookup(reads, counts, k, canonical, cutoff=0, weights=None):
    """(abundance uint32 flat, offsets int64, summary uint32 (n, 4), score float64 (n,) or None) of `reads` (strings)
    against `counts` (kmer_reference.count of whatever was counted)."""
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    abundance = np.full(int(offsets[-1]), NONE, dtype=np.uint32)
    summary = np.empty((len(reads), 4), dtype=np.uint32)
    score = None if weights is None else np.zeros(len(reads), dtype=np.float64)
    for i, read in enumerate(reads):
        raw = window_counts(read, counts, k, canonical)
        found = [min(c, NONE - 1) for c in raw]
        abundance[offsets[i]:offsets[i] + len(found)] = found
        summary[i] = summary_of(found, cutoff)
        if weights is not None:
            score[i] = butterfly_sum(weights[min(c, len(weights) - 1)] for c in raw)
    return abundance, offsets, summary, score


def signed(column):
    """A summary column as the package reports it: int64 with -1 for 0xFFFFFFFF."""
    out = np.asarray(column).astype(np.int64)
    out[out == NONE] = -1
    return out


def locate_single_errors(k, lengths, weak, first_weak, last_weak):
    """The rule of ReadErrorScores.locate_single_errors, read by read (signed summary columns)."""
    out = []
    for n, w, f, l in zip(lengths, weak, first_weak, last_weak):
        last_window = n - k
        if w < 1 or w != l - f + 1 or w > k:
            out.append(-1)
        elif f > 0:
            out.append(f + k - 1)
        elif l < last_window:
            out.append(l)
        else:
            out.append(-1)
    return np.asarray(out, dtype=np.int64)


# ---- the simulated case of DESIGN.md section 6ae: the same numbers on the CPU and on the device ---------------------
CASE = dict(genome_len=6000, seed=20261020, n_reads=2812, read_len=64, error_rate=0.01, k=17, cutoff=3)
# what the restatement gives (tests/test_lookup_cpu.py recomputes and pins them)
CASE_EXPECTED = dict(with_error=1396, flagged=1398, missed=1, false=3, single=1018, located_right=1015,
                     located_wrong=2, located_undecided=1)


@functools.lru_cache(maxsize=None)
def simulated_case():
    """(genome uint8, bases (n, L) uint8, hit (n, L) bool, reads as strings, counts) of CASE, under sim_reference and
    kmer_reference alone.  Computed once; read-only."""
    import sim_reference as sr
    c = CASE
    genome = sr.random_genome(c["genome_len"], c["seed"])
    bases, _, hit, _ = sr.simulate(genome, c["read_len"], 0, c["n_reads"], c["error_rate"], c["seed"], True)
    reads = tuple(row.tobytes().decode() for row in bases)
    counts = kr.count(reads, c["k"], True)
    for a in (genome, bases, hit):
        a.setflags(write=False)
    return genome, bases, hit, reads, counts


@functools.lru_cache(maxsize=None)
def simulated_case_summary(cutoff=CASE["cutoff"]):
    """The restatement's summary (n, 4) uint32 of the simulated case at `cutoff` (read-only)."""
    _, _, _, reads, counts = simulated_case()
    _, _, summary, _ = lookup(reads, counts, CASE["k"], True, cutoff)
    summary.setflags(write=False)
    return summary


def detection_figures(flagged, hit):
    """(reads with a substitution, flagged, missed, falsely flagged, sensitivity, specificity)."""
    wrong = hit.any(axis=1)
    missed = int((wrong & ~flagged).sum())
    false = int((~wrong & flagged).sum())
    n_wrong, n_clean = int(wrong.sum()), int((~wrong).sum())
    return n_wrong, int(flagged.sum()), missed, false, 1.0 - missed / n_wrong, 1.0 - false / n_clean


def location_figures(located, hit):
    """Over the reads with exactly one substitution: (how many, located right, wrong, undecided)."""
    single = hit.sum(axis=1) == 1
    truth = hit.argmax(axis=1)
    right = int((single & (located == truth)).sum())
    undecided = int((single & (located < 0)).sum())
    return int(single.sum()), right, int(single.sum()) - right - undecided, undecided
