"""The correction of isolated substitutions restated in plain Python over tests/kmer_reference.py and
tests/lookup_reference.py (TEST INFRASTRUCTURE ONLY; not collected).  Written from the rule in include/covest_amd.h and
DESIGN.md section 6af, not from the kernel:

  * a window is weak when the table's count for its key is below the cutoff (cutoff 0: none is);
  * a run is a maximal set of consecutive weak windows [f, l]; every run is judged against the ORIGINAL read;
  * its candidate positions are the bases whose covering windows are exactly [f, l]; an alternative (p, b) -- b one of
    the three other bases -- is valid when every window of the run, with base p replaced by b, has a count >= cutoff;
  * exactly one valid alternative: corrected (the new letter keeps the case of the old one); more: ambiguous; none:
    unfixable.  fix = (runs, corrected, ambiguous, unfixable) per read.
"""
import functools

import numpy as np

import kmer_reference as kr
import lookup_reference as lr

LETTERS = "ACGT"


def runs_of(weak):
    """[(f, l)] of the maximal runs of true entries of `weak`."""
    out, f = [], None
    for s, w in enumerate(list(weak) + [False]):
        if w and f is None:
            f = s
        elif not w and f is not None:
            out.append((f, s - 1))
            f = None
    return out


def candidate_positions(f, l, k, length):
    """The bases p of a read of `length` whose covering windows [max(0, p - k + 1), min(p, last)] are exactly [f, l]."""
    last = length - k
    if l - f + 1 > k:
        return []
    if f > 0:
        p = f + k - 1
        return [p] if l == min(p, last) else []
    if l < last:
        return [l]
    return list(range(last, min(k - 1, length - 1) + 1))


def judge_run(d, f, l, counts, k, canonical, cutoff):
    """The valid alternatives [(p, digit)] of the run [f, l] of the digit string `d`."""
    valid = []
    for p in candidate_positions(f, l, k, len(d)):
        for b in "0123":
            if b == d[p]:
                continue
            e = d[:p] + b + d[p + 1:]
            if all(counts.get(kr._key(e[s:s + k], k, canonical), 0) >= cutoff for s in range(f, l + 1)):
                valid.append((p, b))
    return valid


def correct_read(read, counts, k, canonical, cutoff):
    """(corrected read, (runs, corrected, ambiguous, unfixable)) of one read."""
    d = kr._digits(read)
    found = lr.window_counts(read, counts, k, canonical)
    out = list(read)
    row = [0, 0, 0, 0]
    for f, l in runs_of(c < cutoff for c in found):
        valid = judge_run(d, f, l, counts, k, canonical, cutoff)
        row[0] += 1
        if len(valid) == 1:
            p, b = valid[0]
            out[p] = chr(ord(LETTERS[int(b)]) | (ord(read[p]) & 0x20))
            row[1] += 1
        elif valid:
            row[2] += 1
        else:
            row[3] += 1
    return "".join(out), tuple(row)


def correct(reads, counts, k, canonical, cutoff):
    """(out uint8 flat, offsets int64, fix uint32 (n, 4), the corrected reads as strings) of `reads` (strings) against
    `counts` (kmer_reference.count of whatever was counted)."""
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    fix = np.zeros((len(reads), 4), dtype=np.uint32)
    strings = []
    for i, read in enumerate(reads):
        fixed, fix[i] = correct_read(read, counts, k, canonical, cutoff)
        strings.append(fixed)
    out = np.frombuffer("".join(strings).encode(), dtype=np.uint8).copy()
    return out, offsets, fix, strings


# ---- the simulated case of lookup_reference.CASE, corrected: the same numbers on the CPU and on the device --------------
# what the restatement gives at cutoff 3 (tests/test_correct_cpu.py recomputes and pins them)
CASE_EXPECTED = dict(runs=1624, corrected=1402, ambiguous=0, unfixable=222, miscorrected=0, reads_worse=0,
                     wrong_before=1851, wrong_after=449, reads_wrong_before=1396, reads_wrong_after=218,
                     distinct_before=26989, distinct_after=10260, singletons_before=20329, singletons_after=4235)


@functools.lru_cache(maxsize=None)
def simulated_case_corrected(cutoff=lr.CASE["cutoff"]):
    """(out (n, L) uint8, fix (n, 4) uint32, corrected reads as strings) of the simulated case at `cutoff` (read-only)."""
    _, bases, _, reads, counts = lr.simulated_case()
    out, _, fix, strings = correct(reads, counts, lr.CASE["k"], True, cutoff)
    out = out.reshape(bases.shape)
    out.setflags(write=False)
    fix.setflags(write=False)
    return out, fix, tuple(strings)


@functools.lru_cache(maxsize=None)
def simulated_case_truth():
    """The reads of the simulated case as the simulator makes them at error rate 0: (n, L) uint8 (read-only)."""
    import sim_reference as sr
    c = lr.CASE
    truth = sr.simulate(lr.simulated_case()[0], c["read_len"], 0, c["n_reads"], 0.0, c["seed"], True)[0]
    truth.setflags(write=False)
    return truth


def recovery_figures(bases, out, truth):
    """(wrong bases before, after, reads with a wrong base before, after, corrections to a base other than the true
    one, reads with more wrong bases after than before) of (n, L) arrays."""
    before, after = bases != truth, out != truth
    changed = out != bases
    return (int(before.sum()), int(after.sum()), int(before.any(axis=1).sum()), int(after.any(axis=1).sum()),
            int((changed & after).sum()), int((after.sum(axis=1) > before.sum(axis=1)).sum()))


def table_figures(counts):
    """(distinct keys, keys counted once) of a kmer_reference.count."""
    return len(counts), sum(1 for n in counts.values() if n == 1)
