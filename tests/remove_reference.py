"""Removal from a k-mer table restated from its definition.  TEST INFRASTRUCTURE ONLY.

A table is a dict {key: count} (keys as tests/kmer_reference.py makes them).
  * add: every window of read r raises its key's count by 1, or by weights[r]; a weight of 0 touches nothing and
    creates no key;
  * remove: every window of read r lowers its key's count by 1, or by weights[r]; a weight of 0 touches nothing; a key
    the dict does not carry, or a count smaller than what is subtracted, raises Underflow; the key STAYS in the dict
    when its count reaches 0;
  * held: the keys with a count above 0; occupied: the keys the dict carries.
It knows nothing of slots, probe chains or atomics.  tests/test_remove_cpu.py holds it against a loop over every
possible key at k = 2 and 3; tests/test_gpu_remove.py holds the device against it.
"""
from collections import Counter

import kmer_reference as kr


class Underflow(Exception):
    pass


def windows(read, k, canonical):
    """The keys of a read's windows in order; of a read shorter than k the one key add counts for it."""
    d = kr._digits(read)
    if len(d) < k:
        return [kr._key(d, k, canonical)]
    return [kr._key(d[s:s + k], k, canonical) for s in range(len(d) - k + 1)]


class Table:
    def __init__(self, k, canonical=False):
        self.k, self.canonical = int(k), bool(canonical)
        self.counts = {}

    def _per_key(self, reads, weights):
        per_key = Counter()
        for r, read in enumerate(reads):
            w = 1 if weights is None else int(weights[r])
            if w == 0:
                continue
            for key, n in kr.count([read], self.k, self.canonical).items():
                per_key[key] += n * w
        return per_key

    def add(self, reads, weights=None):
        for key, n in self._per_key(reads, weights).items():
            self.counts[key] = self.counts.get(key, 0) + n
        return self

    def remove(self, reads, weights=None):
        """The subtractions commute, so an underflow shows in the totals per key: some order of the windows meets a
        count smaller than what it subtracts exactly when the total exceeds the count."""
        per_key = self._per_key(reads, weights)
        for key, n in per_key.items():
            if key not in self.counts or self.counts[key] < n:
                raise Underflow(key)
        for key, n in per_key.items():
            self.counts[key] -= n
        return self

    def held(self):
        return {key: n for key, n in self.counts.items() if n > 0}

    def occupancy(self):
        """(keys held, keys the dict carries)."""
        return len(self.held()), len(self.counts)

    def compact(self):
        self.counts = self.held()
        return self

    def histogram(self):
        """(count-of-counts list indexed 0 .. max count -- [0] when nothing is held --, keys held)."""
        held = self.held()
        if not held:
            return [0], 0
        per_count = Counter(held.values())
        return [per_count.get(i, 0) for i in range(max(per_count) + 1)], len(held)

    def lookup(self, reads):
        """Per read the counts of its windows' keys in order (0: not held); a read shorter than k has no window."""
        return [[self.counts.get(key, 0) for key in windows(read, self.k, self.canonical)] if len(read) >= self.k else []
                for read in reads]
