"""The duplicate remover on the device (dedup_reads.hip through covest_amd.dedup and the C ABI)
against its restatement (tests/dedup_reference.py): kept reads, copies, the collided count, bases and offsets equal
bit for bit, with guard words around every output -- whatever the number of reads, their lengths, the alignment of their
starts, the byte that tells two reads apart, the reverse complement, or the number of fingerprint bits.  There is no
reference implementation of this step: the expected values are the rule restated, and at 63 bits a dictionary of byte
strings.  No tolerance anywhere.

The host form runs in this process (numpy buffers between guard words, the C ABI called directly).  The device form runs
over the same cases in ONE fresh child process with torch imported first (one HIP runtime a process):
this file run as a program.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dedup_reference as dr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = (0x0ded << 32) | 0x0badcafe   # both halves of the seed in use
PAT, WPAT, CPAT = 0xA5, -0x0123456789abcdef, 0x5A5A5A5A
OTHER = np.frombuffer(b"acgtnACGTN*", dtype=np.uint8)


def near_misses():
    """Reads that look alike and are not equal, and reads that are equal only through the reverse complement."""
    x = dr.random_reads(1, 129, 31)[0]

    def flip(read, at):
        return read[:at] + (b"a" if read[at:at + 1] != b"a" else b"c") + read[at + 1:]
    s, t = dr.random_reads(2, 20, 32)
    rc = lambda r: bytes(dr.revcomp(r))  # noqa: E731
    mixed = dr.random_reads(3, 77, 33, OTHER)
    reads = [x, x[:50], x[:128], flip(x, 0), flip(x, 128), flip(x, 63), flip(x, 64),      # a prefix; one byte differs
             x.upper(), b"A" + x[1:], b"a" + x[1:],                                       # case is not folded
             rc(x), rc(x.upper()),                                                        # equal only with the reverse complement
             s + rc(s), s + rc(s), t + rc(t),                                             # palindromes of even length
             s + b"a" + rc(s), s + b"t" + rc(s), s + b"n" + rc(s), s + b"n" + rc(s),      # odd: a middle base is not its own complement; n is
             mixed[0], rc(mixed[0]), mixed[1], mixed[1], rc(mixed[2]), mixed[2],          # n, *, mixed case
             b"", b"", b"a", b"t", b"a", b"n", x]
    return reads


def alignments():
    """Reads of 1 031, 257 and 301 bases back to back (1 589 = 5 mod 16: the starts of each length run through every
    byte alignment mod 16), equal reads at different alignments among them."""
    a, b, c = dr.random_reads(1, 1031, 41)[0], dr.random_reads(1, 257, 42)[0], dr.random_reads(1, 301, 43)[0]
    fa, fb, fc = iter(dr.random_reads(40, 1031, 44)), iter(dr.random_reads(40, 257, 45)), iter(dr.random_reads(40, 301, 46))
    reads = []
    for i in range(40):
        reads += [a if i % 2 else next(fa), b if i % 3 == 0 else next(fb), c if i % 5 < 2 else next(fc)]
    starts = np.cumsum([0] + [len(r) for r in reads[:-1]])
    for length in (1031, 257, 301):
        assert {int(s) % 16 for s, r in zip(starts, reads) if len(r) == length} == set(range(16))
    return reads


@functools.lru_cache(maxsize=None)
def read_sets():
    """{name: (reads, fixed length or None)}: computed once, shared, never changed."""
    sets = {
        "one": (dr.random_reads(1, 100, 1), 100),
        "1000 copies": (dr.random_reads(1, 100, 2) * 1000, 100),
        "no two equal": (dr.random_reads(500, 100, 3), 100),
        "30 % copies": (dr.with_copies(3000, 100, 0.3, 4), 100),
        "30 % copies, half reversed": (dr.with_copies(3000, 100, 0.3, 5, rc_copies=True), 100),
        "ragged": (dr.ragged(6), None),
        "ragged, other bytes": (dr.ragged(7, alphabet=OTHER), None),
        "near misses": (near_misses(), None),
        "alignments": (alignments(), None),
        "empty reads": ([b""] * 300, 0),
    }
    for length in dr.LENGTHS[1:]:
        sets["length %d" % length] = (dr.with_copies(40, length, 0.3, 8 + length, rc_copies=True), length)
    return sets


def cases():
    """(name of the read set, reverse_complement, fp_bits, seed, first_read)."""
    for name in read_sets():
        for rc in (False, True):
            yield name, rc, 63, SEED, (1 << 32) + 5 if name == "30 % copies" else 0
    for bits in (1, 4, 8):
        for rc in (False, True):
            yield "30 % copies, half reversed" if rc else "30 % copies", rc, bits, SEED + bits, 0
    yield "ragged", True, 4, 9, 7
    yield "near misses", True, 2, 9, 0


@functools.lru_cache(maxsize=None)
def expected(name, rc, bits, seed):
    """(kept, copies, collided, bases, offsets) of the restatement; at 63 bits first held against the dictionary."""
    reads = read_sets()[name][0]
    kept, copies, collided = dr.dedup(reads, bits, seed, rc)
    if bits == 63:
        assert collided == 0, name
        want_kept, want_copies = dr.dictionary(reads, rc)
        assert np.array_equal(kept, want_kept) and np.array_equal(copies, want_copies), name
    else:
        assert collided > 0, (name, bits)
    assert int(copies.sum()) == len(reads)
    bases, offsets = dr.pack([reads[i] for i in kept])
    for a in (kept, copies, bases, offsets):
        a.setflags(write=False)
    return kept, copies, collided, bases, offsets


def guarded(n, dtype, pat):
    """An array of n elements between two guard elements either side, all of it the pattern: (whole, the inner part)."""
    whole = np.full(n + 4, pat, dtype=dtype)
    return whole, whole[2:2 + n]


def check_outputs(where, want, first_read, n, total, counts, bases, offsets, kept, copies):
    """Every output (whole, inner) against the restatement, and nothing written beyond its stated range."""
    want_kept, want_copies, want_collided, want_bases, want_offsets = want
    nk, nb = want_kept.size, want_bases.size
    assert counts[1].tolist() == [nk, nb, want_collided], ("counts", where, counts[1])
    assert np.array_equal(kept[1][:nk], want_kept + first_read), ("kept", where)
    assert np.array_equal(copies[1][:nk], want_copies), ("copies", where)
    assert np.array_equal(offsets[1][:nk + 1], want_offsets), ("offsets", where)
    assert np.array_equal(bases[1][:nb], want_bases), ("bases", where)
    for (whole, inner), used, pat in ((counts, 3, WPAT), (kept, nk, WPAT), (copies, nk, CPAT), (offsets, nk + 1, WPAT),
                                      (bases, nb, PAT)):
        rest = np.concatenate([whole[:2], inner[used:], whole[2 + inner.size:]])
        assert (rest == np.array(pat).astype(whole.dtype)).all(), ("stray write", where)


def run_host(name, rc, bits, seed, first_read, lib):
    reads, fixed = read_sets()[name]
    blob, offs = dr.pack(reads)
    n, total = len(reads), blob.size
    counts, bases, offsets = guarded(3, np.int64, WPAT), guarded(total, np.uint8, PAT), guarded(n + 1, np.int64, WPAT)
    kept, copies = guarded(n, np.int64, WPAT), guarded(n, np.int32, CPAT)
    for with_offsets in ((True, False) if fixed is not None else (True,)):
        for whole, _ in (counts, bases, offsets, kept, copies):
            whole[:] = whole[0]
        c = counts[1]
        rcode = lib.covest_dedup_reads(-1, blob.ctypes.data, offs.ctypes.data if with_offsets else None, n,
                                       0 if with_offsets else fixed, first_read, int(rc), bits, seed, bases[1].ctypes.data,
                                       offsets[1].ctypes.data, kept[1].ctypes.data, copies[1].ctypes.data,
                                       ctypes.cast(c.ctypes.data, ctypes.POINTER(ctypes.c_int64)),
                                       ctypes.cast(c.ctypes.data + 8, ctypes.POINTER(ctypes.c_int64)),
                                       ctypes.cast(c.ctypes.data + 16, ctypes.POINTER(ctypes.c_int64)))
        assert rcode == 0, (name, lib.covest_last_error())
        check_outputs((name, rc, bits, with_offsets), expected(name, rc, bits, seed), first_read, n, total, counts, bases,
                      offsets, kept, copies)


@pytest.mark.parametrize("name,rc,bits,seed,first_read", list(cases()), ids=lambda v: str(v).replace(" ", "_"))
def test_host_form(hip_lib, name, rc, bits, seed, first_read):
    run_host(name, rc, bits, seed, first_read, hip_lib)


def test_no_reads(hip_lib):
    from covest_amd.dedup import dedup_reads
    counts, offsets = guarded(3, np.int64, WPAT), guarded(1, np.int64, WPAT)
    c = counts[1]
    ptr = lambda at: ctypes.cast(c.ctypes.data + at, ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    assert hip_lib.covest_dedup_reads(-1, None, None, 0, 5, 0, 1, 63, 0, None, offsets[1].ctypes.data, None, None,
                                      ptr(0), ptr(8), ptr(16)) == 0
    assert counts[0].tolist() == [WPAT, WPAT, 0, 0, 0, WPAT, WPAT] and offsets[0].tolist() == [WPAT, WPAT, 0, WPAT, WPAT]
    got = dedup_reads(np.zeros((0, 100), dtype=np.uint8))
    assert got.n_reads == 0 and got.n_input == 0 and got.duplicate_share == 0.0 and got.copies_histogram() == {}
    assert got.bases.shape == (0, 100) and got.offsets.tolist() == [0] and got.collided == 0
    got = dedup_reads((np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)), reverse_complement=True)
    assert got.n_reads == 0 and got.offsets.tolist() == [0]


@pytest.mark.parametrize("rc", (False, True))
def test_dedup_reads_returns_the_first_read_of_every_class(hip_lib, rc):
    from covest_amd.dedup import dedup_reads
    for name in ("30 % copies, half reversed", "ragged, other bytes", "near misses", "1000 copies"):
        reads, fixed = read_sets()[name]
        want_kept, want_copies = dr.dictionary(reads, rc)
        first = (1 << 33) + 1
        got = dedup_reads(np.frombuffer(b"".join(reads), dtype=np.uint8).reshape(len(reads), fixed) if fixed
                          else dr.pack(reads), reverse_complement=rc, seed=SEED, first_read=first)
        assert got.collided == 0 and got.rounds == 1
        assert np.array_equal(got.kept, want_kept + first) and np.array_equal(got.copies, want_copies), name
        assert got.copies.dtype == np.int32 and int(got.copies.sum()) == len(reads) == got.n_input
        bases, offsets = dr.pack([reads[i] for i in want_kept])
        assert np.array_equal(np.ascontiguousarray(got.bases).reshape(-1), bases) and np.array_equal(got.offsets, offsets)
        assert got.n_reads == want_kept.size and got.duplicate_share == (len(reads) - want_kept.size) / len(reads)
        values, counts = np.unique(want_copies, return_counts=True)
        assert got.copies_histogram() == dict(zip(values.tolist(), counts.tolist()))


@functools.lru_cache(maxsize=None)
def rounds_case():
    """(fp_bits, seed) at which, by the restatement, round 1 on the 3 000 reads keeps a DUPLICATE beside a collision and
    round 2 (seed + 1, on round 1's output) has no collision left."""
    reads = read_sets()["30 % copies"][0]
    want = dr.dictionary(reads)[0]
    for bits in (20, 21, 22):
        for seed in range(40):
            kept, _, collided = dr.dedup(reads, bits, seed)
            if collided and kept.size > want.size:
                if dr.dedup([reads[i] for i in kept], bits, seed + 1)[2] == 0:
                    return bits, seed
    raise AssertionError("no such case")


def test_rounds_remove_what_survived_beside_a_collision(hip_lib):
    from covest_amd import _capi
    from covest_amd.dedup import _dedup_rounds
    reads = read_sets()["30 % copies"][0]
    blob = np.frombuffer(b"".join(reads), dtype=np.uint8)
    want_kept, want_copies = dr.dictionary(reads)
    bits, seed = rounds_case()
    out, offsets, rows, copies, collided, rounds = _dedup_rounds(blob, None, len(reads), 100, False, bits, seed, -1)
    assert collided == dr.dedup(reads, bits, seed)[2] > 0 and rounds == 2
    assert np.array_equal(rows, want_kept) and np.array_equal(copies, want_copies)
    assert np.array_equal(out, dr.pack([reads[i] for i in want_kept])[0])
    assert np.array_equal(offsets, np.arange(want_kept.size + 1) * 100)
    with pytest.raises(_capi.CovestHipError, match="still collide after 4 rounds"):   # two keys for 2 100 reads
        _dedup_rounds(blob, None, len(reads), 100, False, 1, seed, -1)


def test_simulated_reads_in_and_add_to(hip_lib):
    import kmer_reference as kr
    from covest_amd import simulate as sim
    from covest_amd.dedup import dedup_reads
    from covest_amd.kmer_hist import KmerCounts
    g = sim.random_genome(5_000, 3)
    reads = sim.simulate_reads(g, 100, n_reads=3000, error_rate=0.0, seed=3, first_read=77)
    strings = [bytes(r) for r in reads.bases]
    for rc in (False, True):
        want_kept, want_copies = dr.dictionary(strings, rc)
        assert 0 < want_kept.size < 3000
        got = dedup_reads(reads, reverse_complement=rc)           # numbered from the reads' own first_read
        assert np.array_equal(got.kept, want_kept + 77) and np.array_equal(got.copies, want_copies)
        assert np.array_equal(got.bases, reads.bases[want_kept])
        assert np.array_equal(got.positions, reads.positions[want_kept])
        assert np.array_equal(got.forward, reads.forward[want_kept])
        if not rc:  # equal bytes without an error: the same place and strand, or a repeat of the genome
            assert (got.copies > 1).any()
        counts = got.add_to(KmerCounts(21, canonical=True))
        want_hist, want_distinct = kr.histogram([strings[i].decode() for i in want_kept], 21, True)
        assert counts.histogram() == want_hist and len(counts) == want_distinct
        counts.close()


def test_fasta_tool(hip_lib, tmp_path):
    from covest_amd import dedup
    reads = [r for r in read_sets()["ragged"][0] if r]
    src, dest = tmp_path / "reads.fa", tmp_path / "unique.fa"
    src.write_text("".join(">r%d\n%s\n" % (i, r.decode()) for i, r in enumerate(reads)))
    got = dedup.dedup_reads_file(str(src), str(dest), reverse_complement=True)
    want_kept, want_copies = dr.dictionary(reads, True)
    assert np.array_equal(got.kept, want_kept) and np.array_equal(got.copies, want_copies)
    lines = dest.read_text().split("\n")
    assert lines[0:-1:2] == [">read_%d" % i for i in want_kept] and lines[1::2] == [reads[i].decode() for i in want_kept]


def test_error_codes(hip_lib):
    from covest_amd import _capi
    L = hip_lib
    blob, offs = dr.pack([b"acgt", b"acgt"])
    out, out_offs, kept, copies = np.zeros(8, np.uint8), np.zeros(3, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int32)
    c = [ctypes.c_int64() for _ in range(3)]
    tail = [ctypes.byref(v) for v in c]

    def host(**kw):
        a = dict(offsets=offs.ctypes.data, n=2, read_len=0, first=0, bits=63, out_offsets=out_offs.ctypes.data, tail=tail)
        a.update(kw)
        return L.covest_dedup_reads(-1, blob.ctypes.data, a["offsets"], a["n"], a["read_len"], a["first"], 0, a["bits"], 0,
                                    out.ctypes.data, a["out_offsets"], kept.ctypes.data, copies.ctypes.data, *a["tail"])

    def device(**kw):  # (every one of these is refused before a pointer is looked at)
        a = dict(offsets=4096, n=2, read_len=0, first=0, bits=63, out_offsets=8192, counts=12288)
        a.update(kw)
        return L.covest_dedup_reads_device(-1, 256, a["offsets"], a["n"], a["read_len"], a["first"], 0, a["bits"], 0, 512,
                                           a["out_offsets"], None, None, a["counts"], None)
    assert host() == 0 and [v.value for v in c] == [1, 4, 0]
    down = np.array([0, 4, 2], dtype=np.int64)
    for form, bad in ((host, dict(bits=0)), (host, dict(bits=64)), (host, dict(n=-1)), (host, dict(first=-1)),
                      (host, dict(offsets=None, read_len=-1)), (host, dict(out_offsets=None)),
                      (host, dict(tail=[None] + tail[1:])), (host, dict(tail=tail[:2] + [None])),
                      (host, dict(offsets=down.ctypes.data)), (host, dict(first=(1 << 63) - 1)),
                      (device, dict(bits=0)), (device, dict(bits=64)), (device, dict(bits=-1)), (device, dict(n=-1)),
                      (device, dict(first=-1)), (device, dict(offsets=None, read_len=-1)), (device, dict(out_offsets=None)),
                      (device, dict(counts=None))):
        assert form(**bad) == _capi.COVEST_E_INVALID, bad
        assert b"covest_dedup_reads" in L.covest_last_error(), bad
    assert b"fp_bits must be within 1 .. 63" in (host(bits=64), L.covest_last_error())[1]


def test_print_output_duplicates(hip_lib):
    from covest_amd import constants, print_output, simulate as sim
    from covest_amd.dedup import dedup_reads
    from covest_amd.kmer_hist import KmerCounts
    from covest_amd.models import BasicModel
    g = sim.random_genome(5_000, 5)
    reads = sim.simulate_reads(g, 100, n_reads=2000, error_rate=0.0, seed=5)
    unique = dedup_reads(reads)
    counts = unique.add_to(KmerCounts(21))
    hist = {i: int(v) for i, v in enumerate(counts.histogram()) if i > 0 and v > 0}
    counts.close()
    model = BasicModel(21, 100, hist, 0, max_error=constants.MAX_ERRORS)
    est = [30.0, 0.01]
    plain = print_output(hist, model, True, 1, estimated=est, silent=True)
    record = print_output(hist, model, True, 1, estimated=est, silent=True, duplicates=unique)
    new = {key for key in record if key.startswith("duplicates_")}
    assert new == {"duplicates_reads", "duplicates_kept", "duplicates_share", "duplicates_max_copies"}
    assert {key: value for key, value in record.items() if key not in new} == plain
    assert record["duplicates_reads"] == 2000 and record["duplicates_kept"] == unique.n_reads < 2000
    assert record["duplicates_share"] == (2000 - unique.n_reads) / 2000
    assert record["duplicates_max_copies"] == int(unique.copies.max()) >= 2


# ---- the device form: the same cases, in a child process ---------------------------------------------------------------
def run_device(name, rc, bits, seed, first_read, shifts, torch):
    from covest_amd.dedup import dedup_reads_device
    dev = torch.device("cuda", 0)
    reads, fixed = read_sets()[name]
    blob, offs = dr.pack(reads)
    n, total = len(reads), blob.size
    s_shift, d_shift = shifts
    want = expected(name, rc, bits, seed)
    for with_offsets in ((True, False) if fixed is not None else (True,)):
        src = torch.full((64 + s_shift + total + 64,), PAT, dtype=torch.uint8, device=dev)
        src[64 + s_shift:64 + s_shift + total] = torch.from_numpy(blob).to(dev)
        d_off = torch.from_numpy(offs).to(dev)
        outs = {"counts": (3, torch.int64, WPAT), "bases": (total, torch.uint8, PAT), "offsets": (n + 1, torch.int64, WPAT),
                "kept": (n, torch.int64, WPAT), "copies": (n, torch.int32, CPAT)}
        bufs = {key: torch.full((2 * 16 + (d_shift if key == "bases" else 0) + size,), pat, dtype=dtype, device=dev)
                for key, (size, dtype, pat) in outs.items()}
        at = {key: 16 + (d_shift if key == "bases" else 0) for key in outs}
        ptr = {key: bufs[key].data_ptr() + at[key] * bufs[key].element_size() for key in outs}
        dedup_reads_device(src.data_ptr() + 64 + s_shift, n, ptr["bases"], ptr["counts"], reverse_complement=rc, seed=seed,
                           first_read=first_read, read_len=0 if with_offsets else fixed,
                           offsets_ptr=d_off.data_ptr() if with_offsets else None, out_offsets_ptr=ptr["offsets"],
                           kept_ptr=ptr["kept"], copies_ptr=ptr["copies"], fp_bits=bits,
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = {}
        for key, (size, _, pat) in outs.items():
            whole = bufs[key].cpu().numpy()
            inner = whole[at[key]:at[key] + size]
            # (check_outputs looks at two guard elements either side; the rest of the margins here)
            assert (whole[:at[key] - 2] == np.array(pat).astype(whole.dtype)).all(), ("stray write", key, name)
            assert (whole[at[key] + size + 2:] == np.array(pat).astype(whole.dtype)).all(), ("stray write", key, name)
            got[key] = (whole[at[key] - 2:at[key] + size + 2], inner)
        check_outputs((name, rc, bits, with_offsets, shifts), want, first_read, n, total, got["counts"], got["bases"],
                      got["offsets"], got["kept"], got["copies"])
        s = src.cpu().numpy()
        assert (s[:64 + s_shift] == PAT).all() and (s[64 + s_shift + total:] == PAT).all(), ("source", name)


def device_cases():
    import torch
    SHIFTS = ((0, 1), (1, 7), (7, 0), (0, 7), (4, 0), (13, 3))   # source and destination off a 16-byte boundary
    for i, (name, rc, bits, seed, first_read) in enumerate(cases()):
        for shifts in (SHIFTS if name in ("alignments", "ragged") and bits == 63 else (SHIFTS[i % 6],)):
            run_device(name, rc, bits, seed, first_read, shifts, torch)
    # n_reads == 0: counts (0, 0, 0), out_offsets[0] = 0, nothing else
    from covest_amd.dedup import dedup_reads_device
    dev = torch.device("cuda", 0)
    d_counts = torch.full((5,), WPAT, dtype=torch.int64, device=dev)
    d_o = torch.full((3,), WPAT, dtype=torch.int64, device=dev)
    dedup_reads_device(0, 0, 0, d_counts.data_ptr() + 8, read_len=5, out_offsets_ptr=d_o.data_ptr() + 8,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [WPAT, 0, 0, 0, WPAT] and d_o.cpu().tolist() == [WPAT, 0, WPAT], "n_reads == 0"
    # without the optional outputs: nothing but bases and counts
    reads, fixed = read_sets()["30 % copies"]
    want = expected("30 % copies", False, 63, SEED)
    src = torch.from_numpy(dr.pack(reads)[0]).to(dev)
    dst = torch.full((src.numel() + 32,), PAT, dtype=torch.uint8, device=dev)
    d_counts.fill_(WPAT)
    dedup_reads_device(src.data_ptr(), len(reads), dst.data_ptr() + 16, d_counts.data_ptr() + 8, seed=SEED, read_len=fixed,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [WPAT, want[0].size, want[3].size, 0, WPAT]
    b = dst.cpu().numpy()
    assert np.array_equal(b[16:16 + want[3].size], want[3]) and (b[:16] == PAT).all() and (b[16 + want[3].size:] == PAT).all()


def test_device_form(hip_lib):
    """Raw device pointers (torch tensors): every case of the host form, with and without offsets, source and destination
    off a 16-byte boundary, guard words around every output; no reads; no optional output."""
    proc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "device"],
                          capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0 and "device form ok" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]


if __name__ == "__main__":
    import time
    import torch  # noqa: F401  first: ONE HIP runtime per process
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    t0 = time.perf_counter()
    device_cases()
    print("device form ok, %.2f s" % (time.perf_counter() - t0))
