"""The read simulator without a device: the stream's known answers, the numpy restatement's own statistics (the device
is required to be bit-identical to it, tests/test_gpu_simulate.py, so they hold for the device too), the argument
rules of covest_amd.simulate and of the C entry points, and that nothing is computed where there is no device."""
import ctypes
import math

import numpy as np
import pytest

import sim_reference as sr

# Philox4x32-10 known answers (counter, key, output)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert sr.philox_scalar(counter, key) == want
        got = sr.philox(*[np.array([c], dtype=np.uint64) for c in counter], *key)
        assert tuple(int(w[0]) for w in got) == want
    # the vectorised form over a batch equals the scalar one element by element
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, size=(4, 50), dtype=np.uint64)
    got = sr.philox(c[0], c[1], c[2], c[3], 0x12345678, 0x9abcdef0)
    for i in range(50):
        assert tuple(int(w[i]) for w in got) == sr.philox_scalar(tuple(int(x) for x in c[:, i]), (0x12345678, 0x9abcdef0))


def test_restatement_definition_by_hand():
    """The restatement against the definition spelled out with plain integers for a few reads."""
    seed, L, e = (7 << 32) | 99, 10, 0.3
    genome = sr.random_genome(500, seed).tobytes().decode()
    for i in (0, 1, 2, 3, 4, 7, 499):
        w = sr.philox_scalar(((i >> 2) & sr.MASK, (i >> 2) >> 32, 0, 1), (99, 7))[i & 3]
        assert genome[i] == "ACGT"[w >> 30]
    first = (1 << 32) - 2
    bases, origin = sr.reads_and_origin(genome, L, first, 4, e, seed)
    thr = int(math.floor(e * 2 ** 32))
    for n in range(4):
        r = first + n
        w0, w1, w2, _ = sr.philox_scalar((r & sr.MASK, r >> 32, 0, 0), (99, 7))
        pos = ((w0 | (w1 << 32)) * (500 - L)) >> 64
        fwd = w2 & 1
        assert origin[n] == (pos << 1 | fwd)
        s = genome[pos:pos + L]
        if not fwd:
            s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
        want = []
        for i, b in enumerate(s):
            w = sr.philox_scalar((r & sr.MASK, r >> 32, 1 + (i >> 2), 0), (99, 7))[i & 3]
            code = "ACGT".index(b)
            want.append("ACGT"[(code + 1 + w % 3) & 3] if w < thr else b)
        assert bases[n].tobytes().decode() == "".join(want)


def test_restatement_statistics():
    """10 000 reads of 100 bases from a 50 000-base genome at e = 0.01, fixed seed; every bound is six binomial standard
    deviations of the count it bounds."""
    n, L, g_len, e, seed = 10_000, 100, 50_000, 0.01, 20241018
    genome = sr.random_genome(g_len, seed)
    bases, origin, hit, offs = sr.simulate(genome, L, 0, n, e, seed)
    N = n * L
    subs = int(hit.sum())
    assert abs(subs - N * e) <= 6 * math.sqrt(N * e * (1 - e))          # +-597 around 10 000
    forward = int((origin & 1).sum())
    assert abs(forward - n / 2) <= 6 * math.sqrt(n / 4)
    for k in range(3):
        took = int((offs[hit] == k).sum())
        assert abs(took - subs / 3) <= 6 * math.sqrt(subs * (1 / 3) * (2 / 3)), (k, took, subs)
    pos = origin >> 1
    assert pos.min() >= 0 and pos.max() <= g_len - L - 1
    # a substituted base is never the base it replaces; every other base is the genome's
    twin, _ = sr.reads_and_origin(genome, L, 0, n, 0.0, seed)
    assert np.array_equal(bases != twin, hit)
    # the genome's composition: each base a quarter of 50 000, six standard deviations
    for b in b"ACGT":
        assert abs(int((genome == b).sum()) - g_len / 4) <= 6 * math.sqrt(g_len * 0.25 * 0.75)


def test_argument_validation():
    from covest_amd import simulate as sim
    g = "ACGT" * 30
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 0, n_reads=1)
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 2.5, n_reads=1)
    with pytest.raises(ValueError):
        sim.simulate_reads(g, len(g), n_reads=1)            # genome_len <= read_len
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 10, n_reads=-1)
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 10, n_reads=1, first_read=-1)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            sim.simulate_reads(g, 10, n_reads=1, error_rate=bad)
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 10)                            # neither coverage nor n_reads
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 10, coverage=-1.0)
    with pytest.raises(ValueError):
        sim.simulate_reads(g, 10, n_reads=1, seed=1 << 64)
    with pytest.raises(ValueError):
        sim.simulate_reads("ACGTN" * 30, 10, n_reads=1)     # IUPAC letters are not substituted
    with pytest.raises(ValueError):
        sim.simulate_reads(np.zeros(100, dtype=np.int32), 10, n_reads=1)
    with pytest.raises(ValueError):
        sim.random_genome(-1, 0)
    with pytest.raises(ValueError):
        sim.simulate_reads_device(0, 100, 100, 1, 0)
    assert sim._n_reads(10.0, 1000, 100, None) == 100 and sim._n_reads(0.26, 1000, 100, None) == 3
    assert sim._n_reads(None, 1000, 100, 7) == 7


def test_c_entry_points_refuse_bad_arguments(hip_lib):
    """COVEST_E_INVALID before any device is looked for; n_reads == 0 is COVEST_OK with nothing launched."""
    genome = np.frombuffer(b"ACGTacgt" * 20, dtype=np.uint8).copy()
    bases = np.zeros(1000, dtype=np.uint8)
    g, b = genome.ctypes.data, bases.ctypes.data

    def host(glen=160, L=10, first=0, n=5, e=0.1, gp=g, bp=b):
        return hip_lib.covest_simulate_reads(-1, gp, glen, L, first, n, e, 1, 1, bp, None)

    def device(glen=160, L=10, first=0, n=5, e=0.1):
        return hip_lib.covest_simulate_reads_device(-1, g, glen, L, first, n, e, 1, 1, b, None, None)

    for fn in (host, device):
        assert fn(glen=10) == -1 and fn(glen=9) == -1       # genome_len <= read_len
        assert fn(L=0) == -1 and fn(L=-3) == -1
        assert fn(n=-1) == -1 and fn(first=-1) == -1
        assert fn(e=-0.5) == -1 and fn(e=1.5) == -1 and fn(e=float("nan")) == -1
        assert fn(n=(1 << 62), L=100) == -1                  # n_reads * read_len beyond 64 bits
        assert fn(n=0) == 0
        assert fn(n=0, e=1.0) == 0 and fn(n=0, e=0.0) == 0
    assert host(gp=None) == -1 and host(bp=None) == -1
    bad = np.frombuffer(b"ACGTNACGT" * 20, dtype=np.uint8).copy()
    assert host(glen=bad.size, gp=bad.ctypes.data) == -1
    assert b"acgtACGT" in hip_lib.covest_last_error()
    assert host(glen=bad.size, gp=bad.ctypes.data, n=0) == -1  # the host form looks at the genome whatever n_reads is
    assert hip_lib.covest_random_genome(-1, -1, 0, b) == -1
    assert hip_lib.covest_random_genome(-1, 5, 0, None) == -1
    assert hip_lib.covest_random_genome(-1, 0, 0, None) == 0
    assert hip_lib.covest_random_genome_device(-1, -1, 0, b, None) == -1
    assert hip_lib.covest_random_genome_device(-1, 0, 0, None, None) == 0
    assert not bases.any()


def test_no_cpu_path(hip_lib):
    from covest_amd import _capi, simulate as sim
    if hip_lib.covest_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_capi.CovestHipError):
        sim.simulate_reads("ACGT" * 100, 20, n_reads=5, error_rate=0.1)
    with pytest.raises(_capi.CovestHipError):
        sim.random_genome(100, 1)


def test_simulated_reads_record(tmp_path):
    """SimulatedReads over the restatement's arrays: positions, strands, twin, substitutions, FASTA (host arithmetic)."""
    from covest_amd.simulate import SimulatedReads
    seed, L, n, e = 3, 25, 40, 0.2
    genome = sr.random_genome(2000, seed)
    bases, origin, hit, _ = sr.simulate(genome, L, 5, n, e, seed)
    reads = SimulatedReads(bases, origin, genome.size, e, seed, 5)
    assert reads.n_reads == n and reads.read_length == L and reads.true_coverage == n * L / 2000
    assert np.array_equal(reads.positions, origin >> 1) and np.array_equal(reads.forward, (origin & 1) == 1)
    twin, _ = sr.reads_and_origin(genome, L, 5, n, 0.0, seed)
    assert np.array_equal(reads.error_free(genome), twin)
    assert np.array_equal(reads.error_free(genome.tobytes().decode().lower()), twin)
    assert reads.substitutions(genome) == int(hit.sum())
    path = tmp_path / "reads.fa"
    reads.write_fasta(str(path), genome_id="g1")
    lines = path.read_text().splitlines()
    assert len(lines) == 2 * n
    assert lines[0] == ">read_g1_5-%d" % (origin[0] >> 1) and lines[1] == bases[0].tobytes().decode()
    assert lines[-2] == ">read_g1_%d-%d" % (5 + n - 1, origin[-1] >> 1)
