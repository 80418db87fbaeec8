"""covest_amd/csrc/band.h on the host: the band K-factored cuts a unit's contraction to, against
the exact weighted terms in the log domain (tests/band_shapes.py).  For every (c, e) of C3's axes at stride 3, all 16
q-tiles and every key tile of H10k_rep and of H10k_rep_trim -- and for the small grids of tests/test_gpu_factored_band.py
-- the terms outside the returned band must stay below 2^-64 of every column's sum; on C3 the band must be active (the
share of steps it keeps is printed: DESIGN.md quotes it); and the program runs once under the address and
undefined-behaviour sanitizers, as a binary of its own."""
import numpy as np
import pytest

import band_shapes as bs
from conftest import load_hist

LIMIT = 2.0 ** -64
C3_AXES = [np.linspace(15.0, 30.0, 32), np.linspace(0.005, 0.08, 32), np.linspace(0.3, 0.95, 16), np.array([0.5]),
           np.linspace(0.05, 0.95, 16)]


@pytest.fixture(scope="module")
def band_exe(tmp_path_factory):
    return bs.build_band_check(tmp_path_factory.mktemp("band"))


def sweep(exe, cs, es, qts, ktiles, k=21, r=100):
    """Every (c, e, q-tile long enough for a band, key tile): the band, and the share outside it.  Returns
    (worst share outside, steps kept, steps in all -- of every q-tile's units --, bands refused, bands cut)."""
    keys = [k0 + b for k0, nb in ktiles for b in range(nb)]
    col0 = np.cumsum([0] + [nb for _, nb in ktiles])
    banded = [qt for qt in qts if qt["nsh"] >= bs.MIN_BAND]
    o_top = max(qt["t_hi"] for qt in qts) - 1
    cases, where = [], []
    for c in cs:
        for e in es:
            rates, comb = bs.classes(k, r, c, e)
            for qt in banded:
                for t, (k0, _) in enumerate(ktiles):
                    cases.append(bs.band_case(rates, comb, qt, k0))
                    where.append((c, e, qt["q"], t))
    his = bs.run_band_check(exe, cases)
    worst, kept, total, refused, cut = 0.0, 0, 0, 0, 0
    cut_low = sweep.cut_low = [0]
    at = 0
    for c in cs:
        for e in es:
            rates, comb = bs.classes(k, r, c, e)
            lg = bs.log_terms(rates, comb, o_top, keys)
            for qt in banded:
                for t in range(len(ktiles)):
                    lo, hi = his[at]
                    assert 1 <= hi <= qt["n_steps"], (where[at], hi)
                    share = bs.outside_share(lg[:, col0[t]:col0[t + 1]], qt, (lo, hi))
                    assert share < LIMIT, (where[at], lo, hi, qt, share)
                    worst = max(worst, share)
                    kept += hi - max(lo - 1, 0)
                    cut_low[0] += lo > 0
                    total += qt["n_steps"]
                    refused += hi == qt["n_steps"]
                    cut += hi < qt["n_steps"]
                    at += 1
    assert at == len(his)
    # (the units without a band run their full range)
    plain = sum(qt["n_steps"] for qt in qts if qt["nsh"] < bs.MIN_BAND) * len(ktiles) * len(cs) * len(es)
    return worst, kept + plain, total + plain, refused, cut


@pytest.mark.parametrize("hist_name", ["H10k_rep", "H10k_rep_trim"])
def test_band_is_safe_and_active_on_c3(band_exe, hist_name):
    hist = load_hist(hist_name)
    # (without a tail only the keys with a count are evaluated; the trimmed histogram has a count at every key)
    ktiles = bs.key_tiles([j for j, h in hist.items() if h])
    qts = bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], max(hist))
    assert len(qts) == 16 and sum(qt["nsh"] >= bs.MIN_BAND for qt in qts) >= 4  # (the short tiles, large q, have no band)
    worst, kept, total, refused, cut = sweep(band_exe, C3_AXES[0][::3], C3_AXES[1][::3], qts, ktiles)
    print("\n%s: %d key tiles, %d bands, %d refused (full range), %d cut; steps kept %d of %d = %.1f %%; largest share "
          "outside a band %.3g (limit %.3g); cut at the lower edge %d" % (hist_name, len(ktiles), refused + cut, refused, cut, kept,
                                                                        total, 100.0 * kept / total, worst, LIMIT, sweep.cut_low[0]))
    assert refused > 0, "the early tiles must keep the full range"
    # the band is not trivially the full range: with nothing cut the share would be 1
    assert kept < 0.9 * total, (kept, total)


def test_band_on_the_small_grids_of_the_gpu_test(band_exe):
    import test_gpu_factored_band as g
    ktiles = bs.key_tiles(g.HIST)
    assert len(ktiles) == 10 and sum(1 for a, b in zip(ktiles, ktiles[1:]) if b[0] != a[0] + a[1]) == 1
    for name, axes in g.GRIDS.items():
        qts = bs.q_tiles(axes[2], axes[3], axes[4], max(g.HIST))
        worst, kept, total, refused, cut = sweep(band_exe, axes[0], axes[1], qts, ktiles)
        print("\n%s: q-tiles (q, nsh, steps) %s; %d bands refused, %d cut; steps kept %d of %d; largest share outside %.3g" % (
            name, [(qt["q"], qt["nsh"], qt["n_steps"]) for qt in qts], refused, cut, kept, total, worst))
        for want in g.SITUATIONS[name]:
            if want == "refused":
                assert refused > 0, name
            elif want == "cut":
                assert cut > 0, name
            elif want == "unbanded":
                assert any(qt["nsh"] < bs.MIN_BAND for qt in qts), name
            elif want == "banded":
                assert any(qt["nsh"] >= bs.MIN_BAND for qt in qts), name


def test_band_of_a_key_range_wider_than_a_tile(band_exe):
    """The kernel's last lane stands for every item from the 64th on: one band for the keys from that item's first to the
    histogram's last (tests/test_gpu_factored_band.py LONG_HIST: keys 2017 .. 2200).  The same bound must hold for every
    key of the range."""
    import test_gpu_factored_band as g
    ktiles = bs.key_tiles(g.LONG_HIST)
    assert len(ktiles) == 69
    k_lo, k_hi = ktiles[63][0], ktiles[-1][0] + bs.TILE - 1
    keys = list(range(k_lo, max(g.LONG_HIST) + 1))
    qts = bs.q_tiles(g.LONG_GRID[2], g.LONG_GRID[3], g.LONG_GRID[4], max(g.LONG_HIST))
    cut = 0
    for c in list(g.LONG_GRID[0]) + [60.0, 120.0]:  # (the larger rates: ranges whose band cuts)
        rates, comb = bs.classes(21, 100, c, 0.02)
        lg = bs.log_terms(rates, comb, max(qt["t_hi"] for qt in qts) - 1, keys)
        for qt in qts:
            row = bs.band_case(rates, comb, qt, k_lo)
            row[-1] = k_hi
            lo, hi = bs.run_band_check(band_exe, [row])[0]
            assert bs.outside_share(lg, qt, (lo, hi)) < LIMIT, (c, qt, lo, hi)
            cut += hi < qt["n_steps"] or lo > 0
    assert cut > 0


def test_band_check_under_sanitizers(tmp_path):
    exe = bs.build_band_check(tmp_path, sanitize=True)
    rates, comb = bs.classes(21, 100, 20.0, 0.03)
    qts = bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], 10000)
    cases = [bs.band_case(rates, comb, qt, k0) for qt in qts for k0 in range(1, 982, 32)]
    # (and what a grid's edges can hand it: no rate, q = 1, a unit with two steps, not-a-numbers)
    odd = bs.band_case(rates, comb, qts[0], 1)
    for at, v in ((0, 0.0), (17, float("-inf")), (19, 2.0), (0, float("nan")), (20, float("nan"))):
        row = list(odd)
        row[at] = v
        cases.append(row)
    his = bs.run_band_check(exe, cases)
    full = qts[0]["n_steps"]
    assert all(h >= 1 for _, h in his)
    assert [his[i] for i in (-5, -4, -2, -1)] == [(0, full)] * 4 and his[-3][0] == 0 and 1 <= his[-3][1] <= 2, his[-5:]
