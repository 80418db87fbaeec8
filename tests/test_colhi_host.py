"""K-factored's column limit on the host (covest_amd/csrc/band.h column_limit_of_block,
ll_factored.hip col_hi): per item of the walk the largest copy number any unit of a workgroup reads with a weight that
matters -- a builder wave whose 64 copy numbers all lie above it skips the item.  The rule, restated in
tests/colhi_shapes.py, against the exact weighted terms in the log domain (tests/band_shapes.py): for every (c, e) of
C3's axes at stride 3, every key tile of H10k_rep and H10k_rep_trim and EVERY q-tile -- the ones without a band too --
the terms in the columns above the limit stay below 2^-64 of every column's sum, key by key.  The skipped share of the
(builder wave, key tile) pairs is printed (DESIGN.md quotes it).  The small grids of
tests/test_gpu_factored_colskip.py must hold every situation a skip can go wrong in; and the planner's part of the
rule runs in a program of its own, once under the address and undefined-behaviour sanitizers."""
import math
import os
import subprocess

import numpy as np
import pytest

import band_shapes as bs
import colhi_shapes as cs
from conftest import load_hist
from test_band_host import C3_AXES

LIMIT = 2.0 ** -64


@pytest.fixture(scope="module")
def band_exe(tmp_path_factory):
    return bs.build_band_check(tmp_path_factory.mktemp("colhi"))


def build_colhi_check(out_dir, sanitize=False):
    cxx = bs.host_compiler()
    assert cxx is not None, "no host C++ compiler: the planner's rule cannot be checked"
    exe = os.path.join(str(out_dir), "colhi_check_san" if sanitize else "colhi_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                           ["-I", bs.CSRC, os.path.join(bs.HERE, "colhi_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run_colhi_check(exe, cases):
    text = "".join(" ".join(str(int(v)) for v in row) + "\n" for row in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return [[int(x) for x in line.split()] for line in run.stdout.splitlines()]


def above_share(lg, qt, col_hi):
    """The largest share, over the keys of lg's columns, of the weighted terms of the copy numbers ABOVE col_hi in a
    column's sum: as band_shapes.outside_share, an upper bound that holds for every column of the q-tile -- the dropped
    copy numbers up to the LARGEST cut-off against the geometric terms (o >= 3) below the SMALLEST one."""
    if qt["t_hi"] - 1 <= col_hi:
        return 0.0  # (nothing of the unit lies above the limit)
    assert qt["t_lo"] - 1 > 2, qt
    ln_r = math.log1p(-qt["q"])
    o = np.arange(1, lg.shape[0] + 1, dtype=np.float64)[:, None]
    w = lg + (o - 3.0) * ln_r
    w = w - w[2:qt["t_lo"] - 1].max(axis=0)
    kept = np.exp(w[2:qt["t_lo"] - 1]).sum(axis=0)
    dropped = np.exp(w[col_hi:qt["t_hi"] - 1]).sum(axis=0)
    return float((dropped / kept).max())


def limits(exe, cs_, es, qts, ktiles, charge, check=True, k=21, r=100):
    """{(c, e): col_hi per item} of a tail-less walk (an item a key tile), each checked against the exact terms."""
    held = cs.place_units(qts, charge)
    ranges = cs.item_ranges(ktiles)
    keys = [k0 + b for k0, nb in ktiles for b in range(nb)]
    col0 = np.cumsum([0] + [nb for _, nb in ktiles])
    o_top = max(qt["t_hi"] for qt in qts) - 1
    cases, per = [], {}
    for c in cs_:
        for e in es:
            rates, comb = bs.classes(k, r, c, e)
            rows, where = cs.col_hi_cases(rates, comb, qts, ranges)
            per[(float(c), float(e))] = (len(cases), where)
            cases += rows
    his = bs.run_band_check(exe, cases) if cases else []
    out, worst = {}, 0.0
    for (c, e), (at, where) in per.items():
        table = cs.col_hi_table(qts, held, ranges, where, his[at:at + len(where)], len(ktiles))
        out[(c, e)] = table
        if not check:
            continue
        rates, comb = bs.classes(k, r, c, e)
        lg = bs.log_terms(rates, comb, o_top, keys)
        for t, hi in enumerate(table):
            for qt in qts:
                share = above_share(lg[:, col0[t]:col0[t + 1]], qt, hi)
                assert share < LIMIT, ((c, e), t, hi, qt, share)
                worst = max(worst, share)
    return out, worst, held


def walk_skips(table, w):
    """Per POSITION of the walk (the last tile first, then the tiles in order): does builder wave w skip?"""
    n = len(table)
    order = [n - 1] + list(range(n - 1)) if n >= 2 else list(range(n))
    return [p > 0 and cs.wave_skips(table[t], w) for p, t in enumerate(order)], order


@pytest.mark.parametrize("hist_name", ["H10k_rep", "H10k_rep_trim"])
def test_column_limit_is_safe_and_active_on_c3(band_exe, hist_name):
    hist = load_hist(hist_name)
    ktiles = bs.key_tiles([j for j, h in hist.items() if h])
    qts = bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], max(hist))
    tables, worst, held = limits(band_exe, C3_AXES[0][::3], C3_AXES[1][::3], qts, ktiles, cs.build_cost(ktiles))
    nb = cs.n_builders(qts)
    floor, extra = cs.col_floor(qts, held)
    skipped = [sum(sum(walk_skips(tb, w)[0]) for tb in tables.values()) for w in range(nb)]
    pairs = len(tables) * len(ktiles)
    print("\n%s: %d key tiles, %d builder waves, col_floor %d, builders' long q-tiles handed to the band-making waves %s; "
          "skipped (wave, tile) pairs by wave %s %% (all: %.1f %%); largest share above a limit %.3g (limit %.3g)" % (
              hist_name, len(ktiles), nb, floor, [round(qts[i]["q"], 2) for i in extra],
              " / ".join("%.0f" % (100.0 * s / pairs) for s in skipped), 100.0 * sum(skipped) / (pairs * nb), worst, LIMIT))
    assert nb == 5 and skipped[0] == 0 and floor < cs.WAVE, (nb, skipped, floor)
    # the limit is not trivially the whole row: the upper builder waves skip a third of their tiles or more
    assert sum(skipped[2:]) > 0.3 * 3 * pairs, (skipped, pairs)


def test_situations_of_the_gpu_grids(band_exe):
    """tests/test_gpu_factored_colskip.py cannot pass vacuously: its grids hold a pair that never skips, a wave that
    skips and never returns, one that skips and re-enters, a re-entry on the run start behind the key gap, skips in
    both buffers, and a skip at an item from the 64th on."""
    import test_gpu_factored_colskip as g
    ktiles = bs.key_tiles(g.HIST)
    assert len(ktiles) == 10 and ktiles[7][0] == 260 and ktiles[6][1] < bs.TILE
    found = set()
    for name, axes in g.GRIDS.items():
        qts = bs.q_tiles(axes[2], axes[3], axes[4], max(g.HIST))
        tables, _, held = limits(band_exe, axes[0], axes[1], qts, ktiles, cs.build_cost(ktiles))
        nb = cs.n_builders(qts)
        print("\n%s: %d builder waves of %d, col_floor %s" % (name, nb, len(held), cs.col_floor(qts, held)))
        for (c, e), tb in sorted(tables.items()):
            for w in range(1, nb):
                sk, order = walk_skips(tb, w)
                print("  c %.4g e %.4g wave %d: %s" % (c, e, w, "".join("s" if s else "." for s in sk)))
                if not any(sk):
                    found.add("never skips")
                    continue
                first = sk.index(True)
                if all(sk[first:]):
                    found.add("skips and never returns")
                back = [p for p in range(2, len(sk)) if sk[p - 1] and not sk[p]]
                if back:
                    found.add("skips and re-enters")
                if any(order[p] == 7 for p in back):
                    found.add("re-enters on the run start")
                if {p & 1 for p, s in enumerate(sk) if s} == {0, 1}:
                    found.add("both buffers")
    lk = bs.key_tiles(g.LONG_HIST)
    qts = bs.q_tiles(g.LONG_GRID[2], g.LONG_GRID[3], g.LONG_GRID[4], max(g.LONG_HIST))
    tables, _, _ = limits(band_exe, g.LONG_GRID[0], g.LONG_GRID[1], qts, lk, cs.build_cost(lk))
    assert len(lk) == 69
    for tb in tables.values():
        for w in range(1, cs.n_builders(qts)):
            sk, order = walk_skips(tb, w)
            if any(s and order[p] >= cs.WAVE for p, s in enumerate(sk)):
                found.add("an item from the 64th on")
    assert found == {"never skips", "skips and never returns", "skips and re-enters", "re-enters on the run start",
                     "both buffers", "an item from the 64th on"}, found


def test_planner_rule_against_its_restatement(tmp_path):
    """band.h column_limit_of_block on the slots of C3's and the GPU grids' workgroups against tests/colhi_shapes.py,
    with the list of extra slots cut short too; and once under the sanitizers."""
    import test_gpu_factored_colskip as g
    shapes = [bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], 10000)]
    shapes += [bs.q_tiles(a[2], a[3], a[4], max(g.HIST)) for a in g.GRIDS.values()]
    cases, want = [], []
    for qts in shapes:
        for charge in (18, 24, 27, 40):
            held = cs.place_units(qts, charge)
            for n_extra in (cs.BAND_EXTRA, 1, 0):
                row, tile = cs.slot_case(qts, held, n_extra)
                cases.append(row)
                want.append((qts, held, n_extra, tile))
    # (all waves build: no bands at all; not a plain grid: the same)
    row, tile = cs.slot_case(shapes[0], cs.place_units(shapes[0]))
    cases += [row[:2] + [8] + row[3:], row[:3] + [0] + row[4:]]
    for exe in (build_colhi_check(tmp_path), build_colhi_check(tmp_path, sanitize=True)):
        got = run_colhi_check(exe, cases)
        for (qts, held, n_extra, tile), out in zip(want, got):
            saved, cs.BAND_EXTRA = cs.BAND_EXTRA, n_extra
            try:
                floor, extra = cs.col_floor(qts, held)
            finally:
                cs.BAND_EXTRA = saved
            assert out[0] == floor and [tile[s] for s in out[1:] if s >= 0] == extra, (out, floor, extra, n_extra)
        top = max(qt["t_hi"] for qt in shapes[0]) - 1
        assert got[-2] == [top] + [-1] * cs.BAND_EXTRA and got[-1] == [top] + [-1] * cs.BAND_EXTRA, got[-2:]
