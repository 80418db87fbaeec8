"""The planner's charges and its deal of K-factored's units to waves on the host (DESIGN.md section 6ah;
covest_amd/csrc/unit_deal.h, through tests/deals_check.cpp): the planner's own code on C3's axes -- the strong grid has
the same q axes and histogram, so the same units --, on the GPU test's grid and on the 69-tile one, against the deal
restated in tests/test_gpu_factored_wave_charges.py; the column limit's planner part (band.h column_limit_of_block,
tests/colhi_check.cpp) on THAT deal's slots -- col_floor and band_extra -- against tests/colhi_shapes.py; every shape
the shares are gated off for (fewer than 192 pairs, a chunked part, list modes, more than 8 error classes, low keys)
dealt as tests/colhi_shapes.py deals, which is the deal of the commit before; the column limit's safety against the
exact terms (tests/test_colhi_host.py limits) on the deal C3 really gets; and the overrides of tuning builds, once
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import band_shapes as bs
import colhi_shapes as cs
from conftest import load_hist
from test_band_host import C3_AXES
from test_colhi_host import build_colhi_check, limits, run_colhi_check, walk_skips
from test_gpu_factored_band import LONG_HIST
from test_gpu_factored_wave_charges import EVEN, GRID, HIGH_HIST, LONG_GRID, SHARES, place_units

OPEN = dict(one_block=1, list_mode=0, n_pass=1, o_base=0, low_keys=0)


def build_deals_check(out_dir, sanitize=False, tune=False):
    cxx = bs.host_compiler()
    assert cxx is not None, "no host C++ compiler: the planner's deal cannot be checked"
    exe = os.path.join(str(out_dir), "deals_check%s%s" % ("_san" if sanitize else "", "_tune" if tune else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + (["-DCOVEST_TUNE"] if tune else []) +
                           ["-I", bs.CSRC, os.path.join(bs.HERE, "deals_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def units_of(qts):
    """(q-tile, half, cost) by falling cost, as plan_factored.cpp place_units sorts them (one pass)."""
    units = []
    for i, qt in enumerate(qts):
        nsh = qt["nsh"]
        cost = max(1, qt["n_steps"] - nsh) + cs.UNIT_OVERHEAD + ((1 + (nsh + cs.SHARED_DIV - 1) // cs.SHARED_DIV) if nsh else 0)
        units += [(i, 0, cost), (i, 1, cost)]
    units.sort(key=lambda u: -u[2])
    return units


def case_line(qts, charge, one_block, list_mode, n_pass, o_base, low_keys):
    n_columns, nw = cs.geometry(qts)
    units = units_of(qts)
    return [nw, n_columns, 1, cs.MAX_UNITS, one_block, list_mode, n_pass, o_base, low_keys, charge, cs.LAST_BUILDER_EXTRA,
            len(units)] + [u[2] for u in units]


def run_deals_check(exe, cases, env=None):
    text = "".join(" ".join(str(int(v)) for v in row) + "\n" for row in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, **env) if env else None)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return [[int(x) for x in line.split()] for line in run.stdout.splitlines()]


def held_of(qts, wave_of):
    _, nw = cs.geometry(qts)
    held = [[] for _ in range(nw)]
    for (i, h, _), w in zip(units_of(qts), wave_of):
        held[w].append((i, h))
    return held


def shapes():
    return {"C3 and the strong grid": (bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], 10000), cs.BUILD_COST),
            "192 pairs": (bs.q_tiles(GRID[2], GRID[3], GRID[4], max(HIGH_HIST)), cs.build_cost(bs.key_tiles(HIGH_HIST))),
            "69 tiles": (bs.q_tiles(LONG_GRID[2], LONG_GRID[3], LONG_GRID[4], max(LONG_HIST)), cs.build_cost(bs.key_tiles(LONG_HIST)))}


def test_planner_deal_against_its_restatement(tmp_path):
    exe, colhi = build_deals_check(tmp_path), build_colhi_check(tmp_path)
    gated = [dict(OPEN, one_block=0), dict(OPEN, list_mode=3, o_base=512), dict(OPEN, list_mode=1), dict(OPEN, list_mode=2),
             dict(OPEN, n_pass=3), dict(OPEN, o_base=512), dict(OPEN, low_keys=1)]
    changed = 0
    for name, (qts, charge) in shapes().items():
        got = run_deals_check(exe, [case_line(qts, charge, **g) for g in [OPEN] + gated])
        # where the shares apply: the restated deal with them, each (q-tile, half) held once, no wave beyond its slots
        held = held_of(qts, got[0])
        assert held == place_units(qts, charge, SHARES), name
        assert sorted(u for mine in held for u in mine) == sorted((i, h) for i in range(len(qts)) for h in (0, 1)), name
        assert max(len(mine) for mine in held) <= cs.MAX_UNITS, name
        changed += held != cs.place_units(qts, charge)
        # ... and that deal's col_floor and band_extra, by the planner's rule, equal the restatement's
        row, tile = cs.slot_case(qts, held)
        out = run_colhi_check(colhi, [row])[0]
        floor, extra = cs.col_floor(qts, held)
        assert out[0] == floor and [tile[s] for s in out[1:] if s >= 0] == extra, (name, out, floor, extra)
        # every gated-off shape: the one charge, the deal of the commit before
        for g, wave_of in zip(gated, got[1:]):
            assert held_of(qts, wave_of) == cs.place_units(qts, charge), (name, g)
    assert changed >= 2, "the shares change no deal: nothing is tested"
    # (C3's own deal is among the changed ones: the benchmark's grid runs the new tables)
    qts, charge = shapes()["C3 and the strong grid"]
    assert place_units(qts, charge, SHARES) != cs.place_units(qts, charge)


def test_column_limit_is_safe_on_the_deal_c3_gets(monkeypatch, tmp_path):
    """tests/test_colhi_host.py's check of the limit against the exact terms, on the deal with the shares."""
    band_exe = bs.build_band_check(tmp_path)
    hist = load_hist("H10k_rep")
    ktiles = bs.key_tiles([j for j, h in hist.items() if h])
    qts = bs.q_tiles(C3_AXES[2], C3_AXES[3], C3_AXES[4], max(hist))
    monkeypatch.setattr(cs, "place_units", lambda q, charge=cs.BUILD_COST: place_units(q, charge, SHARES))
    tables, worst, held = limits(band_exe, C3_AXES[0][::3], C3_AXES[1][::3], qts, ktiles, cs.build_cost(ktiles))
    assert held == place_units(qts, cs.BUILD_COST, SHARES)
    nb = cs.n_builders(qts)
    skipped = [sum(sum(walk_skips(tb, w)[0]) for tb in tables.values()) for w in range(nb)]
    floor, extra = cs.col_floor(qts, held)
    print("\nC3 with the shares: col_floor %d, extra q-tiles %s, skipped by wave %s of %d, largest share above a limit %.3g" % (
        floor, extra, skipped, len(tables) * len(ktiles), worst))
    assert nb == 5 and skipped[0] == 0 and floor < cs.WAVE and sum(skipped[2:]) > 0.3 * 3 * len(tables) * len(ktiles)


def test_tuning_overrides_under_the_sanitizers(tmp_path):
    """The environment's lists as the tuning library reads them (unit_deal.h env_int_list, Charges::build_of): even
    shares give the deal of the commit before; absolute charges equal to the shares' give the shares' deal; a list that
    is short, overlong or no list changes nothing it does not reach; no override reaches a gated-off shape."""
    plain, san = build_deals_check(tmp_path, tune=True), build_deals_check(tmp_path, sanitize=True, tune=True)
    qts, charge = shapes()["C3 and the strong grid"]
    lines = [case_line(qts, charge, **OPEN), case_line(qts, charge, **dict(OPEN, one_block=0))]
    want_new, want_old = place_units(qts, charge, SHARES), cs.place_units(qts, charge)
    absolute = ",".join(str((charge * s + 50) // 100) for s in SHARES)
    for exe in (plain, san):
        for env, first in (({}, want_new),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": ",".join(str(s) for s in EVEN)}, want_old),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": "100,100,100,100,100,100,100,100,100,100,100"}, want_old),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": ",".join(str(s) for s in EVEN), "COVEST_FACTORED_BUILD_COST_WAVES": absolute}, want_new),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": ""}, want_new),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": "x,1"}, want_new),
                           ({"COVEST_FACTORED_BUILD_SHARE_WAVES": "100,,7"}, want_new),
                           ({"COVEST_FACTORED_BUILD_COST_WAVES": "-5,99999999999999999999"}, None)):
            got = run_deals_check(exe, lines, env)
            if first is not None:
                assert held_of(qts, got[0]) == first, env
            assert held_of(qts, got[1]) == want_old, env
