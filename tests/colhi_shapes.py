"""What the column-limit tests share (tests/test_colhi_host.py, tests/test_gpu_factored_colskip.py): the deal of
K-factored's units to the waves of a workgroup (covest_amd/csrc/plan_factored.cpp place_units) restated in Python on top
of tests/band_shapes.py, and from it the kernel's per-item column limit `col_hi` (ll_factored.hip; DESIGN.md section
6ac): the largest copy number any unit of the workgroup reads with a weight that matters in an item of the walk.  A
builder wave whose 64 copy numbers all lie above it skips the item."""
import band_shapes as bs

WAVE = 64
MAX_UNITS = 6          # tiles.h kMaxUnits
UNIT_OVERHEAD = 2      # tiles.h kUnitOverhead
SHARED_DIV = 4         # tiles.h kSharedStepsPerMfma
BUILD_COST = 27        # tiles.h kBuildCost
BUILD_COST_LOW = 24    # tiles.h kBuildCostLowKeys
LAST_BUILDER_EXTRA = 4  # tiles.h kLastBuilderExtra
LOW_KEY_TILE = 384     # tiles.h kLowKeyTile
BAND_EXTRA = 4         # tiles.h kBandExtra


def geometry(qts):
    """(columns of G, waves of a workgroup) of a plain part: plan_factored.cpp part_geometry (one workgroup a (c, e))."""
    n_columns = max(qt["t_hi"] for qt in qts) - 1
    n_waves = 4 if (n_columns <= 256 and 2 * len(qts) <= 4 * MAX_UNITS) else 8
    assert 2 * len(qts) <= n_waves * MAX_UNITS, "one workgroup a (c, e): more q-tiles need q-blocks, not restated here"
    return n_columns, n_waves


def build_cost(ktiles, n_items=None):
    """plan_factored.cpp planner_charges: the builders' charge of a histogram (n_items: with a tail, items of the walk)."""
    low = sum(1 for k0, _ in ktiles if k0 <= LOW_KEY_TILE) / float(len(ktiles))
    base = BUILD_COST_LOW if low >= 0.75 else BUILD_COST
    return int(round(base * len(ktiles) / float(n_items or len(ktiles))))


def place_units(qts, charge=BUILD_COST):
    """held[w] = [(q-tile index, half)] as plan_factored.cpp place_units deals them (two buffers: the builders are charged)."""
    n_columns, nw = geometry(qts)
    units = []
    for i, qt in enumerate(qts):
        nsh = qt["nsh"]
        cost = max(1, qt["n_steps"] - nsh) + UNIT_OVERHEAD + ((1 + (nsh + SHARED_DIV - 1) // SHARED_DIV) if nsh else 0)
        units += [(i, 0, cost), (i, 1, cost)]
    units.sort(key=lambda u: -u[2])  # (stable, as std::stable_sort)
    n_bins = min(4, nw)
    bin_load, wave_load = [0] * n_bins, [0] * nw
    for w in range(nw):
        if w * WAVE < n_columns:
            c = charge + (LAST_BUILDER_EXTRA if ((w + 1) * WAVE >= n_columns and w >= n_bins) else 0)
            bin_load[w % n_bins] += c
            wave_load[w] += c
    held = [[] for _ in range(nw)]
    for i, h, cost in units:
        best = -1
        for w in range(nw):
            if len(held[w]) >= MAX_UNITS:
                continue
            if best < 0:
                best = w
                continue
            lb, bb = bin_load[w % n_bins], bin_load[best % n_bins]
            if lb < bb or (lb == bb and wave_load[w] < wave_load[best]):
                best = w
        assert best >= 0
        held[best].append((i, h))
        bin_load[best % n_bins] += cost
        wave_load[best] += cost
    return held


def n_builders(qts):
    n_columns, nw = geometry(qts)
    return min(nw, (n_columns + WAVE - 1) // WAVE)


def band_makers(qts, held):
    """True where a wave that builds nothing exists to make bands (else col_hi stays the whole row)."""
    nb = n_builders(qts)
    return nb < len(held)


def col_floor(qts, held):
    """(FactoredPlan::col_floor, the q-tiles of FactoredPlan::band_extra): the largest copy number read by a unit whose
    band no wave makes (band.h column_limit_of_block).  The waves that build nothing make the bands of their own long
    units (band.h kBandMinShared shared steps or more) and of up to BAND_EXTRA long units of the builders, one a
    q-tile."""
    nb = n_builders(qts)
    if not band_makers(qts, held):
        return max(qt["t_hi"] for qt in qts) - 1, []
    made = {i for mine in held[nb:] for i, _ in mine if qts[i]["nsh"] >= bs.MIN_BAND}
    floor, extra = 1, []
    for w, mine in enumerate(held):
        for i, _ in mine:
            if qts[i]["nsh"] >= bs.MIN_BAND and (i in made or i in extra):
                continue
            if qts[i]["nsh"] >= bs.MIN_BAND and w < nb and len(extra) < BAND_EXTRA:
                extra.append(i)
                continue
            floor = max(floor, qts[i]["t_hi"] - 1)
    return floor, extra


def slot_case(qts, held, n_extra_max=None):
    """A line for tests/colhi_check.cpp: one slot a unit, in the order the waves hold them."""
    nw = len(held)
    tile = [-1] * (nw * MAX_UNITS)
    for w, mine in enumerate(held):
        for k, (i, _) in enumerate(mine):
            tile[w * MAX_UNITS + k] = i
    nsh = [qts[i]["nsh"] if i >= 0 else 0 for i in tile]
    head = [nw, MAX_UNITS, n_builders(qts), 1, 1, BAND_EXTRA if n_extra_max is None else n_extra_max, len(qts)]
    return head + tile + nsh + [0] * len(tile) + [qt["t_hi"] - 1 for qt in qts], tile


def item_ranges(ktiles):
    """(first key, last key counted by the kernel) per entry of col_hi: entry i is item i of the walk, the 64th entry
    every item from the 64th on as one key range (band.h BandBytes); the rows past a short tile's keys counted in."""
    out = []
    for t, (k0, _) in enumerate(ktiles[:WAVE]):
        last = k0 if t < WAVE - 1 else ktiles[-1][0]
        out.append((k0, last + bs.TILE - 1))
    return out


def col_hi_cases(rates, comb, qts, ranges):
    """band_check rows for every (banded q-tile, entry of col_hi), and where each belongs."""
    cases, where = [], []
    for i, qt in enumerate(qts):
        if qt["nsh"] < bs.MIN_BAND:
            continue
        for t, (ka, kb) in enumerate(ranges):
            row = bs.band_case(rates, comb, qt, ka)
            row[-1] = kb
            cases.append(row)
            where.append((i, t))
    return cases, where


def col_hi_table(qts, held, ranges, where, his, n_items):
    """col_hi per item of the walk (the kernel's rule): col_floor, and per banded unit the copy numbers below its
    band's edge, 4 step_hi.  The last tile -- taken first by the walk -- is built in full.  No wave to make bands: the
    whole row."""
    n_columns, _ = geometry(qts)
    if not band_makers(qts, held):
        return [n_columns] * n_items
    floor, _ = col_floor(qts, held)
    table = [floor] * len(ranges)
    for (i, t), (_, hi) in zip(where, his):
        table[t] = max(table[t], bs.STEP * hi)
    out = [table[min(t, WAVE - 1)] for t in range(n_items)]
    out[n_items - 1] = n_columns
    return out


def wave_skips(col_hi, w):
    """Builder wave w (copy numbers 64 w + 1 .. 64 w + 64) skips an item whose limit lies below all of them."""
    return WAVE * w + 1 > col_hi
