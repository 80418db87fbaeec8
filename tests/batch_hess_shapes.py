"""The shapes of the batch Hessian's fixture (tests/golden/batch_hess.json): tests/batch_grad_shapes.py's sixteen, imported
unchanged, and two more for the one edge that is new at second order.  The table holds R2 = 1 + P + P (P + 1) / 2 rows a
point (6 for the basic model, 21 for repeats) and the contraction takes its R2 n rows 64 a wave: the basic shapes' n = 21
and 22 (126 and 132 rows) lie either side of the second wave's end as they are, the repeat model's n = 10 and 11 (210 and
231) lie inside one.  So two repeats shapes with n = 3 and n = 4: 63 rows, one short of a wave, and 84.

They are cut from "repeats-k65-B15-n11", not drawn: its first five rows (the model's own counts, the two all-zero rows, two
seeded rows) at its first n points -- the same model, so batch_grad.json's value and gradient of those (b, i) are theirs
too.  No device, no library, no mpmath.

STORED_ROWS: the fixture keeps every row of a shape with B < 15; of a larger one the model's-own-counts row, the two
all-zero rows (tail 1, tail 0), the first and the last seeded row -- the device evaluates every row all the same."""
import functools

import batch_grad_shapes as S

SEED, K, R, MAX_ERROR, ISOLATED = S.SEED, S.K, S.R, S.MAX_ERROR, S.ISOLATED
BASE = "repeats-k65-B15-n11"
CUTS = {"repeats-k65-B5-n3": (BASE, 5, 3), "repeats-k65-B5-n4": (BASE, 5, 4)}  # name -> (shape cut from, rows, points)
SHAPES = dict(S.SHAPES)
SHAPES.update({name: ("repeats", 65, B, n, {"cut_from": base}) for name, (base, B, n) in CUTS.items()})


def rows_per_point(kind):
    P = 2 if kind == "basic" else 5
    return 1 + P + P * (P + 1) // 2


@functools.lru_cache(maxsize=None)
def shape(name):
    """batch_grad_shapes.shape's dict; for a cut shape the base's with its first rows and points, and "base": (the base's
    name) under which batch_grad.json has the value and gradient of the same (b, i)."""
    if name not in CUTS:
        return dict(S.shape(name), base=name)
    base, B, n = CUTS[name]
    src = S.shape(base)
    assert max(src["rows"].values()) < B - 2 and n <= src["n_inside"]
    return dict(src, name=name, counts=src["counts"][:B].copy(), tails=src["tails"][:B].copy(),
                points=src["points"][:n].copy(), n_inside=n, base=base)


def stored_rows(name):
    """The rows of a shape the fixture stores, ascending."""
    case = shape(name)
    B = case["counts"].shape[0]
    if B < 15:
        return list(range(B))
    named = set(case["rows"].values())
    seeded = [b for b in range(B) if b not in named]
    return sorted(named | {seeded[0], seeded[-1]})
