"""The shapes of the batch gradient's fixture (tests/golden/batch_grad.json): what tests/golden/make_golden_batch_grad.py
evaluates at 50 digits and tests/test_gpu_batch_grad.py on the device -- the model's histogram, the batch's rows and the
points of every shape, from integers and one seeded generator.  No device, no library, no mpmath.

The edges: n_keys in {1, 63, 65, 255, 256, 257} (the wave, the contraction's 16-key step with its 4-key lane groups, the
derivative kernel's 256-key segment), B in {1, 15, 17, 65} (the 16-histogram tile, the 64-histogram workgroup), and n
such that the (P + 1) n table rows straddle a wave's 64: {1, 21, 22} for the basic model, {1, 10, 11} for repeats -- a
covering subset of the product, each edge in at least one shape of each model; one repeats shape with max_error = 3, one
whose points have threshold_o - 1 below, on and beyond one lot of kWave / S = 8 copy numbers, and one shape per model
around the dead key of tests/golden/deriv_shapes.json's `neg_inf` case.

Points.  e, q1, q2, q lie inside the ranges of tests/test_gpu_deriv_shapes.py::test_more_points_than_one_launch (e in
the lower part, 0.005 .. 0.03: at a higher error rate the saturated error classes leave the error-free class a
thousandth of the weight, and with it 1 - sum p_j).  The coverage does NOT lie in that test's 5 .. 15: on keys
1 .. n_keys such a coverage leaves 1 - sum p_j below a double's resolution from 63 keys on -- every row with a tail
would fall into the flip class of tests/parity_helpers.py _tail_slack and be dropped, far beyond the 5 % the generator
allows -- and p_j = 0 in a double at the upper keys.  So the coverage is set from the rate of the error-free class, 1.0 ..
1.4 times the largest key (basic; 0.5 .. 0.7 times for repeats, whose second copy number then reaches past the keys), as
tests/golden/make_golden_deriv_shapes.py and tests/test_gpu_batch.py place theirs.  The last two points of a list of ten
or more lie outside the bounds: basic e < 0 and c > max_cov (the shape's model has one), repeats q1 below its lower
bound and (e < 0, q > 1); their coverage goes with the error rate AFTER the clamp, so that the rate stays where it was
drawn (the repeats point's at 0.6 times the largest key).

Two choices are the all-zero row with tail 1's.  Its gradient is the tail coefficient -S_k / (1 - sp) alone and its
condition sum |t| alone, so the fixture's bound asks for S_c = sum_j d_c p_j to 1e-9 OF ITSELF; where S_c is a 1e-7th of
sum_j |d_c p_j| or less no double evaluation of the per-key terms delivers that.  So the repeats dead-key shape has five
copy numbers (DEAD_Q, LOT_THRESHOLD: the upper ones reach past key 256; with two, all mass lies inside the keys and
S_c / sum |d_c p_j| is 6e-12), and the (e < 0, q > 1) point's rate is set, not drawn (one draw had 4e-7).  With them the
smallest ratio over every point that such a row meets is 1e-4."""
import functools

import numpy as np

SEED = 20250311
K, R, MAX_ERROR = 21, 100, 8
ISOLATED = 3000  # the dead key of deriv_shapes.json's neg_inf case (histogram isolated257)
LOT = 64 // MAX_ERROR  # copy numbers prepared per lot (ll_deriv.hip: OT = kWave / S)

# name -> (model, n_keys, B, n, options)
SHAPES = {
    "basic-k1-B1-n1": ("basic", 1, 1, 1, {}),
    "basic-k63-B15-n21": ("basic", 63, 15, 21, {}),
    "basic-k65-B5-n22": ("basic", 65, 5, 22, {}),
    "basic-k255-B65-n1": ("basic", 255, 65, 1, {}),
    "basic-k256-B5-n21": ("basic", 256, 5, 21, {}),
    "basic-k257-B17-n1": ("basic", 257, 17, 1, {}),
    "basic-dead": ("basic", 257, 3, 8, {"dead": True}),
    "repeats-k1-B17-n1": ("repeats", 1, 17, 1, {}),
    "repeats-k63-B1-n10": ("repeats", 63, 1, 10, {}),
    "repeats-k65-B15-n11": ("repeats", 65, 15, 11, {}),
    "repeats-k255-B17-n1": ("repeats", 255, 17, 1, {}),
    "repeats-k256-B65-n1": ("repeats", 256, 65, 1, {}),
    "repeats-k257-B15-n10": ("repeats", 257, 15, 10, {}),
    "repeats-k65-B5-n11-S3": ("repeats", 65, 5, 11, {"max_error": 3}),
    "repeats-k65-B5-n10-lot": ("repeats", 65, 5, 10, {"lot": True}),
    "repeats-dead": ("repeats", 257, 3, 8, {"dead": True}),
}
LOT_THRESHOLD = 1e-3                      # the lot shape's model threshold: threshold_o follows q closely
LOT_TM1 = (5, LOT - 1, LOT, LOT, LOT + 1, LOT + 2, 2 * LOT + 1)  # threshold_o - 1 of its first seven points ...
LOT_Q = (0.9, 0.72, 0.64, 0.62, 0.57, 0.51, 0.28)                # ... and the q that gives it at q1 = 0.4, q2 = 0.3
MAX_COV_RATE, MAX_COV_E = 1.5, 0.03       # a basic shape's max_cov: where the rate is 1.5 times the largest key at e = 0.03
DEAD_POINT = [142.185, 0.03]              # deriv_shapes.json neg_inf: p_3000 = 1e-3824
DEAD_Q = [0.4, 0.3, 0.9]                  # repeats: with LOT_THRESHOLD threshold_o - 1 = 5 (LOT_Q's first entry), so that the
                                          # upper copy numbers reach past key 256 and 1 - sum p_j is not all cancellation


def _own_hist(n_keys, dead):
    """The model's own histogram (integers only; make_golden_deriv_shapes._hist's bell): keys 1 .. n_keys (30 alone),
    or for the dead-key shapes deriv_shapes.json's isolated257: keys 1 .. 256 and 3000 with count 2."""
    if dead:
        keys = list(range(1, 257)) + [ISOLATED]
        mode, width = 60, 40
    else:
        keys = [30] if n_keys == 1 else list(range(1, n_keys + 1))
        mode, width = (30, 4) if n_keys == 1 else (7 * n_keys // 10, max(4, n_keys // 6))
    counts = [1 + 4000 * width * width // (width * width + (j - mode) ** 2) for j in keys]
    if dead:
        counts[-1] = 2
    return keys, counts


def _c_of(lam0, e):
    return lam0 / ((R - K + 1) / R * (1.0 - e) ** K)


@functools.lru_cache(maxsize=None)
def shape(name):
    """{"spec": the model's case (tests/parity_helpers._model; `hist` inline as keys and counts), "counts" (B, n_keys),
    "tails" (B,), "rows": {"own", "zero_tail1", "zero_tail0", "dead", "alive"} -> row, "points" (n, P), "n_inside": the
    points before the two outside the bounds, "lot_tm1": the threshold_o - 1 asked of the lot shape's first points}."""
    kind, n_keys, B, n, opt = SHAPES[name]
    at = list(SHAPES).index(name)
    rng = np.random.default_rng([SEED, at])
    dead = bool(opt.get("dead"))
    keys, own = _own_hist(n_keys, dead)
    assert len(keys) == n_keys
    top = 256 if dead else max(keys)
    own_tail = 0 if dead or at % 2 == 0 else 37
    spec = {"model": kind, "hist": {"keys": keys, "counts": own}, "k": K, "r": R, "tail": own_tail,
            "max_error": opt.get("max_error", MAX_ERROR)}
    if kind == "basic" and not dead:
        spec["max_cov"] = float(round(_c_of(MAX_COV_RATE * top, MAX_COV_E)))  # (above every point drawn inside)
    if opt.get("lot"):
        spec["threshold"] = LOT_THRESHOLD
    if dead and kind == "repeats":
        spec["threshold"] = LOT_THRESHOLD
    # ---- rows
    counts = rng.integers(0, 10 ** 6 + 1, size=(B, n_keys)).astype(np.float64)
    counts[rng.random((B, n_keys)) < 1.0 / 3.0] = 0.0
    tails = np.where(np.arange(B) % 2 == 1, rng.integers(1, 10 ** 5, size=B), 0).astype(np.float64)
    rows = {"own": 0}
    counts[0], tails[0] = own, own_tail
    if dead:
        rows.update(dead=0, alive=1, zero_tail1=2)
        counts[1], tails[1] = own, 0
        counts[1, keys.index(ISOLATED)] = 0.0
        counts[2], tails[2] = 0.0, 1.0
    elif B >= 3:
        rows.update(zero_tail1=1, zero_tail0=2)
        counts[1], tails[1] = 0.0, 1.0
        counts[2], tails[2] = 0.0, 0.0
    # ---- points
    e = rng.uniform(0.005, 0.03, n)
    lam0 = rng.uniform(1.0, 1.4, n) * top if kind == "basic" else rng.uniform(0.5, 0.7, n) * top
    if kind == "basic":
        pts = np.stack([_c_of(lam0, e), e], axis=1)
    else:
        pts = np.stack([_c_of(lam0, e), e, rng.uniform(0.3, 0.8, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.3, 0.9, n)], axis=1)
    n_inside = n
    if dead:  # the dead point first; beside it points at which key 3000 has mass and the first error class covers the low keys
        # (no rate o lambda_s just above a multiple of 200: there the reference's chunked normaliser hangs on the rounding
        # of the rate, tests/golden/make_golden_deriv_shapes.py rule 2)
        scale = (1730.0, 2370.0) if kind == "basic" else (1330.0, 1670.0)
        pts[:, 1] = 0.02
        pts[:, 0] = _c_of(np.linspace(scale[0], scale[1], n), 0.02)
        if kind == "repeats":
            pts[:, 2:] = DEAD_Q
        pts[0, :2] = DEAD_POINT
    elif n >= 10:
        n_inside = n - 2
        if kind == "basic":  # (the coverage goes with the error rate AFTER the clamp: the rate stays where it was drawn)
            pts[n - 2] = [_c_of(lam0[n - 2], 0.0), -0.1]
            pts[n - 1] = [2.0 * spec["max_cov"], MAX_COV_E]
        else:
            pts[n - 2, 2] = 0.1
            pts[n - 1, :2] = [_c_of(0.6 * top, 0.0), -0.05]
            pts[n - 1, 4] = 1.5
    lot_tm1 = None
    if opt.get("lot"):  # q1 = 0.4, q2 = 0.3 and the q at which threshold_o - 1 is LOT_TM1[i] (the generator asserts it)
        lot_tm1 = list(LOT_TM1)
        for i, q in enumerate(LOT_Q):
            pts[i, 2:] = [0.4, 0.3, q]
    return {"name": name, "kind": kind, "n_keys": n_keys, "spec": spec, "counts": counts, "tails": tails, "rows": rows,
            "points": np.ascontiguousarray(pts), "n_inside": n_inside, "lot_tm1": lot_tm1, "dead": dead}
