"""What the GPU parity tests share (tests/test_gpu_parity.py, tests/test_gpu_variants.py): the comparison at 1e-9
relative with IEEE specials identical, and the graded slack of the tail term tail * log(1 - sp_j) with its committed
budgets (tests/golden/tail_noise_bounds.json); and the bounds of the derivative tests."""
import json
import math
import os

from conftest import load_hist, rel_err

TOL = 1e-9


class _Slack(list):
    """Per point the absolute difference tolerated in the tail term (a list of floats) plus `classes`: per point
    None (the plain 1e-9 decides), "graded" (the conditioning-proportional slack is wider than 1e-10 |LL|) or
    "flip" (the reference's own term is a coin toss); `unit`: |tail| eps / (1 - sp_j) per point, the first-order
    price of ONE eps of error in sp_j (0 where there is no tail term to speak of; for reports)."""
    classes = ()
    unit = ()


def _check(got, want, what, tol=TOL, slack=None):
    """slack[i] > 0: the absolute difference tolerated at point i when the relative one exceeds `tol` (see
    _tail_slack).  Returns the worst relative error among the points that met `tol`."""
    worst, used, worst_use = 0.0, 0, 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        e = rel_err(float(a), float(b))
        if e > tol and slack is not None and slack[i] > 0 and abs(float(a) - float(b)) <= slack[i]:
            used += 1
            worst_use = max(worst_use, abs(float(a) - float(b)) / slack[i])
            continue
        assert e <= tol, "%s[%d]: got %r want %r (rel %.3g%s)" % (
            what, i, float(a), float(b), e,
            "" if slack is None or not slack[i] else ", |diff| %.3g > tail slack %.3g" % (abs(float(a) - float(b)), slack[i]))
        worst = max(worst, e)
    if used:
        print("%s: %d of %d points beyond 1e-9 but inside the tail slack (largest share of it used: %.2g)" % (
            what, used, len(want), worst_use))
    return worst


def _model(case, hist=None):
    """The model of a fixture's case (tests/test_gpu_gradient.py, tests/test_gpu_hessian.py)."""
    from covest_amd import BasicModel, RepeatsModel
    hist = load_hist(case["hist"]) if hist is None else hist
    if case["model"] == "repeats":
        return RepeatsModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"],
                            threshold=case.get("threshold", 1e-8),
                            min_single_copy_ratio=case.get("min_single_copy_ratio", 0.3))
    return BasicModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"], max_cov=case.get("max_cov"))


K_TAIL = 8.0  # rounding errors of K eps per key are granted to the GPU's sp_j (first-order propagation)


# ---- the derivative tests' bounds (tests/test_gpu_gradient.py, _hessian.py, _opg.py, _deriv_shapes.py): the plain TOL applied
# to the quantity's own condition sum from the 50-digit fixture, plus the first-order propagation of the slack
# delta = K_TAIL eps n_keys the parity suite grants sp (only where there is a live tail term: tail != 0 and sp < 1)
def _tail_delta(n_keys):
    return K_TAIL * 2.0 ** -52 * n_keys


def _grad_bound(tail, sp, C, D, delta):
    """|g_k - want| <= TOL C_k + |tail| D_k delta / (1 - sp)^2, D_k = |sum_j d_k p_j|."""
    return TOL * C + (abs(tail) * D * delta / (1 - sp) ** 2 if tail and sp < 1 else 0.0)


def _hess_bound(tail, sp, C, D2, Dk, Dl, delta):
    """|H_kl - want| <= TOL C_kl + s_kl, s_kl = |tail| (D2_kl delta / (1 - sp)^2 + 2 D_k D_l delta / (1 - sp)^3)."""
    s_kl = 0.0
    if tail and sp < 1:
        s_kl = abs(tail) * (D2 * delta / (1 - sp) ** 2 + 2 * Dk * Dl * delta / (1 - sp) ** 3)
    return TOL * C + s_kl


def _opg_slack(tail, sp, Dk, Dl, delta):
    """s_kl = |tail| 2 |S_k| |S_l| delta / (1 - sp)^3 (tests/golden/opg.json stores it as `s`)."""
    return abs(tail) * 2 * Dk * Dl * delta / (1 - sp) ** 3 if tail and sp < 1 else 0.0


def _opg_bound(C, s_kl):
    """|B_kl - want| <= TOL C_kl + s_kl."""
    return TOL * C + s_kl


def _tail_slack(tail, ll, sp, n_keys):
    """What may separate a correct implementation from the reference in the tail term tail * log(1 - sp_j)
    (covest/models.py:103-104), given the sp_j = fsum(p_j) the REFERENCE saw.  The p_j of two correct
    implementations differ by rounding, so their sp_j differ by up to delta = K eps n_keys and the term by
    |tail| |log(1 - delta / (1 - sp_j))| ~ |tail| delta / (1 - sp_j): a slack GRADED by the conditioning, e.g.
    7e-5 absolute at the optimum of the trimmed C3 histogram (1 - sp_j = 1e-4, 380 keys, tail 11 192) against
    1e-9 |LL| = 0.1 -- there the term is simply checked.  Only where |1 - sp_j| <= delta -- the reference's term
    itself hangs on the last bits of an fsum: it flips between 0 (sp_j rounds to >= 1) and tail * log(k 2^-53) -- is
    the old absolute allowance of 40 |tail| (|log 2^-53| = 36.7) kept: the FLIP class.  sp_j > 1 + delta (the
    reference's 200-chunk normaliser makes some pmfs too large) is no coin toss: the term is 0 on
    both sides.  Returns (slack, class, unit) -- see _Slack."""
    if not tail or not math.isfinite(ll):
        return 0.0, None, 0.0
    eps = 2.0 ** -52
    delta = K_TAIL * eps * n_keys
    if sp - 1.0 > delta:
        return 0.0, None, 0.0
    gap = 1.0 - sp
    if gap <= delta:
        return 40.0 * abs(tail), "flip", 0.0
    slack = min(40.0, -math.log1p(-delta / gap)) * abs(tail)
    return slack, ("graded" if slack > 1e-10 * abs(ll) else None), abs(tail) * eps / gap


def _slack_of(tail, lls, sps, n_keys):
    out, classes, unit = _Slack(), [], []
    for ll, sp in zip(lls, sps):
        v, c, u = _tail_slack(tail, ll, sp, n_keys)
        out.append(v)
        classes.append(c)
        unit.append(u)
    out.classes, out.unit = classes, unit
    return out


def _tail_noise(om, points, lls, tail):
    """_tail_slack for every point of a case whose reference values come from the oracle: sp_j = fsum of the
    oracle's p_j (bit-equal to the reference's, tests/test_oracle_golden.py)."""
    if not tail:
        out = _Slack([0.0] * len(lls))
        out.classes, out.unit = [None] * len(lls), [0.0] * len(lls)
        return out
    sps = [math.fsum(om.compute_probabilities(*p).values()) if math.isfinite(ll) else 1.0 for p, ll in zip(points, lls)]
    return _slack_of(tail, lls, sps, len(om.hist))


_BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_noise_bounds.json")
_RECORD = os.environ.get("COVEST_RECORD_TAIL_BOUNDS")  # a path: write the counts there instead of checking them
_recorded = {}


def _slack_budget(name, slack):
    """The slack must stay the exception: how many points of case `name` fall into the FLIP class and how many into
    the GRADED one (a property of the reference's / the oracle's numbers alone, so the same on every box) may not
    exceed the counts committed in tests/golden/tail_noise_bounds.json.  A change that widened the criterion until
    every tail point fell under it would fail here.  COVEST_RECORD_TAIL_BOUNDS=<path> records instead (new cases)."""
    n_flip = sum(1 for c in slack.classes if c == "flip")
    n_graded = sum(1 for c in slack.classes if c == "graded")
    if _RECORD:
        _recorded[name] = {"flip": n_flip, "graded": n_graded, "points": len(slack)}
        with open(_RECORD, "w") as f:
            json.dump(_recorded, f, indent=0, sort_keys=True)
        return n_flip + n_graded
    with open(_BOUNDS_PATH) as f:
        bounds = json.load(f)
    assert name in bounds, "no committed tail-slack bound for case %r" % name
    b = bounds[name]
    assert n_flip <= b["flip"] and n_graded <= b["graded"], (
        "case %r: %d flip / %d graded points under the tail slack, committed bounds %d / %d of %d" % (
            name, n_flip, n_graded, b["flip"], b["graded"], b["points"]))
    return n_flip + n_graded
