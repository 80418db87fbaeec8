"""Posterior classes on the GPU (covest_posterior_classes over csrc/posterior.hip) against the 50-digit yardstick
(tests/golden/posterior.json, tests/posterior_reference.py) and against the shapes its layout can break.

Bounds, from the project's bar on a log pmf (tests/test_gpu_tp.py: 1e-9, plus 4 eps of the magnitude): with
delta_j = 1e-9 + 4 eps L_j on every ln w, L_j the largest |ln w_os(j)| of finite weight,
    |ln p got - want| <= delta_j,      |share or mean got - want| <= 2 delta_j want + 4.94e-324,
and a family's row sums to 1 within 4 eps (number of terms).  Models are made here from small key sets; where a shape is
not in the fixture its reference is computed here by the same 50-digit code, never by the code under test.  Printed
while passing: the worst ratio of error to bound per output."""
import ctypes
import math

import numpy as np
import pytest

from conftest import load_golden, load_hist
import posterior_reference as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
_GOLDEN = load_golden("posterior.json")
_CASES = {c["name"]: c for c in _GOLDEN["cases"]}
_DP = ctypes.POINTER(ctypes.c_double)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _model(cs):
    from covest_amd import BasicModel, RepeatsModel
    hist = {int(j): 1 for j in cs["keys"]}
    if cs["kind"] == "basic":
        return BasicModel(cs["k"], cs["r"], hist, 0, max_error=cs["max_error"])
    return RepeatsModel(cs["k"], cs["r"], hist, 0, max_error=cs["max_error"], threshold=cs["threshold"])


def _threshold_of(model, point):
    """T of a point as the library's host rule gives it (covest_threshold_o); 2 in the basic model."""
    if model.param_count == 2:
        return 2
    return int(model.get_hist_threshold_values(np.asarray([model.fit_to_bounds(list(point))[2:5]]))[0])


def _per_copy_number(cs):
    """{key: (row, C_o for o = 1 .. T - 1)} of a case: from the fixture where its columns are wide enough, else computed
    here at copy_columns = T by the yardstick's code."""
    T = cs["T"]
    for c in _CASES.values():
        if c["name"] == cs["name"] or c.get("wide_of") == cs["name"]:
            if c["copy_columns"] >= max(T - 1, 1) and c["copy_columns"] >= cs["copy_columns"]:
                return {int(j): (row, row["C"][:max(T - 1, 1)]) for j, row in c["rows"].items()}
    wide = dict(cs, copy_columns=max(T, 1))
    got, _ = ref.compute_case(wide)
    assert got["T"] == T
    return {int(j): (row, row["C"][:max(T - 1, 1)]) for j, row in got["rows"].items()}


def _lumped(per_o, columns):
    out = list(per_o[:columns - 1]) + [math.fsum(per_o[columns - 1:])]
    return out + [0.0] * (columns - len(out))


class _Worst:
    def __init__(self):
        self.ratio = {"ln_p": 0.0, "E": 0.0, "C": 0.0, "M": 0.0, "sum_E": 0.0, "sum_C": 0.0}
        self.where = {}

    def note(self, what, err, bound, where):
        r = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        if not r <= self.ratio[what]:
            self.ratio[what], self.where[what] = r, where

    def report(self, title):
        print("%s: worst error / bound  ln p %.3g, E %.3g, C %.3g, M %.3g, row sums E %.3g, C %.3g"
              % (title, self.ratio["ln_p"], self.ratio["E"], self.ratio["C"], self.ratio["M"], self.ratio["sum_E"],
                 self.ratio["sum_C"]))

    def check(self):
        bad = {k: (v, self.where.get(k)) for k, v in self.ratio.items() if not v <= 1.0}
        assert not bad, bad


def _compare(worst, name, keys, got, want_rows, columns, n_terms_c):
    """One point's arrays against {key: (row, lumped C)}."""
    log_p, err, cop, mean = got
    for i, j in enumerate(keys):
        row, want_c = want_rows[j]
        d = ref.delta(row["L"])
        where = (name, j, columns)
        worst.note("ln_p", abs(log_p[i] - row["ln_p"]), d, where)
        for s, w in enumerate(row["E"]):
            worst.note("E", abs(err[i, s] - w), ref.share_bound(w, row["L"]), where + (s,))
        for c, w in enumerate(want_c):
            worst.note("C", abs(cop[i, c] - w), ref.share_bound(w, row["L"]), where + (c,))
        worst.note("M", abs(mean[i] - row["M"]), ref.share_bound(row["M"], row["L"]), where)
        worst.note("sum_E", abs(math.fsum(err[i]) - 1), 4 * EPS * err.shape[1], where)
        worst.note("sum_C", abs(math.fsum(cop[i]) - 1), 4 * EPS * n_terms_c, where)


def test_fixture(hip_lib):
    """Every case of posterior.json within the bounds."""
    worst = _Worst()
    for cs in _GOLDEN["cases"]:
        m = _model(cs)
        assert _threshold_of(m, cs["point"]) == cs["T"], cs["name"]
        got = m.posterior_classes_points([cs["point"]], copy_columns=cs["copy_columns"])
        want = {int(j): (row, row["C"]) for j, row in cs["rows"].items()}
        _compare(worst, cs["name"], cs["keys"], [a[0] for a in got], want, cs["copy_columns"],
                 max(1, min(cs["copy_columns"], cs["T"] - 1)))
        m.close()
    worst.report("fixture, %d cases" % len(_GOLDEN["cases"]))
    worst.check()


@pytest.mark.parametrize("max_error,k,r", [(1, 21, 100), (2, 21, 100), (8, 21, 100), (22, 21, 100), (33, 32, 150),
                                           (64, 63, 150)])
def test_classes_of_the_repeats_model(hip_lib, max_error, k, r):
    """S classes under several copy numbers (T = 5): 64 / S copy numbers a lot in prepare_mix_lot, one for S = 33, 64."""
    cs = {"name": "rep_s%d" % max_error, "kind": "repeats", "k": k, "r": r, "max_error": max_error, "keys": [1, 2, 5],
          "eval_keys": [1, 2, 5], "threshold": 1e-8, "point": [12.0, 0.04, 0.5, 0.4, 0.3], "copy_columns": 6}
    want, _ = ref.compute_case(cs)
    assert want["T"] == 5
    m = _model(cs)
    assert _threshold_of(m, cs["point"]) == 5
    got = m.posterior_classes_points([cs["point"]], copy_columns=6)
    worst = _Worst()
    _compare(worst, cs["name"], cs["keys"], [a[0] for a in got], {int(j): (row, row["C"]) for j, row in want["rows"].items()},
             6, 4)
    worst.report(cs["name"])
    worst.check()
    # ... and exp(ln p) against the existing kernel
    p = m.compute_probabilities(*cs["point"], clamp=True)
    for i, j in enumerate(cs["keys"]):
        assert abs(math.exp(got[0][0, i]) / p[j] - 1) <= 1e-9


@pytest.mark.parametrize("name", ["rep_q1_one", "rep_t3", "rep_t9", "rep_t10", "rep_t400"])
def test_copy_numbers_and_columns(hip_lib, name):
    """T = 2, 3, 64 / S + 1, 64 / S + 2 (S = 8) and 400, each at copy_columns in {1, 2, 3, T - 1, T, T + 5}: against the
    yardstick's per-copy-number shares lumped the same way, and the lumped column against the sum of the widest call's
    columns to T eps relative."""
    cs = _CASES[name]
    T = cs["T"]
    assert T == {"rep_q1_one": 2, "rep_t3": 3, "rep_t9": 64 // 8 + 1, "rep_t10": 64 // 8 + 2, "rep_t400": 400}[name]
    per_o = _per_copy_number(cs)
    m = _model(cs)
    assert _threshold_of(m, cs["point"]) == T
    worst = _Worst()
    calls = {}
    for columns in sorted({1, 2, 3, max(T - 1, 1), T, T + 5}):
        got = [a[0] for a in m.posterior_classes_points([cs["point"]], copy_columns=columns)]
        calls[columns] = got
        want = {j: (row, _lumped(c, columns)) for j, (row, c) in per_o.items()}
        _compare(worst, name, cs["keys"], got, want, columns, max(1, min(columns, T - 1)))
        assert (got[2][:, T - 1:] == 0.0).all()  # columns beyond T - 1
    wide = calls[T + 5]
    for columns, got in calls.items():
        assert _same((got[0], got[1], got[3]), (wide[0], wide[1], wide[3])), columns  # nothing else hangs on the columns
        # (a family is divided by the sum of its own columns, which is added up in another order at another copy_columns)
        single = wide[2][:, :columns - 1]
        assert (np.abs(got[2][:, :columns - 1] - single) <= T * EPS * single).all(), columns
        lump = np.array([math.fsum(r) for r in wide[2][:, columns - 1:]])
        assert (np.abs(got[2][:, columns - 1] - lump) <= T * EPS * lump).all(), columns
    worst.report("%s, T = %d" % (name, T))
    worst.check()
    m.close()


def _basic(keys, max_error=8):
    from covest_amd import BasicModel
    return BasicModel(21, 100, {int(j): 1 for j in keys}, 0, max_error=max_error)


@pytest.fixture(scope="module")
def by_key(hip_lib):
    """The basic and the repeats model's numbers at keys 1 .. 257 and 10000, one key a model at a time would hang on: a
    key's numbers depend on the key alone (the repeats model's T on the largest key, which is 10000 in every set)."""
    from covest_amd import RepeatsModel
    keys = list(range(1, 258)) + [10000]
    b = _basic(keys)
    r = RepeatsModel(21, 100, {j: 1 for j in keys}, 0, max_error=8)
    pb, pr = [9.0, 0.06], [9.0, 0.06, 0.6, 0.5, 0.4]
    out = {"keys": keys, "pb": pb, "pr": pr,
           "basic": [a[0] for a in b.posterior_classes_points([pb], copy_columns=3)],
           "repeats": [a[0] for a in r.posterior_classes_points([pr], copy_columns=3)],
           "p_basic": b.compute_probabilities(*pb, clamp=True), "p_repeats": r.compute_probabilities(*pr, clamp=True)}
    b.close()
    r.close()
    return out


def test_against_the_existing_kernel_over_many_keys(by_key):
    for kind in ("basic", "repeats"):
        log_p, err, cop, mean = by_key[kind]
        p = by_key["p_" + kind]
        n = 0
        for i, j in enumerate(by_key["keys"]):
            if p[j] >= ref.TINY:
                assert abs(math.exp(log_p[i]) / p[j] - 1) <= 1e-9, (kind, j)
                n += 1
        assert n >= 150 and np.isfinite(log_p).all()
        assert (np.abs(err.sum(axis=1) - 1) <= 4 * EPS * err.shape[1]).all()
        assert (np.abs(cop.sum(axis=1) - 1) <= 4 * EPS * cop.shape[1]).all()


@pytest.mark.parametrize("keys", [[1], list(range(1, 64)), list(range(1, 65)), list(range(1, 66)), list(range(1, 258)),
                                  [1, 2, 3, 7, 150, 10000], list(range(100, 0, -1)) + [10000]],
                         ids=["1", "63", "64", "65", "257", "gaps", "100_descending"])
def test_key_counts_around_lane_and_tile_edges(by_key, keys):
    """A wave owns 64 keys and stages 16 columns at a time: 1, 63, 64, 65 and 257 keys, keys with gaps and one large
    key, keys out of order.  Whatever the set and a key's place in it, a key's numbers are the same bytes."""
    from covest_amd import RepeatsModel
    at = {j: i for i, j in enumerate(by_key["keys"])}
    pick = [at[j] for j in keys]
    b = _basic(keys)
    got = [a[0] for a in b.posterior_classes_points([by_key["pb"]], copy_columns=3)]
    assert _same(got, [a[pick] for a in by_key["basic"]])
    b.close()
    if max(keys) == 10000:  # (the repeats model's T hangs on the largest key)
        r = RepeatsModel(21, 100, {j: 1 for j in keys}, 0, max_error=8)
        got = [a[0] for a in r.posterior_classes_points([by_key["pr"]], copy_columns=3)]
        assert _same(got, [a[pick] for a in by_key["repeats"]])
        r.close()


def test_bounds_of_the_parameters(hip_lib):
    from covest_amd import RepeatsModel
    keys = [1, 2, 5, 12]
    r = RepeatsModel(21, 100, {j: 1 for j in keys}, 0, max_error=8)
    # e = 0: only the error-free class has a rate
    log_p, err, cop, mean = [a[0] for a in r.posterior_classes_points([[10.0, 0.0, 0.6, 0.5, 0.3]])]
    assert (err[:, 0] == 1.0).all() and (err[:, 1:] == 0.0).all() and np.isfinite(log_p).all()
    # e = 0.5 (the upper bound): finite, rows sum to 1
    log_p, err, cop, mean = [a[0] for a in r.posterior_classes_points([[10.0, 0.5, 0.6, 0.5, 0.3]])]
    assert np.isfinite(log_p).all() and (np.abs(err.sum(axis=1) - 1) <= 4 * EPS * 8).all()
    # q1 = 1: one copy, exactly
    log_p, err, cop, mean = [a[0] for a in r.posterior_classes_points([[10.0, 0.05, 1.0, 0.5, 0.5]])]
    assert (cop[:, 0] == 1.0).all() and (cop[:, 1:] == 0.0).all() and (mean == 1.0).all()
    # (q2 in {0, 1} and q in {0, 1}: cases rep_q2_zero, rep_q2_one, rep_q_zero, rep_q_one of the fixture)
    # outside the bounds: clamp=True is the clamped point byte for byte, clamp=False is another point
    outside, clamped = [0.001, 0.7, 0.1, 1.5, -0.2], [0.01, 0.5, 0.3, 1.0, 0.0]
    assert r.fit_to_bounds(outside) == clamped
    a = r.posterior_classes_points([outside], clamp=True)
    assert _same(a, r.posterior_classes_points([clamped], clamp=True))
    assert _same(a, r.posterior_classes_points([clamped], clamp=False))
    mild = [10.0, 0.05, 0.2, 0.5, 0.3]  # q1 below its bound only: a point the raw method evaluates as it is
    assert not _same(r.posterior_classes_points([mild], clamp=True), r.posterior_classes_points([mild], clamp=False))
    # no component with weight (a coverage of 0, taken as given): no posterior exists
    log_p, err, cop, mean = [a[0] for a in r.posterior_classes_points([[0.0, 0.05, 0.6, 0.5, 0.3]], copy_columns=20,
                                                                      clamp=False)]
    assert (log_p == -math.inf).all() and np.isnan(err).all() and np.isnan(cop).all() and np.isnan(mean).all()
    r.close()


@pytest.mark.parametrize("name,key", [("basic_high_cov", 1), ("basic_low_cov", 10000), ("rep_high_cov", 1)])
def test_underflow(hip_lib, name, key):
    """Where compute_probabilities returns 0 or a subnormal, ln p is finite and within delta of the fixture, and the
    shares are finite and sum to 1."""
    cs = _CASES[name]
    m = _model(cs)
    p = m.compute_probabilities(*cs["point"], clamp=True)[key]
    assert 0.0 <= p < ref.TINY, p
    log_p, err, cop, mean = [a[0] for a in m.posterior_classes_points([cs["point"]], copy_columns=cs["copy_columns"])]
    i = cs["keys"].index(key)
    row = cs["rows"][str(key)]
    assert row["ln_p"] < math.log(ref.TINY)
    assert math.isfinite(log_p[i]) and abs(log_p[i] - row["ln_p"]) <= ref.delta(row["L"])
    assert np.isfinite(err[i]).all() and np.isfinite(cop[i]).all() and math.isfinite(mean[i])
    assert abs(math.fsum(err[i]) - 1) <= 4 * EPS * err.shape[1]
    assert abs(math.fsum(cop[i]) - 1) <= 4 * EPS * cop.shape[1]
    m.close()


def test_against_the_existing_kernel(hip_lib):
    """exp(log_p) against compute_probabilities(clamp=True), 1e-9 relative where that value is normal: on
    sim_c10_e0.05.hist, and on one repeats point of the fixture."""
    from covest_amd import BasicModel
    hist = load_hist("sim_c10_e0.05")
    b = BasicModel(21, 100, hist, 0, max_error=8)
    log_p = b.posterior_classes_points([[10.0, 0.05]])[0][0]
    p = b.compute_probabilities(10.0, 0.05, clamp=True)
    n = 0
    for i, j in enumerate(hist):
        if p[j] >= ref.TINY:
            assert abs(math.exp(log_p[i]) / p[j] - 1) <= 1e-9, j
            n += 1
    assert n >= 10
    b.close()
    cs = _CASES["rep_threshold_row"]
    m = _model(cs)
    log_p = m.posterior_classes_points([cs["point"]])[0][0]
    p = m.compute_probabilities(*cs["point"], clamp=True)
    for i, j in enumerate(cs["keys"]):
        assert p[j] >= ref.TINY and abs(math.exp(log_p[i]) / p[j] - 1) <= 1e-9, j
    m.close()


def test_determinism_and_the_list_property(hip_lib):
    """The same call twice is the same bytes; five points in one call are the five single calls, byte for byte -- also
    with the points walked in chunks of two (a chunk edge inside the list) and of one."""
    from covest_amd import RepeatsModel
    keys = list(range(1, 71)) + [300]
    r = RepeatsModel(21, 100, {j: 1 for j in keys}, 0, max_error=8)
    pts = np.array([[10.0, 0.05, 0.6, 0.5, 0.3], [3.0, 0.01, 1.0, 0.5, 0.5], [25.0, 0.1, 0.4, 0.9, 0.05],
                    [10.0, 0.05, 0.5, 0.0, 0.3], [7.5, 0.2, 0.35, 0.2, 0.7]])
    ts = [_threshold_of(r, p) for p in pts]
    assert len(set(ts)) >= 3 and min(ts) == 2 and max(ts) > 64, ts  # each point its own T, in one table stride
    for columns in (4, max(ts) + 5):
        whole = r.posterior_classes_points(pts, copy_columns=columns)
        assert _same(whole, r.posterior_classes_points(pts, copy_columns=columns))
        for i in range(5):
            one = r.posterior_classes_points(pts[i:i + 1], copy_columns=columns)
            assert _same(one, [a[i:i + 1] for a in whole]), (columns, i)
        for chunk in (1, 2, 3):
            assert _same(whole, r.posterior_classes_points(pts, copy_columns=columns, _chunk_points=chunk)), chunk
    r.close()


def _guarded(shape, pad=8):
    """(whole, view): `view` of `shape` inside `whole`, `pad` sentinel doubles either side."""
    n = int(np.prod(shape))
    whole = np.full(n + 2 * pad, -7.25)
    return whole, whole[pad:pad + n].reshape(shape)


def test_null_outputs_and_guards(hip_lib):
    from covest_amd import RepeatsModel
    keys = list(range(1, 71))
    K, S, Cc, n = len(keys), 8, 5, 3
    r = RepeatsModel(21, 100, {j: 1 for j in keys}, 0, max_error=S)
    pts = np.array([[10.0, 0.05, 0.6, 0.5, 0.3], [3.0, 0.01, 1.0, 0.5, 0.5], [25.0, 0.1, 0.4, 0.9, 0.05]])
    shapes = [(n, K), (n, K, S), (n, K, Cc), (n, K)]

    def call(skip=None):
        bufs = [_guarded(s) for s in shapes]
        ptrs = [None if i == skip else b[1].ctypes.data_as(_DP) for i, b in enumerate(bufs)]
        rc = hip_lib.covest_posterior_classes(r.handle, n, pts.ctypes.data_as(_DP), 1, Cc, *ptrs)
        assert rc == 0
        for i, (whole, view) in enumerate(bufs):
            assert (whole[:8] == -7.25).all() and (whole[-8:] == -7.25).all(), i  # guards either side
            if i == skip:
                assert (view == -7.25).all()
            else:
                assert not (view == -7.25).any()
        return [b[1] for b in bufs]

    full = call()
    assert _same(full, r.posterior_classes_points(pts, copy_columns=Cc))
    for skip in range(4):
        part = call(skip)
        for i in range(4):
            if i != skip:
                assert np.array_equal(_bits(part[i]), _bits(full[i])), (skip, i)
    # T - 1 < copy_columns: the columns the device does not store are filled on the host, inside the array
    wide = _guarded((n, K, 600))
    assert hip_lib.covest_posterior_classes(r.handle, n, pts.ctypes.data_as(_DP), 1, 600, None, None,
                                            wide[1].ctypes.data_as(_DP), None) == 0
    assert (wide[0][:8] == -7.25).all() and (wide[0][-8:] == -7.25).all()
    assert (np.abs(wide[1][:, :, :Cc - 1] - full[2][:, :, :Cc - 1]) <= 70 * EPS * full[2][:, :, :Cc - 1]).all()
    assert (wide[1][:, :, 70:] == 0).all()
    r.close()


def test_basic_model_has_one_copy_number(hip_lib):
    m = _basic([1, 2, 3, 50])
    log_p, err, cop, mean = [a[0] for a in m.posterior_classes_points([[10.0, 0.05]], copy_columns=3)]
    assert (cop[:, 0] == 1.0).all() and (cop[:, 1:] == 0.0).all() and (mean == 1.0).all()
    one = m.posterior_classes_points([[10.0, 0.05]], copy_columns=1)
    assert (one[2] == 1.0).all() and _same((one[0], one[1], one[3]), ([log_p], [err], [mean]))
    m.close()


def test_error_codes(hip_lib):
    from covest_amd import _capi
    m = _basic([1, 2, 3])
    pts = np.array([[10.0, 0.05]])
    out = [np.full(s, -7.25) for s in ((1, 3), (1, 3, 8), (1, 3, 4), (1, 3))]
    ptrs = [a.ctypes.data_as(_DP) for a in out]
    f, p = hip_lib.covest_posterior_classes, pts.ctypes.data_as(_DP)
    for args, word in (((None, 1, p, 1, 4) + tuple(ptrs), "model"),
                       ((m.handle, -1, p, 1, 4) + tuple(ptrs), "n is negative"),
                       ((m.handle, 1, None, 1, 4) + tuple(ptrs), "params"),
                       ((m.handle, 1, p, 1, 0) + tuple(ptrs), "copy_columns"),
                       ((m.handle, 1, p, 1, 65537) + tuple(ptrs), "copy_columns"),
                       ((m.handle, 1, p, 1, 4, None, None, None, None), "output")):
        assert f(*args) == _capi.COVEST_E_INVALID, word
        assert "covest_posterior_classes" in _capi.last_error() and word in _capi.last_error(), _capi.last_error()
    assert f(m.handle, 0, None, 1, 4, *ptrs) == 0  # n == 0: nothing to do, nothing written
    assert all((a == -7.25).all() for a in out)
    assert f(m.handle, 1, p, 1, 65536, ptrs[0], ptrs[1], None, ptrs[3]) == 0
    m.close()


def test_summary(hip_lib):
    """posterior_classes -> error_cutoff and expected_kmers, recomputed in numpy from the raw arrays."""
    from covest_amd import BasicModel, posterior_classes
    hist = load_hist("sim_c10_e0.05")
    b = BasicModel(21, 100, hist, 0, max_error=8)
    est = (10.0, 0.05)
    pc = posterior_classes(b, est, copy_columns=2)
    log_p, err, cop, mean = [a[0] for a in b.posterior_classes_points([est], copy_columns=2)]
    assert _same((pc.log_p, pc.error_share, pc.copy_share, pc.mean_copies), (log_p, err, cop, mean))
    keys, counts = np.array(list(hist)), np.array(list(hist.values()), dtype=float)
    assert np.array_equal(pc.keys, keys) and np.array_equal(pc.counts, counts)
    bad_share = err[:, 1:].sum(axis=1)
    order = np.argsort(keys)
    cutoff = None
    for i in order[::-1]:  # from the largest key down, while the share stays below
        if not bad_share[i] < 0.5:
            break
        cutoff = int(keys[i])
    assert pc.error_cutoff() == cutoff and cutoff is not None and 1 < cutoff < 10
    got = pc.expected_kmers()
    want = {"erroneous": float((counts * bad_share).sum()), "error_free": float((counts * err[:, 0]).sum()),
            "copies_1": float((counts * cop[:, 0]).sum()), "copies_ge_2": float((counts * cop[:, 1]).sum()), "undefined": 0.0}
    assert set(got) == set(want)
    for name, v in want.items():
        assert abs(got[name] - v) <= 1e-12 * abs(v), name
    assert abs(got["erroneous"] + got["error_free"] - counts.sum()) <= 1e-9 * counts.sum()
    b.close()
