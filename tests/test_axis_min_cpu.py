"""The host side of the per-axis minima (covest_amd.grid.merge_axis_minima / resolve_keep, covest_amd.profile, the
interval keys of covest_amd.report.print_output) on hand-made arrays: nothing here needs a GPU."""
import math

import numpy as np
import pytest

INF = math.inf
HALF_CHI2_95 = 0.5 * 3.841458820694124  # chi2_1.ppf(0.95) / 2


# ----------------------------------------------------------------------------- merge_axis_minima
def test_merge_smaller_value_then_lower_index():
    from covest_amd.grid import merge_axis_minima
    a = (np.array([[1.0, 5.0, INF], [2.0, 2.0, INF]]), np.array([[10, 11, -1], [13, 40, -1]]))
    b = (np.array([[1.0, 4.0, 7.0], [3.0, 2.0, INF]]), np.array([[3, 21, 22], [23, 24, -1]]))
    val, idx = merge_axis_minima([a, b])
    assert val.dtype == np.float64 and idx.dtype == np.int64
    assert val.tolist() == [[1.0, 4.0, 7.0], [2.0, 2.0, INF]]
    assert idx.tolist() == [[3, 21, 22], [13, 24, -1]]  # tie: the lower global index; -1 loses to anything
    val2, idx2 = merge_axis_minima([b, a])  # the order of the blocks does not matter
    assert val2.tolist() == val.tolist() and idx2.tolist() == idx.tolist()
    assert a[0][0, 1] == 5.0 and a[1][0, 1] == 11  # the inputs are left alone


def test_merge_nan_and_minus_one_never_win():
    from covest_amd.grid import merge_axis_minima
    a = (np.array([math.nan, INF, 3.0]), np.array([5, -1, 7]))
    b = (np.array([9.0, INF, math.nan]), np.array([6, -1, 2]))
    val, idx = merge_axis_minima([a, b])
    assert val.tolist() == [9.0, INF, 3.0] and idx.tolist() == [6, -1, 7]
    only = merge_axis_minima([a])
    assert only[0].tolist() == [INF, INF, 3.0] and only[1].tolist() == [-1, -1, 7]
    zero_d = merge_axis_minima([(np.array(4.0), np.array(9)), (np.array(4.0), np.array(2))])  # keep nothing: one cell
    assert zero_d[0].shape == () and float(zero_d[0]) == 4.0 and int(zero_d[1]) == 2
    with pytest.raises(ValueError):
        merge_axis_minima([])
    with pytest.raises(ValueError):
        merge_axis_minima([a, (np.zeros(2), np.zeros(2, dtype=np.int64))])


# ----------------------------------------------------------------------------- keep
def test_keep_names_and_numbers_resolve_alike():
    from covest_amd import BasicModel, RepeatsModel
    from covest_amd.grid import resolve_keep
    hist = {1: 10, 2: 5, 3: 1}
    r = RepeatsModel(21, 100, hist, 0, max_error=8)
    b = BasicModel(21, 100, hist, 0, max_error=8)
    assert resolve_keep(r.params, ("coverage", "error_rate")) == resolve_keep(r.params, (0, 1)) == (3, [0, 1])
    assert resolve_keep(r.params, ("q", "q1")) == resolve_keep(r.params, [2, 4]) == (20, [2, 4])
    assert resolve_keep(r.params, ("error_rate", 3)) == (10, [1, 3])
    assert resolve_keep(r.params, ()) == (0, [])
    assert resolve_keep(r.params, range(5)) == (31, [0, 1, 2, 3, 4])
    assert resolve_keep(b.params, ("error_rate",)) == resolve_keep(b.params, (np.int64(1),)) == (2, [1])
    for bad in (("q1",), (2,), (-1,), (0.5,), ("coverage", 0), (1, 1), ("nope",)):
        with pytest.raises(ValueError):
            resolve_keep(b.params, bad)
    with pytest.raises(ValueError):
        resolve_keep(r.params, (5,))


def test_bad_keep_is_refused_before_any_library_call(monkeypatch):
    """A bad `keep` raises ValueError whether or not a device (or even the library) is there."""
    from covest_amd import BasicModel, _capi, profile

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_capi, "lib", no_library)
    m = BasicModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)
    axes = [np.linspace(8.0, 12.0, 3), np.linspace(0.01, 0.05, 2)]
    for bad in (("q",), (0, 0), (2,)):
        with pytest.raises(ValueError):
            profile.profile_negll(m, axes, bad)
    with pytest.raises(ValueError):
        profile.coverage_interval(m, (10.0, 0.03), axes[:1])  # one axis for a two-parameter model: DenseGrid refuses


def test_axis_minima_fails_loudly_without_device(hip_lib):
    from covest_amd import BasicModel, _capi, profile
    if hip_lib.covest_device_count() > 0:
        pytest.skip("a HIP device is present")
    m = BasicModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)
    axes = [np.linspace(8.0, 12.0, 3), np.linspace(0.01, 0.05, 2)]
    with pytest.raises(_capi.CovestHipError):
        profile.profile_negll(m, axes, ("coverage",))
    with pytest.raises(_capi.CovestHipError):
        profile.coverage_interval(m, (10.0, 0.03), axes)


def test_axis_min_entry_point_refuses_a_null_handle(hip_lib):
    import ctypes
    from covest_amd import _capi
    v, i = ctypes.c_double(), ctypes.c_int64()
    assert hip_lib.covest_grid_axis_min(None, 0, 1, ctypes.byref(v), ctypes.byref(i)) == _capi.COVEST_E_INVALID
    assert "covest_grid_axis_min" in _capi.last_error()


# ----------------------------------------------------------------------------- likelihood_interval
def _parabola(x, x0, curv, floor=1000.0):
    return floor + 0.5 * curv * (x - x0) ** 2


def test_interval_closed_on_both_sides_interpolates_linearly():
    from covest_amd.profile import likelihood_interval
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    p = np.array([10.0, 1.0, 0.0, 1.5, 12.0])
    lo, hi, at = likelihood_interval(x, p)
    t = HALF_CHI2_95  # 1.92: between p[1] and p[0] on the left, p[3] and p[4] on the right
    assert at == 2.0
    assert lo == pytest.approx(1.0 + (t - 1.0) * (0.0 - 1.0) / (10.0 - 1.0), rel=1e-14)
    assert hi == pytest.approx(3.0 + (t - 1.5) * (4.0 - 3.0) / (12.0 - 1.5), rel=1e-14)
    # a parabola sampled finely: the interval is x0 +- sqrt(chi2 / curv) up to the chord error
    xs = np.linspace(9.0, 11.0, 2001)
    lo, hi, at = likelihood_interval(xs, _parabola(xs, 10.0, 400.0))
    half = math.sqrt(2 * HALF_CHI2_95 / 400.0)
    assert at == pytest.approx(10.0, abs=1e-12) and lo == pytest.approx(10.0 - half, abs=1e-6) and hi == pytest.approx(10.0 + half, abs=1e-6)
    # a lower level is a narrower interval
    lo68, hi68, _ = likelihood_interval(xs, _parabola(xs, 10.0, 400.0), level=0.68)
    assert lo < lo68 < 10.0 < hi68 < hi


def test_interval_open_sides_are_none_never_the_axis_end():
    from covest_amd.profile import likelihood_interval
    x = np.linspace(0.0, 1.0, 11)
    rising = 5.0 + 30.0 * x  # the minimum at the first node: nothing to the left of it
    lo, hi, at = likelihood_interval(x, rising)
    assert lo is None and at == 0.0 and hi == pytest.approx(HALF_CHI2_95 / 30.0, rel=1e-12)
    falling = rising[::-1].copy()  # ... and at the last node
    lo, hi, at = likelihood_interval(x, falling)
    assert hi is None and at == 1.0 and lo == pytest.approx(1.0 - HALF_CHI2_95 / 30.0, rel=1e-12)
    shallow = 7.0 + 0.1 * (x - 0.5) ** 2  # never rises above the threshold: open on both sides
    assert likelihood_interval(x, shallow) == (None, None, 0.5)
    flat = np.full(11, 3.0)  # a flat profile: the first node is the minimum, both sides open
    assert likelihood_interval(x, flat) == (None, None, 0.0)
    assert likelihood_interval([2.5], [1.0]) == (None, None, 2.5)


def test_interval_non_finite_cells_count_as_outside():
    from covest_amd.profile import likelihood_interval
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    p = np.array([INF, 0.5, 0.0, 0.4, INF, 0.1])
    lo, hi, at = likelihood_interval(x, p)  # the +inf cells bound the interval at the last node inside
    assert (lo, hi, at) == (1.0, 3.0, 2.0)
    p = np.array([math.nan, 0.5, 0.0, 0.4, 9.0, INF])
    lo, hi, at = likelihood_interval(x, p)
    assert lo == 1.0 and at == 2.0 and hi == pytest.approx(3.0 + (HALF_CHI2_95 - 0.4) / 8.6, rel=1e-14)
    with pytest.raises(ValueError):
        likelihood_interval(x, np.full(6, INF))
    with pytest.raises(ValueError):
        likelihood_interval(x, p[:5])
    with pytest.raises(ValueError):
        likelihood_interval(x, p, level=1.0)


def test_model_construction_stays_free_of_scipy():
    import subprocess
    import sys
    from conftest import REPO
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import covest_amd, covest_amd.profile\n"
            "covest_amd.BasicModel(21, 100, {1: 10, 2: 5}, 0, max_error=8)\n"
            "print('scipy' in sys.modules)\n" % REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.stdout.strip() == "False", (out.stdout, out.stderr[-500:])


# ----------------------------------------------------------------------------- genome size, print_output
class _Model:
    """What print_output and the genome-size mapping touch of a model, with no device behind it."""
    params = ('coverage', 'error_rate')
    hist = {1: 100, 2: 50, 7: 3}
    k, r = 21, 100

    def short_name(self):
        return 'basic'

    def correct_c(self, c):
        return c * (self.r - self.k + 1) / self.r

    def compute_loglikelihood(self, *args):
        return -123.5


def test_genome_size_mapping_reverses_the_order():
    from covest_amd.profile import genome_size_at
    m = _Model()
    hist_orig = {1: 1000, 2: 400, 10: 20}
    occurrences = 1000 + 800 + 200
    assert genome_size_at(m, hist_orig, 10.0) == round(occurrences / (10.0 * 0.8))
    assert genome_size_at(m, hist_orig, 10.0, sample_factor=2) == round(occurrences / (20.0 * 0.8))
    assert genome_size_at(m, hist_orig, None) is None  # an open side stays open
    lo, hi = 9.5, 10.5
    sizes = (genome_size_at(m, hist_orig, hi), genome_size_at(m, hist_orig, lo))
    assert sizes[0] < genome_size_at(m, hist_orig, 10.0) < sizes[1]


def test_print_output_with_and_without_intervals():
    from covest_amd import __version__
    from covest_amd.report import print_output
    m = _Model()
    hist_orig = {1: 1000, 2: 400, 10: 20}
    plain = print_output(hist_orig, m, True, 2, estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True)
    assert plain == {  # today's record, key for key
        'model': 'basic', 'hist_size': 7, 'sample_factor': 2, 'orig_sample_factor': 1, 'success': True,
        'version': __version__, 'starting_points': 1, 'use_grid_search': False,
        'guessed_coverage': 18.0, 'guessed_error_rate': 0.1, 'guessed_loglikelihood': -123.5,
        'coverage': 20.0, 'error_rate': 0.05, 'orig_coverage': 20.0, 'loglikelihood': -123.5,
        'genome_size': round(2000 / (20.0 * 0.8)),
    }
    assert list(plain) == list(print_output(hist_orig, m, True, 2, estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True,
                                            intervals=None))
    iv = {'coverage_interval': (19.6, 20.5), 'genome_size_interval': (122, 128), 'level': 0.95, 'coverage_argmin': 20.0,
          'estimate': (10.0, 0.05)}
    with_iv = print_output(hist_orig, m, True, 2, estimated=(10.0, 0.05), guess=(9.0, 0.1), silent=True, intervals=iv)
    assert {k: v for k, v in with_iv.items() if k in plain} == plain
    assert set(with_iv) - set(plain) == {'coverage_interval', 'genome_size_interval', 'interval_level'}
    assert with_iv['coverage_interval'] == [19.6, 20.5] and with_iv['genome_size_interval'] == [122, 128]
    assert with_iv['interval_level'] == 0.95
    import yaml
    assert yaml.safe_load(yaml.dump(with_iv)) == with_iv  # plain data: the record still prints as YAML
    open_iv = dict(iv, coverage_interval=(None, 20.5), genome_size_interval=None)
    rec = print_output(hist_orig, m, True, 2, estimated=(10.0, 0.05), silent=True, intervals=open_iv)
    assert rec['coverage_interval'] == [None, 20.5] and rec['genome_size_interval'] is None
