"""The bootstrap-t interval without a device: the interval arithmetic on made-up arrays, the free-set
rules in the one helper observed_information and observed_information_batch share, observed_information's dict for a
stubbed model (what it was before the rules moved), and the batch form on a stubbed batch: one pairs call."""
import math

import numpy as np
import pytest

NAMES = ["coverage", "error_rate", "q1"]


def test_the_interval_arithmetic():
    from covest_amd.bootstrap import t_intervals
    rng = np.random.default_rng(5)
    B = 40
    est = np.array([10.0, 0.05, 0.7]) + rng.standard_normal((B, 3)) * [0.2, 0.002, 0.01]
    rse = np.abs(rng.standard_normal((B, 3))) * [0.05, 0.0005, 0.0] + [0.2, 0.002, 0.0]
    ok = np.ones(B, dtype=bool)
    ok[[3, 17]] = False
    rse[5, 0] = math.nan   # a successful replicate without a standard error for the coverage
    rse[:, 2] = math.nan   # no replicate has one for q1 (fixed, say)
    se = {"coverage": 0.21, "error_rate": None, "q1": 0.01}
    iv, used = t_intervals(est, ok, rse, [10.0, 0.05, 0.7], se, NAMES, level=0.9)
    assert used == {"coverage": B - 3, "error_rate": B - 2, "q1": 0}
    assert iv["error_rate"] is None and iv["q1"] is None  # the original has none; fewer than two replicates
    take = ok & np.isfinite(rse[:, 0])
    t = (est[take, 0] - 10.0) / rse[take, 0]
    q_lo, q_hi = np.percentile(t, [5.0, 95.0])
    assert iv["coverage"] == [10.0 - q_hi * 0.21, 10.0 - q_lo * 0.21] and iv["coverage"][0] < iv["coverage"][1]
    # exactly two qualify: an interval; one: None
    two = np.zeros(B, dtype=bool)
    two[[0, 1]] = True
    assert t_intervals(est, two, rse, [10.0, 0.05, 0.7], se, NAMES)[0]["coverage"] is not None
    two[1] = False
    assert t_intervals(est, two, rse, [10.0, 0.05, 0.7], se, NAMES) == ({"coverage": None, "error_rate": None, "q1": None},
                                                                         {"coverage": 1, "error_rate": 1, "q1": 0})
    # a replicate standard error of 0 or inf does not qualify; an empty run gives None everywhere
    rse2 = rse.copy()
    rse2[0, 0], rse2[1, 0] = 0.0, math.inf
    assert t_intervals(est, ok, rse2, [10.0, 0.05, 0.7], se, NAMES)[1]["coverage"] == B - 5
    assert t_intervals(np.empty((0, 3)), np.empty(0, dtype=bool), np.empty((0, 3)), [10.0, 0.05, 0.7], se, NAMES)[0]["coverage"] is None
    with pytest.raises(ValueError):
        t_intervals(est, ok, rse, [10.0, 0.05, 0.7], se, NAMES, level=1.0)


HESS = -np.array([[400.0, 30.0, 0.0, 5.0, 1.0], [30.0, 9.0e4, 0.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0], [5.0, 2.0, 0.0, 50.0, 4.0],
                  [1.0, 3.0, 0.0, 4.0, 70.0]])  # of LL; q1's row all zero


class _Stub:
    params = ("coverage", "error_rate", "q1", "q2", "q")
    bounds = ((0.01, None), (0, 0.5), (0.3, 1), (0, 1), (0, 1))
    param_count = 5

    def __init__(self, hess=HESS):
        self.hess = hess
        self.calls = 0

    def loglikelihood_hessian_points(self, points):
        self.calls += 1
        return np.array([-1234.5]), np.array([[0.1, -0.2, 0.0, 0.3, 0.4]]), self.hess[None, :, :]


def test_observed_information_is_what_it_was():
    """The dict of a stubbed model, key for key: q1 not identified (an all-zero row), q on its bound, q2 fixed."""
    from covest_amd import observed_information
    est = [10.0, 0.05, 0.7, 0.4, 1.0]
    info = observed_information(_Stub(), est, fix=[None, None, None, 0.4, None])
    assert list(info) == ['params', 'estimate', 'bounds', 'loglikelihood', 'gradient', 'hessian', 'free', 'covariance',
                          'correlation', 'standard_errors', 'reason']
    assert info['params'] == list(_Stub.params) and info['estimate'] == est and info['bounds'] == [tuple(b) for b in _Stub.bounds]
    assert info['loglikelihood'] == -1234.5 and info['gradient'] == [0.1, -0.2, 0.0, 0.3, 0.4]
    assert info['hessian'] == (-HESS).tolist() and info['free'] == [0, 1] and info['reason'] is None
    A = -HESS[:2, :2]
    chol = np.linalg.cholesky(A)
    inv_chol = np.linalg.solve(chol, np.eye(2))
    cov = inv_chol.T @ inv_chol
    assert info['covariance'] == cov.tolist()
    se = np.sqrt(np.diag(cov))
    assert info['correlation'] == (cov / np.outer(se, se)).tolist()
    assert info['standard_errors'] == {"coverage": float(se[0]), "error_rate": float(se[1]), "q1": None, "q2": None, "q": None}
    assert np.allclose(cov, np.linalg.inv(A), rtol=1e-12)
    # the reasons
    bad = HESS.copy()
    bad[0, 0] = math.nan
    info = observed_information(_Stub(bad), est)
    assert info['reason'] == "the Hessian is not finite at this point" and info['free'] == [] and info['covariance'] is None
    info = observed_information(_Stub(-HESS), [10.0, 0.05, 0.7, 0.4, 0.5])  # negative definite information
    assert "not positive definite" in info['reason'] and info['free'] == [0, 1, 3, 4] and set(info['standard_errors'].values()) == {None}
    info = observed_information(_Stub(), [0.01, 0.0, 0.7, 0.0, 1.0])
    assert info['reason'].startswith("no free parameter") and info['free'] == []
    with pytest.raises(ValueError):
        observed_information(_Stub(), est[:4])
    with pytest.raises(ValueError):
        observed_information(_Stub(), est, fix=[None])


class _StubBatch:
    """A batch of three histograms whose Hessians are HESS scaled by 1, 4 and NaN."""

    def __init__(self):
        self.model = _Stub()
        self.calls = []

    def __len__(self):
        return 3

    def loglikelihood_hessian_pairs(self, index, points):
        self.calls.append((np.asarray(index).tolist(), np.asarray(points).copy()))
        scale = np.array([1.0, 4.0, math.nan])
        return np.array([-1.0, -2.0, -3.0]), np.tile([0.1, -0.2, 0.0, 0.3, 0.4], (3, 1)), scale[:, None, None] * HESS[None]


def test_the_batch_form_is_one_call_and_the_same_rules():
    from covest_amd import observed_information, observed_information_batch
    from covest_amd.bootstrap import _replicate_standard_errors
    batch = _StubBatch()
    est = np.array([[10.0, 0.05, 0.7, 0.4, 0.5], [11.0, 0.04, 0.7, 0.4, 1.0], [9.0, 0.06, 0.7, 0.4, 0.5]])
    infos = observed_information_batch(batch, est)
    assert len(batch.calls) == 1 and batch.calls[0][0] == [0, 1, 2] and np.array_equal(batch.calls[0][1], est)
    assert batch.model.calls == 0  # (no walk of the model's own histogram)
    assert [info['free'] for info in infos] == [[0, 1, 3, 4], [0, 1, 3], []]
    assert infos[2]['reason'] == "the Hessian is not finite at this point"
    one = observed_information(_Stub(), est[0])  # the same Hessian through the one-model form: the same dict but the value
    assert {k: v for k, v in infos[0].items() if k != 'loglikelihood'} == {k: v for k, v in one.items() if k != 'loglikelihood'}
    assert infos[0]['loglikelihood'] == -1.0 and infos[1]['estimate'] == est[1].tolist()
    # four times the information: half the standard error
    assert math.isclose(infos[1]['standard_errors']['coverage'] * 2,
                        observed_information(_Stub(), est[1])['standard_errors']['coverage'], rel_tol=1e-12)
    rse = _replicate_standard_errors(infos, list(_Stub.params))
    assert rse.shape == (3, 5) and np.all(np.isnan(rse[2])) and np.all(np.isnan(rse[:, 2])) and math.isnan(rse[1, 4])
    assert np.all(np.isfinite(rse[0, [0, 1, 3, 4]])) and rse[0, 0] == infos[0]['standard_errors']['coverage']
    fixed = observed_information_batch(batch, est, fix=[None, 0.05, None, None, None])
    assert fixed[0]['free'] == [0, 3, 4]
