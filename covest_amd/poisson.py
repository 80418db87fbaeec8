"""The truncated-Poisson pmf on the device: the counterpart of the reference's importable C extension,

    from covest_poisson import truncated_poisson          # c_src/covest_poissonmodule.c:7-35

which every likelihood this package computes is a mixture of.  Two routes, the two the
likelihood kernels take: term by term (K-direct's arithmetic; `truncated_poisson`, `truncated_poisson_many`) and the
one-multiply-a-key recurrence of the fast kernels (`truncated_poisson_table`).  There is no CPU path: without the
library or a HIP device every call raises CovestHipError.
"""
import ctypes

import numpy as np

from . import _capi

MODES = {"value": 0, "reference": 1, "log": 2}  # include/covest_amd.h COVEST_TP_*


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _keys(j):
    a = np.asarray(j)
    if a.dtype.kind not in "iu":
        f = np.asarray(a, dtype=np.float64)
        if not np.all(f == np.floor(f)):
            raise ValueError("j must be integers")
    return a.astype(np.int64)


def truncated_poisson_many(l, j, mode="value", device=-1):
    """TP(l[i], j[i]) for arrays of equal length (a scalar on either side is repeated), as a float64 array.

    mode "value": the finite value the formula defines -- 0 where it lies below the doubles' range, never inf, 0.0 at
    l == 0 and at NaN; "reference": what the extension returns, +inf included where its long-double product overflows;
    "log": ln of the value before the last exp, finite wherever l > 0, -inf at l == 0.  j >= 1."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % ", ".join(sorted(MODES)))
    rates, keys = np.broadcast_arrays(np.asarray(l, dtype=np.float64), _keys(j))
    shape = rates.shape
    rates, keys = np.ascontiguousarray(rates).ravel(), np.ascontiguousarray(keys).ravel()
    out = np.empty(rates.size, dtype=np.float64)
    _capi.check(_capi.lib().covest_truncated_poisson(int(device), rates.size, _dp(rates), _ip(keys), MODES[mode], _dp(out)),
                "covest_truncated_poisson")
    return out.reshape(shape)


def truncated_poisson(l, j, device=-1):
    """Drop-in for covest_poisson.truncated_poisson(l, j): one value, as the extension returns it (reference mode:
    +inf where its running long-double product overflows).  j >= 1 (the likelihood asks for no other key)."""
    return float(truncated_poisson_many([float(l)], [int(j)], "reference", device)[0])


def truncated_poisson_table(l, keys, device=-1):
    """table[i, b] = TP(l[i], keys[b]) in "value" mode, by the recurrence the fast likelihood kernels walk.
    keys: strictly ascending integers in 1..16384."""
    rates = np.ascontiguousarray(np.asarray(l, dtype=np.float64)).ravel()
    ks = np.ascontiguousarray(_keys(keys)).ravel()
    out = np.empty((rates.size, ks.size), dtype=np.float64)
    _capi.check(_capi.lib().covest_truncated_poisson_table(int(device), rates.size, _dp(rates), ks.size, _ip(ks), _dp(out)),
                "covest_truncated_poisson_table")
    return out
