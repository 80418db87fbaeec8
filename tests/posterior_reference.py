"""The yardstick of the posterior classes (tests/golden/posterior.json, tests/test_posterior_cpu.py,
tests/test_gpu_posterior.py): test infrastructure, not collected.

The mixture of covest/models.py:81-98 (basic) and :211-242 (repeats) taken apart before its terms are added:

    ln w_os(j) = ln b_o + ln a_os + ln TP(x_os, j),   x_os = o * l_s
    ln p_j = logsumexp over (o, s);  E_s(j) = sum_o w_os / p_j;  C_o(j) = sum_s w_os / p_j;  M(j) = sum_o o C_o(j)

a_os, b_o, l_s, x_os and T = threshold_o are PYTHON DOUBLES, computed by the reference's own expressions restated here
(the same operations in the same order: `1.0 - exp(-x)`, the naive sums, fix_zero); everything from those doubles on is
mpmath at 50 digits, ln TP by make_golden_tp_log.ln_tp -- the reference's normaliser, imported, not copied.
"""
import math
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_tp_log import ln_tp, skipped  # noqa: E402

mp.mp.dps = 50
EPS = 2.0 ** -52
TINY = 2.2250738585072014e-308  # the smallest normal double
DENORM_MIN = 4.94e-324


def comb_table(k):
    """self.comb of covest/models.py:25 (scipy.misc.comb then, scipy.special.comb now: the same float routine)."""
    from scipy.special import comb
    return [comb(k, s) * (3 ** s) for s in range(k + 1)]


def b_o_function(q1, q2, q):
    """RepeatsModel.get_b_o, covest/models.py:193-208."""
    o_2 = (1 - q1) * q2
    o_n = (1 - q1) * (1 - q2) * q

    def b_o(o):
        if o == 0:
            return 0
        elif o == 1:
            return q1
        elif o == 2:
            return o_2
        else:
            return o_n * (1 - q) ** (o - 3)
    return b_o


def threshold_o(b_o, threshold, hist_max):
    """RepeatsModel.get_hist_threshold, covest/models.py:185-191."""
    if threshold is not None:
        for o in range(1, hist_max):
            if b_o(o) <= threshold:
                return o
    return hist_max


def mixture_doubles(kind, k, r, max_error, point, threshold, hist_max):
    """(T, x[o][s], a[o][s], b[o]) for o = 1 .. T - 1 (index 0 unused), as the reference forms them in double."""
    S = min(k + 1, max_error)
    comb = comb_table(k)
    c, err = point[0], point[1]
    ck = c * (r - k + 1) / r                                                  # correct_c        models.py:71-72
    l_s = [ck * (3 ** -s) * (1.0 - err) ** (k - s) * err ** s for s in range(S)]  # _get_lambda_s  models.py:76-79
    if kind == "basic":
        T, b = 2, [None, 1.0]
    else:
        b_o = b_o_function(*point[2:5])
        T = threshold_o(b_o, threshold, hist_max)
        b = [None] + [float(b_o(o)) for o in range(1, T)]
    x, a = [None], [None]
    for o in range(1, T):
        # models.py:87 (basic: exp(-l_s[s])) and :221 (repeats: exp(o * -l_s[s])); o = 1 gives the same double
        n = [comb[s] * (1.0 - math.exp(o * -l_s[s])) for s in range(S)]
        tot = 0.0
        for t in range(S):  # the builtin sum of the reference's interpreter: naive, left to right  models.py:88,225
            tot += n[t]
        if tot == 0:
            tot = 1         # fix_zero
        a.append([n[s] / tot for s in range(S)])
        x.append([o * l_s[s] for s in range(S)])
    return T, x, a, b


def any_rate_skipped(x):
    """make_golden_tp_log's own rule on some component rate: x > 200 with x / x_res > 1e5."""
    return any(skipped(v) for row in x[1:] for v in row if v > 0)


def classes_at_key(j, T, x, a, b, copy_columns):
    """At key j: (ln p, E[S], C[copy_columns], M, L) -- mpmath numbers but L, the largest |ln w_os(j)| over the
    components of finite weight, a double.  ln p = -inf, NaN shares and mean where no component has weight."""
    S = len(a[1]) if T > 1 else 0
    lw = {}
    for o in range(1, T):
        for s in range(S):
            if a[o][s] * b[o] == 0 or not x[o][s] > 0:
                continue
            lw[(o, s)] = mp.log(mp.mpf(b[o])) + mp.log(mp.mpf(a[o][s])) + ln_tp(x[o][s], j)
    S = S or 1
    if not lw:
        nan = mp.mpf("nan")
        return mp.mpf("-inf"), [nan] * S, [nan] * copy_columns, nan, 0.0
    top = max(lw.values())
    w = {key: mp.exp(v - top) for key, v in lw.items()}
    total = mp.fsum(w.values())
    E = [mp.fsum(v for (o, s), v in w.items() if s == t) / total for t in range(S)]
    by_o = {o: mp.fsum(v for (oo, s), v in w.items() if oo == o) / total for o in range(1, T)}
    C = [mp.mpf(0)] * copy_columns
    for o, v in by_o.items():
        C[min(o, copy_columns) - 1] += v
    M = mp.fsum(o * v for o, v in by_o.items())
    L = max(abs(float(v)) for v in lw.values())
    return top + mp.log(total), E, C, M, L


def compute_case(case):
    """A case {kind, k, r, max_error, keys, threshold, point, copy_columns} -> its golden entries, doubles."""
    T, x, a, b = mixture_doubles(case["kind"], case["k"], case["r"], case["max_error"], case["point"],
                                 case["threshold"], max(case["keys"]))
    out = {"T": T, "rows": {}}
    for j in case["eval_keys"]:
        ln_p, E, C, M, L = classes_at_key(j, T, x, a, b, case["copy_columns"])
        out["rows"][str(j)] = {"ln_p": float(ln_p), "E": [float(v) for v in E], "C": [float(v) for v in C],
                               "M": float(M), "L": L}
    return out, (T, x, a, b)


def delta(L):
    """The project's bar on a log pmf (tests/test_gpu_tp.py): 1e-9, plus 4 eps of the magnitude."""
    return 1e-9 + 4 * EPS * L


def share_bound(want, L):
    """On a share or the mean: a softmax share moves by at most 2 delta relative when every ln w moves by delta."""
    return 2 * delta(L) * abs(want) + DENORM_MIN
