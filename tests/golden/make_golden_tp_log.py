#!/usr/bin/env python3
"""tests/golden/tp_log.json: ln TP(l, j) of the reference's truncated-Poisson pmf, at 50 digits (mpmath).

    python tests/golden/make_golden_tp_log.py

The pmf is the one c_src/covest_poissonmodule.c:7-35 computes, restated in the log domain with the REFERENCE's
normaliser, not ln(e^l - 1): 200 is taken off l while l > 200 (in double arithmetic, as there), each time with a
division by e^200; what is left divides as expl(l_res) - 1 (e^l_res rounded to the long double's 64 bits first), or --
the two `<= 1e-8` branches -- as l itself where l <= 1e-8, and as the ORIGINAL l where the residual is <= 1e-8:

    ln TP = ln prod_{i <= j} fl(l / i) - D(l),    D = 200 n + ln(e^l_res - 1)   |   200 n + ln l   |   ln l,

fl(l / i) the quotient rounded to a double as the extension's loop forms it (within 1e-14 of j ln l - ln j! for
j <= 10 000, five orders below the 1e-9 the values are used at).

Evaluated at every (l, j) of tp_table.json, at the edges of tp_bitwise.json with l > 0, and at the rows of
tp_bitwise.json whose reference value is +inf (the log is finite there: what the value mode is held to).  The yardstick
hangs on the reference's own numbers: exp of every value must reproduce the fixtures' finite NORMAL values to 1e-15
relative, asserted here.

Rows whose l lies just above a multiple of 200 -- l / l_res > 1e5, the selection rule of make_golden_hessian.py -- are
left out: there D hangs on the last bits of l_res, e^l_res - 1 formed in x87 long double differs from the exact value by
up to 2^-64 / l_res, and a yardstick that is not the reference's own arithmetic cannot be held to 1e-9.  At most 5 % of
the rows may go that way; checked here.
"""
import json
import math
import os

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
MAX_EXP = 200.0
SKIP_RATIO = 1e5
SKIP_CAP = 0.05
REPRODUCE_REL = 1e-15


def residual(l):
    """(n, l_res): the extension's `while (l > MAX_EXP) l -= MAX_EXP` in double arithmetic (:25-28)."""
    n = 0
    while l > MAX_EXP:
        l -= MAX_EXP
        n += 1
    return n, l


def expl_minus_1(x):
    """expl(x) - 1 as the extension forms it (:30): e^x rounded to the 64-bit significand of the x87 long double
    BEFORE the subtraction -- a relative 2^-64 / x of the difference, 2.7e-12 at x = 2e-8 -- then the exact difference
    (the subtraction itself is exact or rounds at 2^-64 of a number >= 1)."""
    with mp.workprec(64):
        e = +mp.exp(mp.mpf(x))
    return e - 1


def ln_tp(l, j):
    n, res = residual(l)
    if l <= 1e-8 or res <= 1e-8:
        d = 200 * n + mp.log(mp.mpf(l))
    else:
        d = 200 * n + mp.log(expl_minus_1(res))
    return ln_product(l, j) - d


def ln_product(l, j):
    """ln prod_{i <= j} (l / i) with every quotient rounded to a double, as `p1 *= l / i` forms it (:23: l is a double,
    i an int, the quotient a double before it is widened) -- the product itself exact.  Against l^j / j! that is a
    random walk of j roundings of 1.1e-16, 1e-15 at j = 100: without it exp() of these values could not reproduce the
    reference's to 1e-15.  What is left out is the long-double product's own rounding, j 2^-64 at most."""
    p = mp.mpf(1)
    for i in range(1, j + 1):
        p *= mp.mpf(l / i)
    return mp.log(p)


def skipped(l):
    n, res = residual(l)
    return n > 0 and l / res > SKIP_RATIO


def main():
    table = json.load(open(os.path.join(HERE, "tp_table.json")))
    bitwise = json.load(open(os.path.join(HERE, "tp_bitwise.json")))
    cases = [(r, "tp_table") for r in table["rows"]]
    cases += [(r, "tp_bitwise.edges") for r in bitwise["edges"] if r[0] > 0]
    cases += [(r, "tp_bitwise.rows(+inf)") for r in bitwise["rows"] if r[2] == math.inf]
    seen = set()  # (a pair that two of the sources hold is one case, under the first source's name)
    cases = [c for c in cases if (c[0][0], c[0][1]) not in seen and not seen.add((c[0][0], c[0][1]))]
    rows, n_skipped, worst, n_checked = [], 0, 0.0, 0
    tiny = 2.2250738585072014e-308
    for (l, j, ref), src in cases:
        if skipped(l):
            n_skipped += 1
            continue
        v = ln_tp(l, int(j))
        if math.isfinite(ref) and ref >= tiny:  # a finite normal value of the reference: exp must reproduce it
            rel = abs(mp.exp(v) / mp.mpf(ref) - 1)
            worst = max(worst, float(rel))
            n_checked += 1
            assert rel <= REPRODUCE_REL, (l, j, ref, float(rel))
        rows.append([l, int(j), float(v), src])
    print("%d rows, %d skipped (l / l_res > %g), %d finite normal reference values reproduced, worst %.3g relative"
          % (len(rows), n_skipped, SKIP_RATIO, n_checked, worst))
    assert n_skipped <= SKIP_CAP * len(cases), (n_skipped, len(cases))
    out = {"what": "ln of covest_poisson.truncated_poisson(l, j), the reference's normaliser, mpmath at 50 digits; "
                   "rows: [l, j, ln TP, source]",
           "digits": mp.mp.dps, "skip_ratio": SKIP_RATIO, "skipped": n_skipped, "cases": len(cases),
           "reproduces_reference_to": REPRODUCE_REL, "worst_reproduction": worst, "rows": rows}
    with open(os.path.join(HERE, "tp_log.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
