#!/usr/bin/env python3
"""tests/golden/posterior.json: the posterior classes per key (ln p_j, error shares, copy shares, mean copy number) of
the reference's mixture, at 50 digits (mpmath).

    python tests/golden/make_golden_posterior.py

The arithmetic is tests/posterior_reference.py: a_os, b_o, l_s, x_os and T are Python doubles formed by the reference's
own expressions, everything from them on is 50 digits, ln TP is make_golden_tp_log.ln_tp.  The restatement hangs on the
reference: exp(ln p_j) must reproduce the CPU oracle's compute_probabilities (oracle/covest_oracle.py, pinned by the
reference's golden vectors) to 1e-12 relative wherever that value is a normal double -- asserted here.  T is checked
against threshold_o.json where the point is there.

A candidate case is left out where some component rate falls under make_golden_tp_log.py's own rule (x > 200 with
x / x_res > 1e5: there the yardstick is not the reference's arithmetic); at most 5 % of the candidates may go that way,
asserted here.  A model's keys are the keys the case is evaluated at (12 at most): T hangs on the largest.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
import posterior_reference as ref  # noqa: E402

SKIP_CAP = 0.05
ORACLE_REL = 1e-12


def case(name, kind, k, r, max_error, keys, point, copy_columns=3, threshold=1e-8):
    return {"name": name, "kind": kind, "k": k, "r": r, "max_error": max_error, "keys": keys, "eval_keys": keys,
            "threshold": threshold, "point": list(point), "copy_columns": copy_columns}


def candidates():
    c = [
        case("basic_s8", "basic", 21, 100, 8, [1, 2, 3, 4, 5, 7, 10, 15, 20, 30, 50, 100], (10.0, 0.05)),
        case("basic_s1", "basic", 21, 100, 1, [1, 2, 3, 10], (5.0, 0.01)),
        case("basic_s2", "basic", 21, 100, 2, [1, 2, 3, 10, 40], (20.0, 0.1)),
        case("basic_s22", "basic", 21, 100, 22, [1, 2, 3, 7, 150], (30.0, 0.1)),
        case("basic_k32_s33", "basic", 32, 150, 33, [1, 2, 5, 30, 90], (25.0, 0.03)),
        case("basic_k63_s64", "basic", 63, 150, 64, [1, 2, 5, 30], (40.0, 0.02)),
        case("basic_e0", "basic", 21, 100, 8, [1, 2, 8, 20], (10.0, 0.0)),
        case("basic_e_half", "basic", 21, 100, 8, [1, 2, 8, 20], (10.0, 0.5)),
        case("basic_high_cov", "basic", 21, 100, 1, [1, 2, 1000, 4000], (4000.0, 0.05)),
        case("basic_low_cov", "basic", 21, 100, 8, [1, 3, 150, 10000], (0.5, 0.05)),
        case("rep_q1_one", "repeats", 21, 100, 8, [1, 2, 5, 9], (10.0, 0.05, 1.0, 0.5, 0.5)),
        case("rep_t3", "repeats", 21, 100, 8, [1, 2, 3], (10.0, 0.05, 0.6, 0.5, 0.3)),
        case("rep_t9", "repeats", 21, 100, 8, [1, 2, 4, 9], (10.0, 0.05, 0.6, 0.5, 0.3)),
        case("rep_t10", "repeats", 21, 100, 8, [1, 3, 10], (10.0, 0.05, 0.6, 0.5, 0.3)),
        case("rep_t400", "repeats", 21, 100, 2, [1, 2, 5, 50, 200, 400], (3.0, 0.02, 0.35, 0.5, 0.02)),
        case("rep_q2_zero", "repeats", 21, 100, 8, [1, 2, 6, 12], (10.0, 0.05, 0.5, 0.0, 0.3)),
        case("rep_q2_one", "repeats", 21, 100, 8, [1, 2, 6, 12], (10.0, 0.05, 0.5, 1.0, 0.3)),
        case("rep_q_zero", "repeats", 21, 100, 8, [1, 2, 6, 12], (10.0, 0.05, 0.5, 0.5, 0.0)),
        case("rep_q_one", "repeats", 21, 100, 8, [1, 2, 6, 12], (10.0, 0.05, 0.5, 0.5, 1.0)),
        case("rep_threshold_row", "repeats", 21, 100, 8, [1, 2, 8, 15], (10.0, 0.05, 0.3, 0.25, 0.001)),
        case("rep_s22_t5", "repeats", 21, 100, 22, [1, 2, 3, 5], (8.0, 0.08, 0.5, 0.4, 0.3)),
        case("rep_high_cov", "repeats", 21, 100, 1, [1, 10], (4000.0, 0.05, 0.5, 0.5, 0.3)),
    ]
    # the same cases at a wider copy_columns (T + 5 and T - 1): the lumped column against the sum of the wide call's
    wide = []
    for base, columns in (("rep_t9", 14), ("rep_t9", 8), ("rep_t400", 405), ("rep_threshold_row", 20)):
        b = dict(next(x for x in c if x["name"] == base))
        b["name"], b["wide_of"], b["copy_columns"] = "%s_cc%d" % (base, columns), base, columns
        wide.append(b)
    return c + wide


def check_against_oracle(oracle, cs, rows):
    hist = {int(j): 1 for j in cs["keys"]}
    m = oracle.OracleModel(cs["kind"], cs["k"], cs["r"], hist, 0, max_error=cs["max_error"], threshold=cs["threshold"])
    want = m.compute_probabilities(*cs["point"])
    worst = 0.0
    for j in cs["eval_keys"]:
        p = want[j]
        if math.isfinite(p) and p >= ref.TINY:
            rel = abs(math.exp(rows[str(j)]["ln_p"]) / p - 1)
            worst = max(worst, rel)
            assert rel <= ORACLE_REL, (cs["name"], j, p, rel)
    return worst


def main():
    from oracle import covest_oracle
    covest_oracle.build()
    thresholds = {tuple(r[:4]): r[4] for r in json.load(open(os.path.join(HERE, "threshold_o.json")))["rows"]}
    cands = candidates()
    cases, n_skipped, worst, n_pinned = [], 0, 0.0, 0
    for cs in cands:
        T, x, a, b = ref.mixture_doubles(cs["kind"], cs["k"], cs["r"], cs["max_error"], cs["point"], cs["threshold"],
                                         max(cs["keys"]))
        if ref.any_rate_skipped(x):
            n_skipped += 1
            print("left out:", cs["name"])
            continue
        if cs["kind"] == "repeats":
            row = (max(cs["keys"]),) + tuple(cs["point"][2:5])
            if row in thresholds:
                assert thresholds[row] == T, (cs["name"], thresholds[row], T)
                n_pinned += 1
        got, _ = ref.compute_case(cs)
        assert got["T"] == T
        worst = max(worst, check_against_oracle(covest_oracle, cs, got["rows"]))
        cs = dict(cs)
        cs.update(got)
        cases.append(cs)
        print("%-24s T = %-4d %d keys" % (cs["name"], T, len(cs["eval_keys"])), flush=True)
    assert n_skipped <= SKIP_CAP * len(cands), (n_skipped, len(cands))
    assert n_pinned >= 1
    print("%d cases of %d candidates, %d left out; exp(ln p) against the oracle: worst %.3g relative; %d T pinned by "
          "threshold_o.json" % (len(cases), len(cands), n_skipped, worst, n_pinned))
    out = {"what": "posterior classes per key of the reference's mixture: ln p_j, error shares E[s], copy shares "
                   "C[column] (column c < copy_columns - 1: o = c + 1; the last: o >= copy_columns), mean copy number "
                   "M, and L = max |ln w_os(j)| over the components of finite weight; mpmath at 50 digits over the "
                   "reference's doubles (tests/posterior_reference.py)",
           "digits": 50, "candidates": len(cands), "skipped": n_skipped, "skip_cap": SKIP_CAP,
           "reproduces_oracle_to": ORACLE_REL, "worst_reproduction": worst, "cases": cases}
    with open(os.path.join(HERE, "posterior.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
