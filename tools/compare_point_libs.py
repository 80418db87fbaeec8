"""Two builds of the library side by side on the point-list entry points (covest_eval_points, covest_eval_points_grad,
covest_eval_points_hess): what a change did to the numbers.

For each library, in a child process of its own (COVEST_AMD_LIB is read at import): loglikelihood_gradient_points and
loglikelihood_hessian_points at every point of tests/golden/gradient.json and tests/golden/hessian.json, and at the four
set-ups and the batches of 1, 20 and 300 points of the tests' "company" cases; and loglikelihood_points on value_sets(),
which are chosen to reach every route of covest_eval_points -- each set says which (its launch record, the list modes
of its plans, the kinds of threshold_o in it), the child checks that against launch_record() and covest_threshold_o,
and the comparison fails if a set missed its route or the two libraries launched differently.  The arrays are dumped
as .npy and compared.  Reads tests/golden/ and the two libraries, nothing else.

    python tools/compare_point_libs.py --new covest_amd/lib/libcovest_amd.so --parent /path/lib_parent.so \
        [--work DIR] [--out profiles/points_ab.txt]
    python tools/compare_point_libs.py --rehearse      # no device: the sets' threshold_o kinds against what they claim
"""
import argparse
import itertools
import json
import math
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
COMPANY = [("repeats", "H10k_rep_trim", 11192), ("basic", "H10k_basic_trim", 163), ("repeats", "sim_c10_e0.05", 0),
           ("repeats", "H10k_rep", 0)]


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def sets():
    """(name, case, points) of every evaluation; the fixtures' cases carry their condition sums."""
    out = []
    for fixture in ("gradient.json", "hessian.json"):
        for ci, case in enumerate(golden(fixture)["cases"]):
            out.append(("%s_%d" % (fixture.split(".")[0], ci), case, np.array(case["points"], dtype=np.float64)))
    for ci, (kind, hist, tail) in enumerate(COMPANY):  # as tests/test_gpu_gradient.py, tests/test_gpu_hessian.py
        rng = np.random.default_rng(5)
        case = {"model": kind, "hist": hist, "k": 21, "r": 100, "tail": tail, "max_error": 8}
        if kind == "repeats":
            c0 = 24.0 if hist.startswith("H10k") else 10.0
            point = [c0, 0.02, 0.6, 0.5, 0.2]
            others = np.column_stack([rng.uniform(0.5 * c0, 1.5 * c0, 300), rng.uniform(0.005, 0.1, 300), rng.uniform(0.3, 1, 300),
                                      rng.uniform(0, 1, 300), rng.uniform(0.15, 1, 300)])
        else:
            point = [4000.0, 0.02]
            others = np.column_stack([rng.uniform(3000, 5000, 300), rng.uniform(0.005, 0.05, 300)])
        out.append(("company_%d_1" % ci, case, np.array([point])))
        for n, at in ((20, 7), (300, 150)):
            batch = others[:n].copy()
            batch[at] = point
            out.append(("company_%d_%d" % (ci, n), case, batch))
    return out


# ---- the value sets: (name, case, points, kernel, want); want = the route the set is there for:
#   "only": the exact set of launches | "launch": prefixes of launches that must be there
#   "modes": the list modes of its K-factored plans, exactly | "kinds": the kinds of threshold_o in it, exactly
#   (fits: threshold_o - 1 in 1..512, big: beyond, one: threshold_o == 1)
SUB_HIST = {1: 1000, 2: 500, 150: 6000, 151: 40, 153: 7}  # tests/test_gpu_variants.py: a key with a subnormal p_j
LIST_HIST = {**{j: max(1, int(20000 * math.exp(-0.07 * i))) for i, j in enumerate(range(1, 61))}, 700: 3}


def _list_points(seed, n, c_hi):  # tests/test_gpu_variants.py
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0.5, c_hi, n), rng.uniform(0.005, 0.15, n), rng.uniform(0.3, 1.0, n),
                            rng.uniform(0.0, 1.0, n), np.concatenate([rng.uniform(0.006, 0.02, n // 2),
                                                                      rng.uniform(0.1, 0.95, n - n // 2)])])


def _product(axes):
    return np.array(list(itertools.product(*axes)), dtype=np.float64)


def value_sets():
    out = []
    rng = np.random.default_rng(11)
    basic = {"model": "basic", "hist": "H10k_basic", "k": 21, "r": 100, "tail": 0, "max_error": 8}
    pts = np.column_stack([rng.uniform(3000, 5000, 5000), rng.uniform(0.005, 0.05, 5000)])
    for kernel in ("auto", "recur", "direct"):  # both sides of the in-place limit (256 points)
        for n in (1, 6, 256, 257, 5000):
            want = {"only": ["ll_direct"]} if kernel == "direct" else {"launch": ["ll_basic<", "fix_"]}
            out.append(("basic_%s_%d" % (kernel, n), basic, pts[:n], kernel, want))
    grid = _product([np.linspace(0.50, 0.85, 141), [0.01, 0.02]])
    for tail in (0, 9):  # K-basic hands points back, the fix pass patches values: in place (141 points) and not (282)
        case = {"model": "basic", "hist": SUB_HIST, "k": 21, "r": 100, "tail": tail, "max_error": 8}
        for n, sel in ((141, grid[::2]), (282, grid)):
            out.append(("sub_hist_basic_t%d_%d" % (tail, n), case, sel, "recur", {"launch": ["ll_basic<8", "fix_basic_packed<8>"]}))
    rep = {"model": "repeats", "hist": "H10k_rep", "k": 21, "r": 100, "tail": 0, "max_error": 8}
    pts = np.column_stack([rng.uniform(12, 36, 5000), rng.uniform(0.005, 0.1, 5000), rng.uniform(0.3, 1, 5000),
                           rng.uniform(0, 1, 5000), rng.uniform(0.15, 1, 5000)])
    for n in (1, 4, 5, 64, 300):  # list mode, both sides of the tables' in-place limit (4 points)
        out.append(("repeats_list_%d" % n, rep, pts[:n], "auto", {"launch": ["ll_factored<"], "modes": [1]}))
    out.append(("repeats_auto_5000", rep, pts, "auto", {"only": ["ll_direct"]}))
    for tail in (0, 4):  # one call with all three kinds of point, then each kind alone
        case = {"model": "repeats", "hist": LIST_HIST, "k": 21, "r": 100, "tail": tail, "max_error": 8, "min_single_copy_ratio": 0.0}
        mixed = _list_points(17 + tail, 40, 40.0)
        mixed[3::7, 2] = 0.0  # q1 = 0: threshold_o == 1
        kinds = route_kinds(case, mixed)
        out.append(("mixed_t%d" % tail, case, mixed, "factored",
                    {"launch": ["ll_factored<512", "ll_finish_partials", "ll_direct"], "modes": [1, 2], "kinds": ["big", "fits", "one"]}))
        for kind, launch, modes in (("fits", ["ll_factored<"], [1]), ("big", ["ll_factored<512", "ll_finish_partials"], [2]),
                                    ("one", None, [])):
            want = {"modes": modes, "kinds": [kind]}
            want.update({"only": ["ll_direct"]} if launch is None else {"launch": launch})
            out.append(("%s_alone_t%d" % (kind, tail), case, mixed[kinds == kind], "factored", want))
    grid = _product([np.exp(np.linspace(np.log(0.03), np.log(0.8), 60)), [0.01], [0.7, 0.9], [0.5], [0.6, 0.95, 1.0]])
    for tail in (0, 9):
        # list mode 1 hands keys back and the host's strict pass (fix_list) patches them; more than 8 error classes: K-direct
        case = {"model": "repeats", "hist": SUB_HIST, "k": 21, "r": 100, "tail": tail, "max_error": 8}
        out.append(("sub_hist_repeats_t%d" % tail, case, grid, "auto", {"launch": ["ll_factored<", "fix_list<"], "modes": [1], "kinds": ["fits"]}))
        out.append(("repeats_s16_t%d" % tail, dict(case, max_error=16), grid, "auto", {"only": ["ll_direct"]}))
    return out


def make_model(case):
    from bench import load_hist
    from covest_amd import BasicModel, RepeatsModel
    hist = case["hist"] if isinstance(case["hist"], dict) else load_hist(case["hist"])
    if case["model"] == "repeats":
        return RepeatsModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"],
                            threshold=case.get("threshold", 1e-8), min_single_copy_ratio=case.get("min_single_copy_ratio", 0.3))
    return BasicModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"], max_cov=case.get("max_cov"))


def route_kinds(case, points):
    """fits / big / one per point of a repeats-model list, as covest_eval_points sorts them: by covest_threshold_o of the
    clamped (q1, q2, q).  Host arithmetic of the library, no device."""
    m = make_model(case)
    q = np.array([m.fit_to_bounds(p)[2:5] for p in points], dtype=np.float64)
    t = m.get_hist_threshold_values(q)
    return np.where(t - 1 < 1, "one", np.where(t - 1 <= 512, "fits", "big"))


def route_misses(want, kinds, rec):
    """What of `want` a set did not do (rec None: the rehearsal, kinds only)."""
    miss = []
    if "kinds" in want and sorted(set(kinds)) != want["kinds"]:
        miss.append("kinds %s, wanted %s" % (sorted(set(kinds)), want["kinds"]))
    if rec is not None:
        names = list(rec["launches"])
        if "only" in want and sorted(names) != want["only"]:
            miss.append("launches %s, wanted only %s" % (names, want["only"]))
        miss += ["no launch of %s* among %s" % (p, names) for p in want.get("launch", []) if not any(n.startswith(p) for n in names)]
        modes = sorted({p["list_mode"] for p in rec["plans"]})
        if "modes" in want and modes != want["modes"]:
            miss.append("list modes %s, wanted %s" % (modes, want["modes"]))
    return miss


def rehearse():
    bad = 0
    for name, case, points, kernel, want in value_sets():
        kinds = route_kinds(case, points) if case["model"] == "repeats" else np.array([], dtype=str)
        miss = route_misses(want, kinds, None) + ([] if len(points) else ["empty"])
        bad += len(miss)
        print("%-24s n=%4d %-8s %s %s" % (name, len(points), kernel, dict(zip(*np.unique(kinds, return_counts=True))), miss or "ok"))
    return 1 if bad else 0


def dump(work):
    routes = {}
    for name, case, points, kernel, want in value_sets():
        m = make_model(case)
        np.save(os.path.join(work, "%s.v_ll.npy" % name), m.loglikelihood_points(points, kernel=kernel))
        rec = m.launch_record()
        kinds = route_kinds(case, points) if case["model"] == "repeats" else np.array([], dtype=str)
        routes[name] = {"launches": list(rec["launches"].items()), "modes": [p["list_mode"] for p in rec["plans"]],
                        "kinds": {str(k): int(c) for k, c in zip(*np.unique(kinds, return_counts=True))},
                        "missed": route_misses(want, kinds, rec) + ([] if len(points) else ["empty"])}
        m.close()
        print("done: %s" % name, file=sys.stderr, flush=True)  # (progress, for a caller that watches the run)
    with open(os.path.join(work, "routes.json"), "w") as f:
        json.dump(routes, f)
    for name, case, points in sets():
        m = make_model(case)
        g_ll, g_grad = m.loglikelihood_gradient_points(points)
        h_ll, h_grad, h_hess = m.loglikelihood_hessian_points(points)
        for what, arr in (("g_ll", g_ll), ("g_grad", g_grad), ("h_ll", h_ll), ("h_grad", h_grad), ("h_hess", h_hess)):
            np.save(os.path.join(work, "%s.%s.npy" % (name, what)), np.asarray(arr, dtype=np.float64))
        m.close()
        print("done: %s" % name, file=sys.stderr, flush=True)


class Exact:
    """Elements compared, elements that differ as numbers or in where NaN sits, elements that differ only in a zero's sign."""

    def __init__(self, title):
        self.title, self.n, self.differ, self.zero_sign, self.listed = title, 0, 0, 0, []

    def add(self, name, a, b):
        a, b = a.ravel(), b.ravel()
        assert a.shape == b.shape, name
        self.n += a.size
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        zs = (a == b) & (np.signbit(a) != np.signbit(b))
        self.differ += int(bad.sum())
        self.zero_sign += int(zs.sum())
        for i in np.flatnonzero(bad | zs):
            self.listed.append("    %s[%d]: %r (%s) against %r (%s), %s" % (
                name, i, float(a[i]), a[i].tobytes().hex(), float(b[i]), b[i].tobytes().hex(),
                "sign of zero" if zs[i] else "%g ulp" % (abs(a[i] - b[i]) / np.spacing(max(abs(a[i]), abs(b[i]))))))

    def lines(self):
        return ["%s: %d elements compared, %d differ, %d differ only in the sign of a zero" % (self.title, self.n, self.differ,
                                                                                             self.zero_sign)] + self.listed[:60]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="(child) evaluate with the library COVEST_AMD_LIB selects and dump the arrays here")
    ap.add_argument("--new")
    ap.add_argument("--parent")
    ap.add_argument("--work")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "points_ab.txt"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse()
    if args.dump:
        dump(args.dump)
        return 0
    work = args.work or tempfile.mkdtemp(prefix="points_ab_")
    for tag, lib in (("new", args.new), ("parent", args.parent)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", os.path.join(work, tag)], env=env, timeout=900).returncode
        if rc != 0:  # nothing more is started after a child that failed
            print("the %s library's run ended with status %d" % (tag, rc))
            return 1

    def load(tag, name, what):
        return np.load(os.path.join(work, tag, "%s.%s.npy" % (name, what)))

    grad_same = Exact("K-grad value and gradient, new against parent")
    hval_same = Exact("K-hess value, new against parent")
    hrest_same = Exact("K-hess gradient and Hessian, new against parent")
    own_same = Exact("K-hess gradient against K-grad gradient, both of the new library")
    own_parent = Exact("(for comparison) K-hess gradient against K-grad gradient, both of the parent library")
    worst_g, worst_h, worst_g_rel, worst_h_rel = (0.0, ""), (0.0, ""), 0.0, 0.0
    n_g = n_h = n_g_diff = n_h_diff = 0
    for name, case, points in sets():
        grad_same.add(name + ".ll", load("new", name, "g_ll"), load("parent", name, "g_ll"))
        grad_same.add(name + ".grad", load("new", name, "g_grad"), load("parent", name, "g_grad"))
        hval_same.add(name + ".ll", load("new", name, "h_ll"), load("parent", name, "h_ll"))
        hrest_same.add(name + ".grad", load("new", name, "h_grad"), load("parent", name, "h_grad"))
        hrest_same.add(name + ".hess", load("new", name, "h_hess"), load("parent", name, "h_hess"))
        own_same.add(name + ".grad", load("new", name, "h_grad"), load("new", name, "g_grad"))
        own_parent.add(name + ".grad", load("parent", name, "h_grad"), load("parent", name, "g_grad"))
        dg = np.abs(load("new", name, "h_grad") - load("parent", name, "h_grad"))
        dh = np.abs(load("new", name, "h_hess") - load("parent", name, "h_hess"))
        n_g, n_h = n_g + dg.size, n_h + dh.size
        n_g_diff, n_h_diff = n_g_diff + int((dg > 0).sum()), n_h_diff + int((dh > 0).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_g_rel = max(worst_g_rel, float(np.nanmax(np.where(dg > 0, dg / np.abs(load("parent", name, "h_grad")), 0.0))))
            worst_h_rel = max(worst_h_rel, float(np.nanmax(np.where(dh > 0, dh / np.abs(load("parent", name, "h_hess")), 0.0))))
        # the fixtures' own condition sums: gradient.json has C (gradient), hessian.json Cg (gradient) and C (Hessian)
        Cg = case.get("Cg") if name.startswith("hessian") else case.get("C")
        if Cg is not None:
            Cg = np.array(Cg, dtype=np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = float(np.nanmax(np.where((Cg > 0) & (dg > 0), dg / Cg, 0.0)))
            worst_g = max(worst_g, (r, name))
        if name.startswith("hessian"):
            C = np.array(case["C"], dtype=np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = float(np.nanmax(np.where((C > 0) & (dh > 0), dh / C, 0.0)))
            worst_h = max(worst_h, (r, name))
    # the value sets: every array bit for bit, every set on its route, the same launches from both libraries
    value_same = Exact("covest_eval_points, new against parent")
    routes = {}
    for tag in ("new", "parent"):
        with open(os.path.join(work, tag, "routes.json")) as f:
            routes[tag] = json.load(f)
    route_lines, off_route = [], 0
    for name, case, points, kernel, want in value_sets():
        value_same.add(name, load("new", name, "v_ll"), load("parent", name, "v_ll"))
        r, rp = routes["new"][name], routes["parent"][name]
        missed = list(r["missed"])
        if (r["launches"], r["modes"]) != (rp["launches"], rp["modes"]):
            missed.append("the parent launched %s, modes %s" % (rp["launches"], rp["modes"]))
        off_route += len(missed)
        route_lines.append("  %-24s n=%4d %-8s %s modes %s kinds %s: %s" % (
            name, len(points), kernel, " ".join("%s x%d" % (n, c) for n, c in r["launches"]), r["modes"], r["kinds"],
            "; ".join(missed) if missed else "on its route, as the parent"))
    lines = ["# the point-list entry points, new library against the parent's (tools/compare_point_libs.py)"]
    lines += value_same.lines() + ["routes of the value sets (launch record of the new library, threshold_o kinds): %d missed" % off_route]
    lines += route_lines
    for e in (grad_same, hval_same, hrest_same):
        lines += e.lines()
    lines += ["K-hess gradient, new against parent: %d of %d elements differ; largest |new - parent| / C_k %.3g (%s); largest "
              "|new - parent| / |parent| %.3g" % (n_g_diff, n_g, worst_g[0], worst_g[1], worst_g_rel),
              "K-hess Hessian, new against parent: %d of %d elements differ; largest |new - parent| / C_kl %.3g (%s); largest "
              "|new - parent| / |parent| %.3g" % (n_h_diff, n_h, worst_h[0], worst_h[1], worst_h_rel)]
    lines += own_same.lines() + own_parent.lines()[:1]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    same = (value_same, grad_same, hval_same, hrest_same)
    return 1 if off_route or any(e.differ or e.zero_sign for e in same) else 0


if __name__ == "__main__":
    sys.exit(main())
