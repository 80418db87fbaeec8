"""Two builds of the library side by side on the derivative entry points (covest_eval_points_grad, covest_eval_points_hess;
ll_deriv.hip): what a change of the kernels did to the numbers.

For each library, in a child process of its own (COVEST_AMD_LIB is read at import), loglikelihood_gradient_points and
loglikelihood_hessian_points at every point of tests/golden/gradient.json and tests/golden/hessian.json, and at the four
set-ups and the batches of 1, 20 and 300 points of the tests' "company" cases; the arrays are dumped as .npy and compared.
Reads tests/golden/ and the two libraries, nothing else.

    python tools/compare_deriv_libs.py --new covest_amd/lib/libcovest_amd.so --parent /path/lib_parent.so \
        [--work DIR] [--out profiles/deriv_ab.txt]
"""
import argparse
import json
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


def dump(work):
    from bench import load_hist
    from covest_amd import BasicModel, RepeatsModel
    for name, case, points in sets():
        hist = load_hist(case["hist"])
        if case["model"] == "repeats":
            m = RepeatsModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"],
                             threshold=case.get("threshold", 1e-8), min_single_copy_ratio=case.get("min_single_copy_ratio", 0.3))
        else:
            m = BasicModel(case["k"], case["r"], hist, case["tail"], max_error=case["max_error"], max_cov=case.get("max_cov"))
        g_ll, g_grad = m.loglikelihood_gradient_points(points)
        h_ll, h_grad, h_hess = m.loglikelihood_hessian_points(points)
        for what, arr in (("g_ll", g_ll), ("g_grad", g_grad), ("h_ll", h_ll), ("h_grad", h_grad), ("h_hess", h_hess)):
            np.save(os.path.join(work, "%s.%s.npy" % (name, what)), np.asarray(arr, dtype=np.float64))
        m.close()


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deriv_ab.txt"))
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
        return 0
    work = args.work or tempfile.mkdtemp(prefix="deriv_ab_")
    for tag, lib in (("new", args.new), ("parent", args.parent)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", os.path.join(work, tag)], env=env, timeout=600).returncode
        if rc != 0:  # nothing more is started after a child that failed
            print("the %s library's run ended with status %d" % (tag, rc))
            return 1

    def load(tag, name, what):
        return np.load(os.path.join(work, tag, "%s.%s.npy" % (name, what)))

    grad_same = Exact("K-grad value and gradient, new against parent")
    hval_same = Exact("K-hess value, new against parent")
    own_same = Exact("K-hess gradient against K-grad gradient, both of the new library")
    own_parent = Exact("(for comparison) K-hess gradient against K-grad gradient, both of the parent library")
    worst_g, worst_h, worst_g_rel, worst_h_rel = (0.0, ""), (0.0, ""), 0.0, 0.0
    n_g = n_h = n_g_diff = n_h_diff = 0
    for name, case, points in sets():
        grad_same.add(name + ".ll", load("new", name, "g_ll"), load("parent", name, "g_ll"))
        grad_same.add(name + ".grad", load("new", name, "g_grad"), load("parent", name, "g_grad"))
        hval_same.add(name + ".ll", load("new", name, "h_ll"), load("parent", name, "h_ll"))
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
    lines = ["# the derivative entry points, new library against the parent's (tools/compare_deriv_libs.py)"]
    for e in (grad_same, hval_same):
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
    return 1 if grad_same.differ or hval_same.differ else 0


if __name__ == "__main__":
    sys.exit(main())
