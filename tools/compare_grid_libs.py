"""Two builds of the library side by side on dense repeats grids (covest_grid_*; K-factored's planner, plan_factored.cpp):
what a change did to the numbers and to the plans.

For each library, in a child process of its own (COVEST_AMD_LIB is read at import), every set below is evaluated; the
whole log-likelihood array, the arg-min pair and launch_record() (launches, and every field of every plan) are dumped and
then compared: nothing may differ.  A set that does not show the plan feature it is there for fails the run.  The sets:
  * every entry of tests/test_gpu_variants.py FACTORED_CASES (imported), and the launch-split grid of
    test_factored_grid_variants (restated here: the test builds it inside its body);
  * the bench workloads c3 and c3t (bench.workload);
  * one handle re-configured through DenseGrid.reset over the grids of two optimize_grid searches on the 15-key
    histogram -- grids of at most kArgminSmall = 16384 points, which a reset handle reads in place, with several
    workgroups per (c, e) -- the second search started next to the bounds, so that its axes are cut by them.  (A grid
    the bounds cut down to under a thousand points goes to K-direct under kernel="auto": it is compared like the others
    and not asked for K-factored's features, and most of the grids must be K-factored's);
  * ragged flat_range blocks of the sets in RAGGED, against the other library's and against the own whole grid.

  * the basic model's hand-back: the grid with a subnormal key of every entry of tests/test_gpu_variants.py BASIC_CASES
    (K-basic queues points, the strict pass patches them: every fix_basic_packed<S>, and fix_list<2,1> at 22 classes).

    python tools/compare_grid_libs.py --new covest_amd/lib/libcovest_amd.so --parent /path/lib_parent.so \
        [--work DIR] [--out profiles/plan_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402

RAGGED = ("shared steps", "long parts S8", "22 classes")
SEARCHES = ([10.0, 0.05, 0.65, 0.5, 0.5], [10.0, 0.05, 0.95, 0.97, 0.93])  # bench.py's og start; one beside q1, q2, q <= 1
IN_PLACE_MAX = 16384  # kernels.h kArgminSmall


def _launched(prefixes):
    return lambda rec: [p for p in prefixes if not any(n.startswith(p) for n in rec["launches"])]


def grid_sets():
    """(name, model arguments, axes, kernel, check): check(record) -> what the set missed (empty: on its route).  Model
    arguments: (k, r, histogram, tail, max_error), the repeats model's; with "basic" in front, the basic model's."""
    import test_gpu_variants as tv
    from bench import load_hist, workload, workload_tail
    out = []
    for name, hist, tail, S, k, axes, launches, plan_ok in tv.FACTORED_CASES:
        def check(rec, launches=launches, plan_ok=plan_ok):
            return sorted(set(launches) - set(rec["launches"])) + ([] if plan_ok(rec["plans"]) else ["its plan predicate"])
        out.append((name, (k, 100, hist, tail, S), axes, "factored", check))
    # tests/test_gpu_variants.py test_factored_grid_variants: past the launch split, 2 049 x 2 049 rows, two weight vectors
    axes = [np.linspace(0.5, 30.0, 2049), np.linspace(0.001, 0.2, 2049), [0.7], [0.5], [0.3, 0.8]]
    def split(rec):
        n = sum(c for name, c in rec["launches"].items() if name.startswith("ll_factored<"))
        return ([] if tv._plan(n_qblocks=1)(rec["plans"]) else ["n_qblocks=1"]) + ([] if n > 1 else ["more than one launch"])
    out.append(("launch split", (21, 100, tv._falling(range(1, 21), 5000), 0, 8), axes, "factored", split))
    for k, S, basic, fix in tv.BASIC_CASES:
        for tail in (0, 9):
            launches = [basic % (",tail" if tail else ""), fix]
            out.append(("basic k%d S%d%s" % (k, S, " tail" if tail else ""), ("basic", k, 100, tv.SUB_HIST, tail, S),
                        tv._basic_axes(k), "recur", lambda rec, launches=launches: sorted(set(launches) - set(rec["launches"]))))
    for w in ("c3", "c3t"):
        kind, hname, axes = workload(w, 1)
        out.append(("bench " + w, (21, 100, load_hist(hname), workload_tail(w), 8), axes, "auto", _launched(["ll_factored<"])))
    return out


def _evaluate(grid, kernel):
    grid.evaluate(kernel=kernel)
    best = grid.argmin()
    return grid.loglikelihoods(), np.array([best[0], float(best[1])]), grid.launch_record()


def _ragged(m, axes, kernel, name, total):
    import test_gpu_variants as tv
    from covest_amd import DenseGrid
    cuts = [0] + sorted(int(c) for c in tv._sample(name + " cuts", total - 2, 2) + 1) + [total]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        blk = DenseGrid(m, axes, flat_range=(lo, hi))
        blk.evaluate(kernel=kernel)
        parts.append(blk.loglikelihoods())
        blk.close()
    return np.concatenate(parts)


def search_grids(m):
    """The model-space axes of every grid the searches of SEARCHES evaluate, in order."""
    from covest_amd import CoverageEstimator, optimize_grid
    est = CoverageEstimator(m)
    grids, grid_for = [], est._grid_for

    def recording(axes):
        grids.append([np.array(a, dtype=np.float64) for a in axes])
        return grid_for(axes)

    est._grid_for = recording
    for guess in SEARCHES:
        optimize_grid(est.likelihood_f, list(guess), bounds=est.bounds)
    return grids


def dump(work):
    from bench import load_hist
    from covest_amd import BasicModel, DenseGrid, RepeatsModel, constants
    records = {}

    def keep(name, ll, best, rec, missed):
        np.save(os.path.join(work, "%s.ll.npy" % name), ll)
        np.save(os.path.join(work, "%s.best.npy" % name), best)
        records[name] = {"launches": sorted(rec["launches"].items()), "plans": rec["plans"], "missed": missed}
        print("done: %s" % name, file=sys.stderr, flush=True)  # (progress, for a caller that watches the run)

    for name, margs, axes, kernel, check in grid_sets():
        cls = BasicModel if margs[0] == "basic" else RepeatsModel
        k, r, hist, tail, S = margs[-5:]
        m = cls(k, r, hist, tail, max_error=S)
        g = DenseGrid(m, axes)
        ll, best, rec = _evaluate(g, kernel)
        keep(name, ll, best, rec, check(rec))
        if name in RAGGED:
            blocks = _ragged(m, axes, kernel, name, g.total)
            np.save(os.path.join(work, "%s.blocks.npy" % name), blocks)
            if not np.array_equal(blocks, ll, equal_nan=True):
                records[name]["missed"].append("ragged blocks differ from the own whole grid")
        g.close()
        m.close()
    m = RepeatsModel(21, 100, load_hist("sim_c10_e0.05"), 0, max_error=8)
    grids = search_grids(m)
    g, n_cut, n_direct = None, 0, 0
    for i, axes in enumerate(grids):
        g = DenseGrid(m, axes) if g is None else g.reset(axes)
        ll, best, rec = _evaluate(g, "auto")
        cut = any(1 < len(a) < 2 * constants.GRID_DEPTH for a in axes) or any(len(a) == 0 for a in axes)
        n_cut += cut
        direct = "ll_direct" in rec["launches"] and not rec["plans"]  # (too few points for K-factored: see the head)
        n_direct += direct
        missed = [] if direct else _launched(["ll_factored<"])(rec)
        if i and len(ll) > IN_PLACE_MAX:
            missed.append("%d points: not read in place" % len(ll))
        if not direct and not any(p["n_qblocks"] > 1 and p["list_mode"] == 0 for p in rec["plans"]):
            missed.append("several workgroups per (c, e)")
        keep("reset %02d%s" % (i, " cut" if cut else ""), ll, best, rec, missed)
    records["resets"] = {"launches": [], "plans": [], "missed": ([] if n_cut and len(grids) - n_cut > 1 else ["a grid cut by the bounds and two uncut ones"]) +
                         ([] if 2 * n_direct < len(grids) else ["%d of %d grids went to K-direct" % (n_direct, len(grids))])}
    g.close()
    m.close()
    with open(os.path.join(work, "records.json"), "w") as f:
        json.dump(records, f)


def compare(work, out):
    rec = {}
    for tag in ("new", "parent"):
        with open(os.path.join(work, tag, "records.json")) as f:
            rec[tag] = json.load(f)
    n_numbers = n_differ = n_records = n_rec_differ = n_missed = 0
    lines = ["# dense grids, new library against the parent's (tools/compare_grid_libs.py)"]
    if list(rec["new"]) != list(rec["parent"]):
        lines.append("the two libraries evaluated different sets: %s" % sorted(set(rec["new"]) ^ set(rec["parent"])))
        n_rec_differ += 1
    for name, r in rec["new"].items():
        rp = rec["parent"].get(name, {})
        differ, n = 0, 0
        for what in ("ll", "best", "blocks"):
            path = [os.path.join(work, tag, "%s.%s.npy" % (name, what)) for tag in ("new", "parent")]
            if not os.path.exists(path[0]):
                continue
            a, b = np.load(path[0]), np.load(path[1]) if os.path.exists(path[1]) else None
            n += a.size
            differ += a.size if b is None or a.shape != b.shape else int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
        same_rec = (r["launches"], r["plans"]) == (rp.get("launches"), rp.get("plans"))
        n_numbers, n_differ, n_records, n_rec_differ = n_numbers + n, n_differ + differ, n_records + 1, n_rec_differ + (not same_rec)
        n_missed += len(r["missed"])
        plans = " | ".join(" ".join("%s=%d" % kv for kv in p.items()) for p in r["plans"])
        lines.append("  %-30s %9d numbers, %d differ; record %s; %s\n      %s\n      %s" % (
            name, n, differ, "as the parent's" if same_rec else "DIFFERS from the parent's %s %s" % (rp.get("launches"), rp.get("plans")),
            "misses " + "; ".join(r["missed"]) if r["missed"] else "shows what it is there for",
            " ".join("%s x%d" % (k, c) for k, c in r["launches"]), plans))
    lines.insert(1, "%d numbers compared (log-likelihoods, arg-min pairs, ragged blocks): %d differ; %d launch records (launches and "
                    "every field of every plan): %d differ; features the sets are there for: %d missed"
                 % (n_numbers, n_differ, n_records, n_rec_differ, n_missed))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 1 if n_differ or n_rec_differ or n_missed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="(child) evaluate with the library COVEST_AMD_LIB selects and dump the arrays here")
    ap.add_argument("--new")
    ap.add_argument("--parent")
    ap.add_argument("--work")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plan_ab.txt"))
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
        return 0
    work = args.work or tempfile.mkdtemp(prefix="plan_ab_")
    for tag, lib in (("new", args.new), ("parent", args.parent)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", os.path.join(work, tag)], env=env, timeout=900).returncode
        if rc != 0:  # nothing more is started after a child that failed
            print("the %s library's run ended with status %d" % (tag, rc))
            return 1
    return compare(work, args.out)


if __name__ == "__main__":
    sys.exit(main())
