"""What the Hessian of a histogram batch costs, measured: writes profiles/batch_hess.txt.

Throughput: tools/batch_grad.py's job -- the repeat model on tests/golden/H10k_rep_trim.hist, B in {16, 256} replicates drawn
at the golden optimum, tools/batch_cross.py's seeded list of 4096 points around it.  Per B: the Hessian cross call's time
(covest_batch_eval_cross_hess into a buffer allocated beforehand; median of 20 after 3 warm-ups, HIP events around the call,
the smallest and the largest beside it), its split into the table kernels (the derivative kernel's walk at order 2, its
finishing pass, the packing of the tail coefficients), the contraction kernels (the MFMA contraction over R2 n = 21 n
rows, the fix-up and the specials pass) and the rest (read-backs and the copy of B n 21 doubles) from the batch's own
events (covest_batch_info); the method's mirror of the triangle on the host beside it (host clock); the 4096-request Hessian
pairs call likewise; the gradient cross call of the same batch; and the route without a batch for the same job in the same
process -- B twin models, each loglikelihood_hessian_points(points), median of 2 passes after 1.

Bootstrap: parametric_bootstrap with 64 replicates, the basic model on sim_c10_e0.05 and the repeat model, every refit
route, studentized=True against False: wall time (median of 3 alternating runs after a warm-up of 2 replicates).

Every step that uses the GPU is a child process under a time limit of its own, and the steps are chained: the first that
fails ends the run.  Nothing is tuned and no ratio is asserted: the file is the record.

    python tools/batch_hess.py [--out profiles/batch_hess.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from batch_cross import N_POINTS, SEED, DeviceClock, golden_repeats_model  # noqa: E402

STEPS = (("cross-16", 300), ("cross-256", 600), ("bootstrap-basic", 300), ("bootstrap-repeats", 400))
ROUTES = (("lockstep-gradient", {}), ("lockstep", {}), ("sequential", {"gradient": "analytic"}))
R2 = 21


def _spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def _timed(clock, batch, call):
    """20 calls after 3: [(ms by events, table ms, contraction ms)]."""
    for _ in range(3):
        call()
    runs = []
    for _ in range(20):
        ms = clock.ms(call)
        info = batch.info()
        runs.append((ms, info["table_ns"] / 1e6, info["contraction_ns"] / 1e6))
    return {"call_ms": _spread([r[0] for r in runs]), "table_ms": _spread([r[1] for r in runs]),
            "contraction_ms": _spread([r[2] for r in runs])}


def step_cross(n_hist):
    import numpy as np
    from covest_amd import HistogramBatch, _capi
    from covest_amd.bootstrap import _replicate_model
    model, optimum = golden_repeats_model()
    rng = np.random.default_rng(SEED)
    pts = np.array(optimum) * rng.uniform(0.9, 1.1, size=(N_POINTS, 5))
    for d, (lo, hi) in enumerate(model.bounds):
        pts[:, d] = np.clip(pts[:, d], lo, hi)
    pts = np.ascontiguousarray(pts)
    batch = HistogramBatch.draw(model, optimum, n_hist, seed=SEED)
    clock = DeviceClock()
    lib, handle = _capi.lib(), batch._open()
    out = np.empty((n_hist, N_POINTS, R2), dtype=np.float64)
    index = np.ascontiguousarray(np.arange(N_POINTS) % n_hist, dtype=np.int64)
    out_pairs = np.empty((N_POINTS, R2), dtype=np.float64)
    cross = _timed(clock, batch, lambda: _capi.check(lib.covest_batch_eval_cross_hess(handle, N_POINTS, pts.ctypes.data, out.ctypes.data), "cross_hess"))
    info = batch.info()
    pairs = _timed(clock, batch, lambda: _capi.check(lib.covest_batch_eval_pairs_hess(handle, N_POINTS, index.ctypes.data, pts.ctypes.data,
                                                                                     out_pairs.ctypes.data), "pairs_hess"))
    grad = _timed(clock, batch, lambda: batch.loglikelihood_gradient_cross(pts))
    t0 = time.perf_counter()
    ll, g, hess = batch.loglikelihood_hessian_cross(pts)
    method_ms = (time.perf_counter() - t0) * 1e3
    del out
    counts, tails = batch.counts()
    keys = list(model.hist)
    t0 = time.perf_counter()
    twins = [_replicate_model(model, keys, counts[b], tails[b]) for b in range(n_hist)]
    for twin in twins:
        twin.handle
    create_s = time.perf_counter() - t0
    passes = []
    worst_ll = worst_h = 0.0
    specials = True
    for at in range(3):
        t0 = time.perf_counter()
        rows = [twin.loglikelihood_hessian_points(pts) for twin in twins]  # (each call ends in a blocking copy)
        passes.append((time.perf_counter() - t0) * 1e3)
    scale = np.maximum(np.abs(np.array([r[2] for r in rows])).max(axis=(0, 1)), 1e-300)  # per entry: the job's largest
    for b, (t_ll, _, t_h) in enumerate(rows):
        both = np.isfinite(t_ll) & np.isfinite(ll[b])
        specials = specials and bool(np.array_equal(np.isfinite(t_ll), np.isfinite(ll[b])))
        worst_ll = max(worst_ll, float(np.max(np.abs(t_ll[both] - ll[b][both]) / np.abs(t_ll[both]))))
        worst_h = max(worst_h, float(np.max(np.abs(t_h - hess[b])[both] / scale)))
    for twin in twins:
        twin.close()
    return {"n_hist": n_hist, "n_points": N_POINTS, "n_keys": len(model.hist), "info": info, "cross": cross, "pairs": pairs,
            "grad": grad, "method_ms": method_ms, "result_mb": n_hist * N_POINTS * R2 * 8 / 1e6,
            "twins_ms": _spread(passes[1:]), "twins_create_ms": create_s * 1e3, "agree_ll": worst_ll, "agree_hess": worst_h,
            "specials_equal": specials}


def step_bootstrap(kind):
    from conftest import load_golden, load_hist
    from covest_amd import BasicModel, constants, observed_information, parametric_bootstrap
    from covest_amd.hist_steps import process_histogram
    if kind == "basic":
        hist, tail, _, _, _ = process_histogram(load_hist("sim_c10_e0.05"), 21, 100)
        model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
        opt = load_golden("own_optimum.json")["models"]["basic"]
        point = [opt[name] for name in model.params]
        options = {"err_scale": constants.DEFAULT_ERR_SCALE}
    else:
        model, point = golden_repeats_model()
        options = {}
    original = observed_information(model, point)
    out = {"model": kind, "replicates": 64, "original_reason": original["reason"], "original_se": original["standard_errors"]}
    cases = [(refit, extra, st) for refit, extra in ROUTES for st in (False, True)]
    seconds, last = {(r, st): [] for r, _, st in cases}, {}
    for refit, extra, st in cases:
        parametric_bootstrap(model, point, replicates=2, seed=SEED, refit=refit, studentized=st, **dict(options, **extra))
    for _ in range(3):  # the cases alternate: what else the machine does falls on all of them
        for refit, extra, st in cases:
            t0 = time.perf_counter()
            last[(refit, st)] = parametric_bootstrap(model, point, replicates=64, seed=SEED, refit=refit, studentized=st,
                                                     **dict(options, **extra))
            seconds[(refit, st)].append(time.perf_counter() - t0)
    for refit, _ in ROUTES:
        boot = last[(refit, True)]
        out[refit] = {"plain_s": _spread(seconds[(refit, False)]), "studentized_s": _spread(seconds[(refit, True)]),
                      "failed": boot["failed"], "used": boot["studentized_used"], "t_intervals": boot["t_intervals"],
                      "percentile_intervals": boot["percentile_intervals"]}
    return out


def _ms(s):
    return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])


def _split(p):
    rest = p["call_ms"]["median"] - p["table_ms"]["median"] - p["contraction_ms"]["median"]
    return "call %s = table %s + contraction %s + rest %.3f" % (_ms(p["call_ms"]), _ms(p["table_ms"]), _ms(p["contraction_ms"]), rest)


def write(path, parts):
    lines = ["# tools/batch_hess.py: the Hessian of a histogram batch against the routes without it (DESIGN.md section 6x)",
             "# one MI355X; times in ms unless they say s, as median (smallest .. largest) of the repeats; 'call' by HIP events",
             "# around the entry point (its result buffer allocated beforehand), 20 after 3; 'table' and 'contraction' are the",
             "# batch's own events around its kernels (table: the derivative kernel's walk at order 2, its finishing pass, the",
             "# packing of the tail coefficients; contraction: the MFMA kernel over 21 n rows or the pairs kernel, the fix-up and",
             "# the specials pass), 'rest' the remainder of the call (the read-back of the dead-key counts, the copy of the",
             "# result); 'twins' is B twin models, each loglikelihood_hessian_points(points), host clock, 2 passes after 1, models",
             "# created beforehand; 'gradient cross' is loglikelihood_gradient_cross of the same batch.  None is a pass mark."]
    for name, _ in STEPS:
        p = parts[name]
        if name.startswith("cross"):
            lines.append("# [%s] repeat model, H10k_rep_trim, %d keys, B = %d drawn replicates, n = %d points, %d table rows a point"
                         % (name, p["n_keys"], p["n_hist"], p["n_points"], R2))
            c = p["cross"]
            rest = c["call_ms"]["median"] - c["table_ms"]["median"] - c["contraction_ms"]["median"]
            lines.append("    Hessian cross:  %s; chunks %d, tiles %d, dead points %d" % (_split(c), p["info"]["table_chunks"],
                                                                                           p["info"]["cross_tiles"], p["info"]["dead_points"]))
            lines.append("                    the result is %.1f MB: rest / call = %.2f; the method (mirror of the triangle on the host"
                         " included), one call by the host clock: %.1f" % (p["result_mb"], rest / c["call_ms"]["median"], p["method_ms"]))
            lines.append("    Hessian pairs:  %s (%d requests)" % (_split(p["pairs"]), p["n_points"]))
            lines.append("    gradient cross: %s; Hessian call / gradient call = %.2f, table / table = %.2f"
                         % (_split(p["grad"]), c["call_ms"]["median"] / p["grad"]["call_ms"]["median"],
                            c["table_ms"]["median"] / p["grad"]["table_ms"]["median"]))
            lines.append("    twins %s (+ %.1f to create the models); twins / Hessian cross = %.1f"
                         % (_ms(p["twins_ms"]), p["twins_create_ms"], p["twins_ms"]["median"] / c["call_ms"]["median"]))
            lines.append("    against the twins: value, largest relative difference %.3g; Hessian, largest difference over the job's"
                         " largest entry of the pair %.3g; specials in the same places: %s" % (p["agree_ll"], p["agree_hess"], p["specials_equal"]))
        else:
            lines.append("# [%s] parametric_bootstrap, %s model, %d replicates, wall time in s, 3 alternating runs"
                         % (name, p["model"], p["replicates"]))
            for refit, extra in ROUTES:
                r = p[refit]
                label = refit + (' gradient="analytic"' if extra else "")
                a, b = r["plain_s"], r["studentized_s"]
                lines.append("    %-32s studentized=False %.3f (%.3f .. %.3f) s, True %.3f (%.3f .. %.3f) s, True - False = %.3f s;"
                             " failed %d, used %s" % (label, a["median"], a["min"], a["max"], b["median"], b["min"], b["max"],
                                                      b["median"] - a["median"], r["failed"],
                                                      "/".join(str(v) for v in r["used"].values())))
            lines.append("    the original's own standard errors: %s%s" % (
                ", ".join("%s %s" % (n, "none" if v is None else "%.3g" % v) for n, v in p["original_se"].items()),
                "" if p["original_reason"] is None else " (%s)" % p["original_reason"]))
            r = p["lockstep-gradient"]
            for pname, iv in r["t_intervals"].items():
                if iv is not None:
                    lines.append("    %-12s t-interval [%.8g, %.8g]   percentile [%.8g, %.8g]   (lockstep-gradient)"
                                 % ((pname,) + tuple(iv) + tuple(r["percentile_intervals"][pname])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_hess.txt"))
    ap.add_argument("--step", help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        kind, _, what = args.step.partition("-")
        result = step_cross(int(what)) if kind == "cross" else step_bootstrap(what)
        print("RESULT " + json.dumps(result))
        return 0
    parts = {}
    for name, limit in STEPS:  # chained: the first step that fails, faults or runs out of time ends the run
        run = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                             capture_output=True, text=True)
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout + run.stderr)
            sys.stderr.write("step %s ended with status %d: nothing more is started\n" % (name, run.returncode))
            return run.returncode or 1
        parts[name] = json.loads(found[-1][len("RESULT "):])
        print("step %s done" % name, flush=True)
    write(args.out, parts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
