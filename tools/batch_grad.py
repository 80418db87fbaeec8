"""What the gradient of a histogram batch costs, measured: writes profiles/batch_grad.txt.

Throughput: the repeat model on tests/golden/H10k_rep_trim.hist, B in {16, 256} replicates drawn at the golden optimum,
tools/batch_cross.py's seeded list of 4096 points around it.  Per B: the gradient-cross call's time (median of 20 after 3
warm-ups, HIP events on the library's stream around the call; beside it the smallest and the largest of the 20), its
split into the table kernels (the derivative kernel's walk, its finishing pass, the packing of the tail coefficients),
the contraction kernels (the MFMA contraction over (P + 1) n rows, the fix-up and the specials pass) and the remainder
(read-backs and the copy of the result) from the batch's own events (covest_batch_info); the route without a batch for
the same job in the same process -- B twin models, each loglikelihood_gradient_points(points), median of 3 passes after
1 --; and the value-only loglikelihood_cross of the same batch, for scale.

Bootstrap: parametric_bootstrap with 64 replicates, both models: refit="lockstep-gradient" against "lockstep" and against
"sequential" with gradient="analytic"; wall time (median of 3 runs after a warm-up of 2 replicates, smallest and largest
beside it), failed refits, and the rounds of evaluation: for the lock-step routes the merged launches, for the
sequential one the evaluations of the replicate that took most and their total.

Every step that uses the GPU is a child process under a time limit of its own, and the steps are chained: the first
that fails ends the run.  Nothing is tuned and no ratio is asserted: the file is the record.

    python tools/batch_grad.py [--out profiles/batch_grad.txt]
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

STEPS = (("cross-16", 300), ("cross-256", 500), ("bootstrap-basic", 300), ("bootstrap-repeats", 400))
ROUTES = (("lockstep-gradient", {}), ("lockstep", {}), ("sequential", {"gradient": "analytic"}))


def _spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def step_cross(n_hist):
    import numpy as np
    from covest_amd import HistogramBatch
    from covest_amd.bootstrap import _replicate_model
    model, optimum = golden_repeats_model()
    rng = np.random.default_rng(SEED)
    pts = np.array(optimum) * rng.uniform(0.9, 1.1, size=(N_POINTS, 5))
    for d, (lo, hi) in enumerate(model.bounds):
        pts[:, d] = np.clip(pts[:, d], lo, hi)
    batch = HistogramBatch.draw(model, optimum, n_hist, seed=SEED)
    clock = DeviceClock()
    for _ in range(3):
        ll, grad = batch.loglikelihood_gradient_cross(pts)
    runs = []
    for _ in range(20):
        ms = clock.ms(lambda: batch.loglikelihood_gradient_cross(pts))
        info = batch.info()
        runs.append((ms, info["table_ns"] / 1e6, info["contraction_ns"] / 1e6))
    info = batch.info()
    for _ in range(3):
        value = batch.loglikelihood_cross(pts)
    value_runs = []
    for _ in range(20):
        ms = clock.ms(lambda: batch.loglikelihood_cross(pts))
        value_info = batch.info()
        value_runs.append((ms, value_info["table_ns"] / 1e6, value_info["contraction_ns"] / 1e6))
    counts, tails = batch.counts()
    keys = list(model.hist)
    t0 = time.perf_counter()
    twins = [_replicate_model(model, keys, counts[b], tails[b]) for b in range(n_hist)]
    for twin in twins:
        twin.handle
    create_s = time.perf_counter() - t0
    passes = []
    for _ in range(4):
        t0 = time.perf_counter()
        rows = [twin.loglikelihood_gradient_points(pts) for twin in twins]  # (each call ends in a blocking copy)
        passes.append((time.perf_counter() - t0) * 1e3)
    twin_ll = np.array([r[0] for r in rows])
    twin_grad = np.array([r[1] for r in rows])
    for twin in twins:
        twin.close()
    both = np.isfinite(twin_ll) & np.isfinite(ll)
    scale = np.maximum(np.abs(twin_grad).max(axis=(0, 1)), 1e-300)  # per parameter: the largest component of the job
    return {"n_hist": n_hist, "n_points": N_POINTS, "n_keys": len(model.hist), "info": info,
            "call_ms": _spread([r[0] for r in runs]), "table_ms": _spread([r[1] for r in runs]),
            "contraction_ms": _spread([r[2] for r in runs]),
            "value_ms": _spread([r[0] for r in value_runs]), "value_table_ms": _spread([r[1] for r in value_runs]),
            "value_contraction_ms": _spread([r[2] for r in value_runs]),
            "twins_ms": _spread(passes[1:]), "twins_create_ms": create_s * 1e3,
            "agree_ll": float(np.max(np.abs(twin_ll[both] - ll[both]) / np.abs(twin_ll[both]))),
            "agree_value": float(np.max(np.abs(value[both] - ll[both]) / np.abs(value[both]))),
            "agree_grad": float(np.max(np.abs(twin_grad - grad)[both] / scale)),
            "specials_equal": bool(np.array_equal(np.isfinite(twin_ll), np.isfinite(ll)))}


class _Count:
    """Calls of a method, counted without changing what it returns."""

    def __init__(self, cls, name):
        self.cls, self.name, self.calls, self.original = cls, name, [], getattr(cls, name)
        counter = self

        def wrapped(this, *args, **kwargs):
            counter.calls.append(this)
            return counter.original(this, *args, **kwargs)

        setattr(cls, name, wrapped)

    def restore(self):
        setattr(self.cls, self.name, self.original)


def step_bootstrap(kind):
    from conftest import load_golden, load_hist
    from covest_amd import BasicModel, HistogramBatch, RepeatsModel, constants, parametric_bootstrap
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
    out = {"model": kind, "replicates": 64}
    seconds, last = {refit: [] for refit, _ in ROUTES}, {}
    for refit, extra in ROUTES:
        parametric_bootstrap(model, point, replicates=2, seed=SEED, refit=refit, **dict(options, **extra))  # (code objects, buffers)
    for _ in range(3):  # the routes alternate: what else the machine does falls on all of them
        for refit, extra in ROUTES:
            t0 = time.perf_counter()
            last[refit] = parametric_bootstrap(model, point, replicates=64, seed=SEED, refit=refit, **dict(options, **extra))
            seconds[refit].append(time.perf_counter() - t0)
    for refit, extra in ROUTES:
        counters = [_Count(HistogramBatch, "loglikelihood_pairs"), _Count(HistogramBatch, "loglikelihood_gradient_pairs"),
                    _Count(BasicModel if kind == "basic" else RepeatsModel, "loglikelihood_gradient_points")]
        try:
            parametric_bootstrap(model, point, replicates=64, seed=SEED, refit=refit, **dict(options, **extra))
        finally:
            for c in counters:
                c.restore()
        if refit == "lockstep":
            rounds = {"launches": len(counters[0].calls) - 1}  # (the last is the log-likelihood at the estimates)
        elif refit == "lockstep-gradient":
            rounds = {"launches": len(counters[1].calls)}
        else:
            per = {}
            for who in counters[2].calls:  # (the objects themselves are kept: no identity is used twice)
                per[id(who)] = per.get(id(who), 0) + 1
            rounds = {"launches": len(counters[2].calls), "most_of_one_replicate": max(per.values())}
        boot = last[refit]
        out[refit] = {"seconds": _spread(seconds[refit]), "failed": boot["failed"], "rounds": rounds, "mean": boot["mean"],
                      "standard_errors": boot["standard_errors"]}
    return out


def _ms(s):
    return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])


def write(path, parts):
    lines = ["# tools/batch_grad.py: the gradient of a histogram batch against the routes without it (DESIGN.md section 6u)",
             "# one MI355X; times in ms unless they say s, as median (smallest .. largest) of the repeats; 'call' by HIP events",
             "# around the call, 20 after 3; 'table' and 'contraction' are the batch's own events around its kernels (table: the",
             "# derivative kernel's walk, its finishing pass, the packing of the tail coefficients; contraction: the MFMA kernel",
             "# over (P + 1) n rows, the fix-up and the specials pass), 'rest' the remainder of the call (the read-back of the",
             "# dead-key counts, the copy of the result); 'twins' is B twin models, each loglikelihood_gradient_points(points), host",
             "# clock, 3 passes after 1, models created beforehand; 'value only' is loglikelihood_cross of the same batch"]
    for name, _ in STEPS:
        p = parts[name]
        if name.startswith("cross"):
            lines.append("# [%s] repeat model, H10k_rep_trim, %d keys, B = %d drawn replicates, n = %d points, %d table rows a point"
                         % (name, p["n_keys"], p["n_hist"], p["n_points"], 6))
            rest = p["call_ms"]["median"] - p["table_ms"]["median"] - p["contraction_ms"]["median"]
            lines.append("    gradient cross: call %s = table %s + contraction %s + rest %.3f; chunks %d, tiles %d, dead points %d"
                         % (_ms(p["call_ms"]), _ms(p["table_ms"]), _ms(p["contraction_ms"]), rest, p["info"]["table_chunks"],
                            p["info"]["cross_tiles"], p["info"]["dead_points"]))
            lines.append("    value only:     call %s = table %s + contraction %s; gradient call / value call = %.2f, table / table = %.2f"
                         % (_ms(p["value_ms"]), _ms(p["value_table_ms"]), _ms(p["value_contraction_ms"]),
                            p["call_ms"]["median"] / p["value_ms"]["median"], p["table_ms"]["median"] / p["value_table_ms"]["median"]))
            lines.append("    twins %s (+ %.1f to create the models); twins / gradient cross = %.1f"
                         % (_ms(p["twins_ms"]), p["twins_create_ms"], p["twins_ms"]["median"] / p["call_ms"]["median"]))
            lines.append("    against the twins: value, largest relative difference %.3g; gradient, largest difference over the job's"
                         " largest component of the parameter %.3g; against value only %.3g; specials in the same places: %s"
                         % (p["agree_ll"], p["agree_grad"], p["agree_value"], p["specials_equal"]))
        else:
            lines.append("# [%s] parametric_bootstrap, %s model, %d replicates, wall time in s, 3 runs" % (name, p["model"], p["replicates"]))
            for refit, extra in ROUTES:
                r = p[refit]
                label = refit + (' gradient="analytic"' if extra else "")
                rounds = ("%d merged launches" % r["rounds"]["launches"] if refit != "sequential" else
                          "%d evaluations, %d of the replicate that took most" % (r["rounds"]["launches"], r["rounds"]["most_of_one_replicate"]))
                lines.append("    %-32s %.3f (%.3f .. %.3f) s, failed %d, %s"
                             % (label, r["seconds"]["median"], r["seconds"]["min"], r["seconds"]["max"], r["failed"], rounds))
            g = p["lockstep-gradient"]["seconds"]["median"]
            lines.append("    lockstep / lockstep-gradient = %.2f, sequential analytic / lockstep-gradient = %.2f"
                         % (p["lockstep"]["seconds"]["median"] / g, p["sequential"]["seconds"]["median"] / g))
            for pname in p["sequential"]["mean"]:
                if p["sequential"]["mean"][pname] is not None:
                    lines.append("    %-12s mean %s   se %s   (lockstep-gradient | lockstep | sequential analytic)"
                                 % (pname, " | ".join("%.6g" % p[r]["mean"][pname] for r, _ in ROUTES),
                                    " | ".join("%.3g" % p[r]["standard_errors"][pname] for r, _ in ROUTES)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_grad.txt"))
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
