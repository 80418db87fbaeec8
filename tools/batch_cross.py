"""What a histogram batch costs, measured: writes profiles/batch_cross.txt.

Cross: the repeat model on tests/golden/H10k_rep_trim.hist, B in {16, 256} replicates drawn at the golden optimum, a
seeded list of 4096 points around it.  Per B: the cross call's time (median of 20 after 3 warm-ups, HIP events on the
library's stream around the call), its split into the table kernels, the contraction kernels and the remainder (fix-up,
read-backs and copies) from the batch's own events (covest_batch_info), the contraction's achieved fp64 rate beside the
75 TFLOP/s this project measured for v_mfma_f64_16x16x4_f64 (header of ll_factored.hip), and the route without a
batch for the same job, in the same process: B twin models, each loglikelihood_points(points) (median of 3 passes
after 1; the models are created before the clock starts, their creation is timed beside it).

Bootstrap: parametric_bootstrap with 64 replicates, sequential against lock-step, both models, wall time.

Every step that uses the GPU is a child process under a time limit of its own, and the steps are chained: the first
that fails ends the run.  Nothing is tuned and no ratio is asserted: the file is the record.

    python tools/batch_cross.py [--out profiles/batch_cross.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SEED = 1
N_POINTS = 4096
MFMA_F64_TFLOPS = 75.0  # measured by this project for the instruction (ll_factored.hip's header)
STEPS = (("cross-16", 240), ("cross-256", 420), ("bootstrap-basic", 200), ("bootstrap-repeats", 300))


def golden_repeats_model():
    import numpy as np
    from conftest import load_golden, load_hist
    from covest_amd import RepeatsModel
    g = load_golden("c3_trim.json")
    cand = g["candidates"]
    at = np.unravel_index(cand["flat_index"][int(np.argmax(cand["ll"]))], [len(a) for a in g["axes"]])
    c, e, q1, q = (g["axes"][d][i] for d, i in enumerate(at))
    model = RepeatsModel(g["k"], g["r"], load_hist(g["hist"]), g["tail"], max_error=g["max_error"])
    return model, [c, e, q1, g["q2"], q]


class DeviceClock:
    """HIP events on the null stream of the runtime the library is bound to."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.hip.hipEventCreate(ctypes.byref(self.a)) == 0 and self.hip.hipEventCreate(ctypes.byref(self.b)) == 0

    def ms(self, call):
        assert self.hip.hipEventRecord(self.a, None) == 0
        call()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        out = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(out), self.a, self.b) == 0
        return float(out.value)


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
        cross = batch.loglikelihood_cross(pts)
    runs = []
    for _ in range(20):
        ms = clock.ms(lambda: batch.loglikelihood_cross(pts))
        info = batch.info()
        runs.append((ms, info["table_ns"] / 1e6, info["contraction_ns"] / 1e6, info))
    ms, table_ms, contract_ms = (statistics.median(r[i] for r in runs) for i in range(3))
    info = runs[-1][3]
    n_keys = len(model.hist)
    flops = 2.0 * n_hist * N_POINTS * n_keys
    counts, tails = batch.counts()
    keys = list(model.hist)
    t0 = time.perf_counter()
    twins = [_replicate_model(model, keys, counts[b], tails[b]) for b in range(n_hist)]
    for twin in twins:
        twin.handle
    create_s = time.perf_counter() - t0
    passes, worst = [], 0.0
    for k in range(4):
        t0 = time.perf_counter()
        rows = [twin.loglikelihood_points(pts) for twin in twins]  # (each call ends in a blocking copy)
        passes.append(time.perf_counter() - t0)
    rows = np.array(rows)
    both = np.isfinite(rows) & np.isfinite(cross)
    worst = float(np.max(np.abs(rows[both] - cross[both]) / np.abs(rows[both])))
    record = twins[0].launch_record()["launches"]
    for twin in twins:
        twin.close()
    return {"n_hist": n_hist, "n_points": N_POINTS, "n_keys": n_keys, "cross_ms": ms, "table_ms": table_ms,
            "contraction_ms": contract_ms, "rest_ms": ms - table_ms - contract_ms, "info": info,
            "contraction_tflops": flops / (contract_ms * 1e-3) / 1e12, "twins_ms": statistics.median(passes[1:]) * 1e3,
            "twins_create_ms": create_s * 1e3, "twins_launches": record, "agree": worst,
            "specials_equal": bool(np.array_equal(np.isfinite(rows), np.isfinite(cross)))}


def step_bootstrap(kind):
    from conftest import load_hist
    from covest_amd import BasicModel, CoverageEstimator, constants, parametric_bootstrap
    from covest_amd.hist_steps import process_histogram
    if kind == "basic":
        hist, tail, _, guess_c, guess_e = process_histogram(load_hist("sim_c10_e0.05"), 21, 100)
        model = BasicModel(21, 100, hist, tail, max_error=constants.MAX_ERRORS)
        point, ok = CoverageEstimator(model, err_scale=constants.DEFAULT_ERR_SCALE).compute_coverage([guess_c, guess_e])
        options = {"err_scale": constants.DEFAULT_ERR_SCALE}
    else:
        model, point = golden_repeats_model()
        options = {}
    out = {"model": kind, "replicates": 64}
    for refit in ("sequential", "lockstep"):
        parametric_bootstrap(model, point, replicates=2, seed=SEED, refit=refit, **options)  # (code objects, buffers)
        t0 = time.perf_counter()
        boot = parametric_bootstrap(model, point, replicates=64, seed=SEED, refit=refit, **options)
        out[refit] = {"seconds": time.perf_counter() - t0, "failed": boot["failed"],
                      "mean": boot["mean"], "standard_errors": boot["standard_errors"]}
    return out


def write(path, parts):
    lines = ["# tools/batch_cross.py: a histogram batch against the route without one (DESIGN.md section 6r)",
             "# one MI355X; times in ms unless they say s; 'cross' by HIP events around the call, median of 20 after 3;",
             "# 'table' and 'contraction' are the batch's own events around its kernels, 'rest' the remainder of the call",
             "# (fix-up, the read-back of the dead-key counts, the copy of the result); 'twins' is B twin models, each",
             "# loglikelihood_points(points), host clock, median of 3 passes after 1, models created beforehand"]
    for name, _ in STEPS:
        p = parts[name]
        if name.startswith("cross"):
            lines.append("# [%s] repeat model, H10k_rep_trim, %d keys, B = %d drawn replicates, n = %d points"
                         % (name, p["n_keys"], p["n_hist"], p["n_points"]))
            lines.append("    cross %.3f = table %.3f + contraction %.3f + rest %.3f; chunks %d, tiles %d, dead points %d,"
                         " fix-up waves %d" % (p["cross_ms"], p["table_ms"], p["contraction_ms"], p["rest_ms"],
                                               p["info"]["table_chunks"], p["info"]["cross_tiles"],
                                               p["info"]["dead_points"], p["info"]["fixup_waves"]))
            share = p["contraction_tflops"] / MFMA_F64_TFLOPS
            lines.append("    contraction %.2f TFLOP/s fp64 = %.1f %% of the %.0f TFLOP/s measured for v_mfma_f64_16x16x4_f64%s"
                         % (p["contraction_tflops"], 100 * share, MFMA_F64_TFLOPS,
                            " -- below half the instruction's rate: it reads its operands from HBM/L2 lane by lane and is"
                            " not the bottleneck while the table is K-direct's" if share < 0.5 else ""))
            lines.append("    twins %.1f (+ %.1f to create the models), launches of one twin %s; twins / cross = %.2f"
                         % (p["twins_ms"], p["twins_create_ms"], json.dumps(p["twins_launches"], sort_keys=True),
                            p["twins_ms"] / p["cross_ms"]))
            lines.append("    largest relative difference cross against twins %.3g; specials in the same places: %s"
                         % (p["agree"], p["specials_equal"]))
        else:
            s, l = p["sequential"], p["lockstep"]
            lines.append("# [%s] parametric_bootstrap, %s model, %d replicates, wall time" % (name, p["model"], p["replicates"]))
            lines.append("    sequential %.2f s (failed %d), lock-step %.2f s (failed %d); sequential / lock-step = %.2f"
                         % (s["seconds"], s["failed"], l["seconds"], l["failed"], s["seconds"] / l["seconds"]))
            for pname in s["mean"]:
                if s["mean"][pname] is not None:
                    lines.append("    %-12s mean %.6g | %.6g   se %.3g | %.3g   (sequential | lock-step)"
                                 % (pname, s["mean"][pname], l["mean"][pname], s["standard_errors"][pname],
                                    l["standard_errors"][pname]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_cross.txt"))
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
