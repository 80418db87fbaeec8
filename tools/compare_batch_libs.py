"""Two builds of the library side by side on histogram batches (covest_batch_*; abi_batch.cpp, ll_batch.hip): what a change
did to the numbers, to the counters and, with --time, to the time of a call.

Values.  For each library, in a child process of its own (COVEST_AMD_LIB is read at import) under a time limit of its
own, every job below is evaluated and every array it returns is dumped; the parent process compares the files' bytes
(NaN by bit pattern, the sign of a zero too): nothing may differ.  The jobs:
  * every shape of tests/test_gpu_batch.py SHAPES and of tests/batch_grad_shapes.py, through the six evaluating methods
    of HistogramBatch -- cross, pairs, arg-min, gradient cross, gradient pairs, score table -- and counts() of a draw;
  * the three two-chunk jobs of tests/test_gpu_batch_chunks.py (value pairs, gradient cross, score table; of the score
    table's 268 MB the SHA-256 is kept, and its tail coefficients whole);
  * after every call the count fields of info() (not the two time fields).

Times (--time).  The job of tools/batch_cross.py and batch_grad.py: the repeats model on H10k_rep_trim.hist, 4096 seeded
points, B in {16, 256} drawn replicates; the value cross call, the gradient cross call and the 4096-request pairs call,
value and gradient.  A figure is the median of 20 calls after 3 warm-ups by HIP events around the call; five rounds, the
libraries alternating, each round of each library a process of its own.  The rule is profiles/reads_refactor_ab.txt's:
accepted when the new library's median over the rounds is <= the parent's median (1 + s), s = (the parent's largest -
smallest) / its median.  A miss is recorded as a miss, with the split from info()'s time fields beside it.

The steps are chained: nothing more is started after a child that failed or ran out of time.

    python tools/compare_batch_libs.py --new covest_amd/lib/libcovest_amd.so --parent /path/lib_parent.so \\
        [--time] [--work DIR] [--out profiles/batch_refactor_ab.txt]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np  # noqa: E402

COUNT_FIELDS = ("points_tabled", "table_chunks", "cross_tiles", "dead_points", "fixup_waves", "pairs_requests")
ROUNDS, CALLS, WARM_UPS = 5, 20, 3
DUMP_LIMIT, CLOCK_LIMIT = 900, 300  # seconds a child may take


class Dump:
    def __init__(self, work):
        self.work, self.records = work, {}

    def keep(self, job, what, batch, arrays):
        """One call's arrays (a tuple or one array) and the counters it left."""
        arrays = arrays if isinstance(arrays, tuple) else (arrays,)
        for at, a in enumerate(arrays):
            np.save(os.path.join(self.work, "%s.%s.%d.npy" % (job, what, at)), np.ascontiguousarray(a))
        info = batch.info()
        self.records["%s.%s" % (job, what)] = {"arrays": len(arrays), "info": [info[f] for f in COUNT_FIELDS]}


def all_forms(dump, job, model, counts, tails, points):
    from covest_amd import HistogramBatch
    batch = HistogramBatch(model, counts, tails)
    index = np.arange(len(points)) % max(len(batch), 1)
    dump.keep(job, "cross", batch, batch.loglikelihood_cross(points))
    dump.keep(job, "pairs", batch, batch.loglikelihood_pairs(index, points))
    dump.keep(job, "argmin", batch, batch.argmin_cross(points))
    dump.keep(job, "grad_cross", batch, batch.loglikelihood_gradient_cross(points))
    dump.keep(job, "grad_pairs", batch, batch.loglikelihood_gradient_pairs(index, points))
    dump.keep(job, "score_table", batch, batch.score_table(points))
    batch.close()
    drawn = HistogramBatch.draw(model, model.fit_to_bounds(points[0].tolist()), replicates=3, seed=7, n_draws=5000)
    dump.keep(job, "draw", drawn, drawn.counts())
    drawn.close()
    print("done: %s" % job, file=sys.stderr, flush=True)


def two_chunk_jobs(dump):
    """tests/test_gpu_batch_chunks.py's three lists, whole."""
    import test_gpu_batch_chunks as tc
    from covest_amd import BasicModel, HistogramBatch, _capi
    model = BasicModel(tc.K, tc.R, tc._keys(), 0, max_error=tc.MAX_ERROR)
    # value pairs
    n = tc.PER_VALUE + 40
    at = np.array([3, 77, tc.PER_VALUE - 1, tc.PER_VALUE, tc.PER_VALUE + 39])
    counts, tails = tc._histograms(6, 1)
    batch = HistogramBatch(model, counts, tails)
    pts, index = np.tile(np.array([tc.FILLER]), (n, 1)), np.zeros(n, dtype=np.int64)
    pts[at], index[at] = tc.INSIDE, [1, 2, 3, 4, 5]
    dump.keep("two-chunks", "pairs", batch, batch.loglikelihood_pairs(index, pts))
    batch.close()
    # gradient cross and the score table: the same list, the dead-key point in the second chunk
    n = tc.PER_GRAD + 21
    at = np.array([tc.PER_GRAD - 1, tc.PER_GRAD, n - 1, tc.PER_GRAD + 10])
    counts, tails = tc._histograms(17, 2)
    batch = HistogramBatch(model, counts, tails)
    dead = tc._dead_keys(batch)
    batch.close()
    counts[2, dead] = 0.0
    counts[16] = counts[2]
    counts[16, dead[len(dead) // 2]] = 12345.0
    batch = HistogramBatch(model, counts, tails)
    pts = np.tile(np.array([tc.FILLER]), (n, 1))
    pts[at[:3]], pts[at[3]] = tc.INSIDE[:3], tc.DEAD_POINT
    dump.keep("two-chunks", "grad_cross", batch, batch.loglikelihood_gradient_cross(pts))
    rows, tail = np.empty((n, 3, tc.N_KEYS)), np.empty((n, 3))
    _capi.check(_capi.lib().covest_batch_score_table(batch._open(), n, pts.ctypes.data, rows.ctypes.data, tail.ctypes.data),
                "covest_batch_score_table")
    digest = np.frombuffer(hashlib.sha256(memoryview(rows).cast("B")).digest(), dtype=np.uint8)
    dump.keep("two-chunks", "score_table", batch, (digest, tail, rows[at]))
    dump.records["two-chunks.score_table"]["numbers"] = int(rows.size)
    batch.close()
    model.close()
    print("done: two-chunks", file=sys.stderr, flush=True)


def dump(work):
    import batch_grad_shapes as S
    import test_gpu_batch as tb
    from covest_amd import BasicModel, RepeatsModel
    from parity_helpers import _model
    d = Dump(work)
    for shape, name in zip(tb.SHAPES, tb.SHAPE_IDS):
        case = tb._case(*shape)
        cls = BasicModel if case["kind"] == "basic" else RepeatsModel
        model = cls(tb.K, tb.R, (case["keys"], case["own"]), case["model_tail"], max_error=tb.MAX_ERROR)
        all_forms(d, "value-" + name, model, case["counts"], case["tails"], case["points"])
        model.close()
    for name in S.SHAPES:
        case = S.shape(name)
        hist = case["spec"]["hist"]
        model = _model(case["spec"], hist=dict(zip(hist["keys"], hist["counts"])))
        all_forms(d, "grad-" + name, model, case["counts"], case["tails"], case["points"])
        model.close()
    two_chunk_jobs(d)
    with open(os.path.join(work, "records.json"), "w") as f:
        json.dump(d.records, f)


def compare(work):
    """(lines, failed)"""
    rec = {}
    for tag in ("new", "parent"):
        with open(os.path.join(work, tag, "records.json")) as f:
            rec[tag] = json.load(f)
    lines, n_numbers, n_arrays, n_differ, n_info = [], 0, 0, 0, 0
    if list(rec["new"]) != list(rec["parent"]):
        lines.append("the two libraries ran different calls: %s" % sorted(set(rec["new"]) ^ set(rec["parent"])))
        n_differ += 1
    jobs = {}
    for call, r in rec["new"].items():
        rp = rec["parent"].get(call, {})
        differ, numbers = 0, r.get("numbers", 0)
        for at in range(r["arrays"]):
            raw = []
            for tag in ("new", "parent"):
                path = os.path.join(work, tag, "%s.%d.npy" % (call, at))
                raw.append(open(path, "rb").read() if os.path.exists(path) else None)  # (header and data: shape, type, bytes)
            numbers += np.load(os.path.join(work, "new", "%s.%d.npy" % (call, at))).size
            differ += raw[0] != raw[1]
        same_info = r["info"] == rp.get("info")
        n_numbers, n_arrays, n_differ, n_info = n_numbers + numbers, n_arrays + r["arrays"], n_differ + differ, n_info + (not same_info)
        job = jobs.setdefault(call.rsplit(".", 1)[0], [0, 0, 0, 0])
        job[0], job[1], job[2], job[3] = job[0] + 1, job[1] + numbers, job[2] + differ, job[3] + (not same_info)
        if differ or not same_info:
            lines.append("  %s: %d of its arrays DIFFER; counters %s (new) %s (parent)" % (call, differ, r["info"], rp.get("info")))
    for job, (calls, numbers, differ, info) in jobs.items():
        lines.append("  %-34s %d calls, %10d numbers, arrays that differ: %d, counter sets that differ: %d" % (job, calls, numbers, differ, info))
    lines.insert(0, "values: %d calls, %d arrays, %d numbers compared byte for byte (NaN by bit pattern): %d arrays differ; "
                    "count fields of info() after every call: %d sets differ" % (len(rec["new"]), n_arrays, n_numbers, n_differ, n_info))
    return lines, bool(n_differ or n_info)


def clock():
    """(child) the figures of one round with the library COVEST_AMD_LIB selects, as one RESULT line."""
    from batch_cross import N_POINTS, SEED, DeviceClock, golden_repeats_model
    from covest_amd import HistogramBatch
    model, optimum = golden_repeats_model()
    rng = np.random.default_rng(SEED)
    pts = np.array(optimum) * rng.uniform(0.9, 1.1, size=(N_POINTS, 5))
    for d, (lo, hi) in enumerate(model.bounds):
        pts[:, d] = np.clip(pts[:, d], lo, hi)
    timer, out = DeviceClock(), {}
    for n_hist in (16, 256):
        batch = HistogramBatch.draw(model, optimum, n_hist, seed=SEED)
        index = np.arange(N_POINTS) % n_hist
        calls = (("value cross", lambda: batch.loglikelihood_cross(pts)),
                 ("gradient cross", lambda: batch.loglikelihood_gradient_cross(pts)),
                 ("value pairs", lambda: batch.loglikelihood_pairs(index, pts)),
                 ("gradient pairs", lambda: batch.loglikelihood_gradient_pairs(index, pts)))
        for name, call in calls:
            for _ in range(WARM_UPS):
                call()
            runs = []
            for _ in range(CALLS):
                ms = timer.ms(call)
                info = batch.info()
                runs.append((ms, info["table_ns"] / 1e6, info["contraction_ns"] / 1e6))
            out["B=%d %s" % (n_hist, name)] = [statistics.median(r[at] for r in runs) for at in range(3)]
        batch.close()
    model.close()
    print("RESULT " + json.dumps(out))


def time_rounds(libs):
    """(lines, failed): ROUNDS rounds, the libraries alternating."""
    rounds = {"new": [], "parent": []}
    for r in range(ROUNDS):
        for tag in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
            run = subprocess.run(["timeout", "-k", "10", str(CLOCK_LIMIT), sys.executable, os.path.abspath(__file__), "--clock"],
                                 env=dict(os.environ, COVEST_AMD_LIB=libs[tag]), capture_output=True, text=True)
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout + run.stderr)
                return ["times: round %d of the %s library ended with status %d: nothing more was started" % (r, tag, run.returncode)], True
            rounds[tag].append(json.loads(found[-1][len("RESULT "):]))
            print("round %d %s done" % (r, tag), flush=True)
    lines = ["times: ms by HIP events around the call, median of %d calls after %d warm-ups; %d rounds, the libraries alternating,"
             % (CALLS, WARM_UPS, ROUNDS),
             "  a process each; per figure the median over the rounds (smallest .. largest); accepted when new <= parent (1 + s),",
             "  s = (parent's largest - smallest) / parent's median; [table + contraction] are info()'s time fields, medians likewise",
             "  (the parent's value pairs call does not time its contraction: 0)"]
    missed = 0
    for figure in rounds["parent"][0]:
        col = {tag: [[r[figure][at] for r in rounds[tag]] for at in range(3)] for tag in rounds}
        p, n = statistics.median(col["parent"][0]), statistics.median(col["new"][0])
        s = (max(col["parent"][0]) - min(col["parent"][0])) / p
        ok = n <= p * (1.0 + s)
        missed += not ok
        lines.append("  %-22s parent %8.3f (%8.3f .. %8.3f) [%7.3f + %6.3f]   new %8.3f (%8.3f .. %8.3f) [%7.3f + %6.3f]   new/parent %.4f, s %.4f: %s"
                     % (figure, p, min(col["parent"][0]), max(col["parent"][0]), statistics.median(col["parent"][1]),
                        statistics.median(col["parent"][2]), n, min(col["new"][0]), max(col["new"][0]),
                        statistics.median(col["new"][1]), statistics.median(col["new"][2]), n / p, s, "accepted" if ok else "MISS"))
    lines.append("  figures missed: %d of %d" % (missed, len(rounds["parent"][0])))
    return lines, bool(missed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="(child) evaluate with the library COVEST_AMD_LIB selects and dump the arrays here")
    ap.add_argument("--clock", action="store_true", help="(child) one round of the timed calls")
    ap.add_argument("--new")
    ap.add_argument("--parent")
    ap.add_argument("--time", action="store_true", help="after the values, the timed rounds")
    ap.add_argument("--work")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_refactor_ab.txt"))
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
        return 0
    if args.clock:
        clock()
        return 0
    libs = {"new": os.path.abspath(args.new), "parent": os.path.abspath(args.parent)}
    work = args.work or tempfile.mkdtemp(prefix="batch_ab_")
    lines = ["# histogram batches, new library against the parent's (tools/compare_batch_libs.py)"]
    failed = False
    for tag in ("new", "parent"):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        rc = subprocess.run(["timeout", "-k", "10", str(DUMP_LIMIT), sys.executable, os.path.abspath(__file__), "--dump",
                             os.path.join(work, tag)], env=dict(os.environ, COVEST_AMD_LIB=libs[tag])).returncode
        if rc != 0:  # nothing more is started after a child that failed
            lines.append("values: the %s library's run ended with status %d: nothing more was started" % (tag, rc))
            failed = True
            break
    if not failed:
        part, failed = compare(work)
        lines += part
    if args.time and not failed:
        part, failed = time_rounds(libs)
        lines += part
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
