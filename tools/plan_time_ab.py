"""What a change to K-factored's planner (plan_factored.cpp) did to the host time of building a plan: bench.py's `og`
workload (optimize_grid: a plan per iteration) and the `grid` row of tools/time_host.py for c3 (handle creation with its
plan), two libraries alternating, a fresh process each, `rounds` times each -- as tools/latency.py --ab.

    python tools/plan_time_ab.py NEW.so PARENT.so [--rounds 5] [--out profiles/plan_time_ab.txt]

Per row both medians and spreads (max - min over the rounds).  A row is marked when the new median exceeds the parent's
by more than the parent's own spread in this same run, and the exit status says whether any is.
"""
import argparse
import ast
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_process(lib):
    """{row: value} of one bench.py --workload og and one tools/time_host.py under `lib`; None if a child failed."""
    env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
    rows = {}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--workload", "og", "--steps", "5", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        return None
    result = json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])
    for case in result["cases"]:
        label = case["histogram"].split(" ")[0]
        rows["og %s: search, ms" % label] = 1e3 * case["time_to_argmin_s"]
        rows["og %s: handle and plan, us an iteration" % label] = 1e3 * case["split_ms"]["grid_handle_and_plan"] / case["iterations"]
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "time_host.py")], env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        return None
    for line in p.stdout.splitlines():
        if line.startswith("c3 "):
            rows["time_host c3: grid, ms"] = ast.literal_eval(line[line.index("{"):line.index("}") + 1])["grid"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("new")
    ap.add_argument("parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plan_time_ab.txt"))
    args = ap.parse_args()
    got = {"new": {}, "parent": {}}
    for r in range(args.rounds):
        for tag, lib in (("parent", args.parent), ("new", args.new)):
            rows = one_process(lib)
            if rows is None:  # nothing more is started after a child that failed
                print("round %d: a run of the %s library failed" % (r, tag))
                return 2
            for k, v in rows.items():
                got[tag].setdefault(k, []).append(v)
            print("round %d %s done" % (r, tag), flush=True)
    lines = ["# median and spread (max - min) of %d fresh processes each, parent and new alternating (tools/plan_time_ab.py)" % args.rounds,
             "%-48s %10s %8s %10s %8s  %s" % ("row", "parent", "spread", "new", "spread", "new - parent")]
    slower = 0
    for key in got["parent"]:
        a, b = got["parent"][key], got["new"][key]
        ma, mb, sa, sb = statistics.median(a), statistics.median(b), max(a) - min(a), max(b) - min(b)
        over = mb > ma + sa
        slower += over
        lines.append("%-48s %10.3f %8.3f %10.3f %8.3f  %+8.3f%s" % (key, ma, sa, mb, sb, mb - ma,
                                                                     "  BEYOND the parent's spread" if over else ""))
    lines.append("rows whose new median exceeds the parent's by more than the parent's spread: %d" % slower)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
