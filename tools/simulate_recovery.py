"""How close one whole estimate lands to the truth when the reads are simulated (covest_amd.simulate): genome ->
reads -> canonical 21-mer histogram -> estimate, basic model, for seeds 1..8 at the settings of tests/sim_recovery.py
(tests/test_gpu_simulate.py::test_estimate_recovers_the_truth runs seed 0 and allows twice the largest deviation recorded
here, under fixed caps).  Truth, estimate and relative deviation per seed and quantity.

    python tools/simulate_recovery.py [--out profiles/simulate_recovery.txt]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from sim_recovery import LOOP, recover  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "simulate_recovery.txt"))
    ap.add_argument("--seeds", default="1-8")
    args = ap.parse_args()
    a, b = (int(x) for x in args.seeds.split("-"))
    lines = ["# estimate against truth from simulated reads: genome %(genome_len)d, L = %(read_len)d, c = %(coverage)g, "
             "e = %(error_rate)g, k = %(k)d canonical, basic model" % LOOP,
             "# %-4s %-18s %14s %14s %10s" % ("seed", "quantity", "truth", "estimate", "rel. dev.")]
    worst = {}
    for seed in range(a, b + 1):
        for q, (truth, est, dev) in recover(seed).items():
            lines.append("  %-4d %-18s %14.8g %14.8g %10.5f" % (seed, q, truth, est, dev))
            worst[q] = max(worst.get(q, 0.0), dev)
    for q, dev in worst.items():
        lines.append("# largest deviation, %-18s %10.5f" % (q, dev))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
