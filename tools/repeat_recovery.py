"""How close one whole estimate of the repeat model lands to the truth when genome and reads are simulated
(covest_amd.simulate): repeat genome -> reads -> forward-strand 21-mer histogram -> estimate, repeats model, for seeds
1..8 at the settings of tests/repeat_recovery.py (tests/test_gpu_repeat.py::test_estimate_recovers_the_repeat_truth runs
seed 0 and allows twice the largest deviation recorded here, under fixed caps).  Truth, estimate and deviation per seed
and quantity: relative for coverage, error rate and genome size, absolute for q1, q2 and q.

    python tools/repeat_recovery.py [--out profiles/repeat_recovery.txt]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from repeat_recovery import LOOP, RELATIVE, recover  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "repeat_recovery.txt"))
    ap.add_argument("--seeds", default="1-8")
    args = ap.parse_args()
    a, b = (int(x) for x in args.seeds.split("-"))
    lines = ["# estimate against truth from simulated reads of a repeat genome: genome %(genome_len)d, unit_len %(unit_len)d, "
             "(q1, q2, q) = (%(q1)g, %(q2)g, %(q)g), divergence %(divergence)g, L = %(read_len)d, c = %(coverage)g, "
             "e = %(error_rate)g, k = %(k)d forward strand, repeats model" % LOOP,
             "# deviation: relative for %s; absolute for q1, q2, q" % ", ".join(RELATIVE),
             "# %-4s %-18s %14s %14s %10s" % ("seed", "quantity", "truth", "estimate", "deviation")]
    worst = {}
    for seed in range(a, b + 1):
        for name, (truth, est, dev) in recover(seed).items():
            lines.append("  %-4d %-18s %14.8g %14.8g %10.5f" % (seed, name, truth, est, dev))
            worst[name] = max(worst.get(name, 0.0), dev)
    for name, dev in worst.items():
        lines.append("# largest deviation, %-18s %10.5f" % (name, dev))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
