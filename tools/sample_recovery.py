"""How close one whole estimate lands to the truth when the simulated reads went through the sampler
(covest_amd.sample): genome -> reads at c = 40 -> sample at factor 2 -> canonical 21-mer histogram -> estimate, basic
model, for seeds 1..8 at the settings of tests/sample_recovery.py, against the SAMPLE's truth
(tests/test_gpu_sample.py::test_estimate_recovers_the_samples_truth runs seed 0 and allows twice the largest deviation
recorded here, under fixed caps).

    python tools/sample_recovery.py [--out profiles/sample_recovery.txt]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from sample_recovery import COVERAGE, FACTOR, recover  # noqa: E402
from sim_recovery import LOOP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_recovery.txt"))
    ap.add_argument("--seeds", default="1-8")
    args = ap.parse_args()
    a, b = (int(x) for x in args.seeds.split("-"))
    lines = ["# estimate against the sample's truth: genome %d, L = %d, c = %g sampled at factor %g, e = %g, k = %d "
             "canonical, basic model" % (LOOP["genome_len"], LOOP["read_len"], COVERAGE, FACTOR, LOOP["error_rate"], LOOP["k"]),
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
