"""Rate of the draw kernel (covest_draw_histograms_device, draw_hist.hip) in draws per second, beside two yardsticks
taking turns with it in the same run:
  random_genome   covest_random_genome_device writing 2 n B bases -- the same number of Philox blocks, the floor on the
                  random-number work;
  torch           torch's own route: torch.searchsorted of torch.rand (float64) against the cdf, then torch.bincount.
Two shapes -- the cells of the trimmed histogram (H10k_rep_trim.hist, its tail cell included) and all 10 001 cells of
H10k_rep.hist, both at the repeat model's defaults -- and, for a modal cell of the usual size, the trimmed histogram at
the point tools/time_hessian.py times (its grid optimum); each at n = 10^8, B = 1 and n = 10^6, B = 100.  HIP events on the stream after a spin-up, the
median of N timed repetitions.  Reported only: there is no bar.

Run in a fresh process; torch is imported first (one HIP runtime a process).

    python tools/time_draw.py [--reps 7] [--out profiles/draw_rate.txt]
    COVEST_AMD_LIB=tools/bin/libcovest_nohot.so python tools/time_draw.py --kernel-only --append --note "COVEST_DRAW_HOT=0"
      (the A/B of the hot-cell counters: python -m covest_amd.build --out tools/bin/libcovest_nohot.so -DCOVEST_DRAW_HOT=0)
"""
import argparse
import os
import statistics
import sys

import torch  # first

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

from bench import load_hist  # noqa: E402
from covest_amd import RepeatsModel, _capi, bootstrap as bs, simulate as sim  # noqa: E402

SEED = 20240701
OPTIMUM = [23.7, 0.0195, 0.56, 0.5, 0.11]  # of H10k_rep_trim (the point tools/time_hessian.py times)
SHAPES = [("H10k_rep_trim", 11192, None), ("H10k_rep", 0, None), ("H10k_rep_trim", 11192, OPTIMUM)]
LOADS = [(10 ** 8, 1), (10 ** 6, 100)]


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "draw_rate.txt"))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_draw.py needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.lib()
    lines = []
    if not args.append:
        lines += ["# draw kernel: 10^9 draws per second, median of %d; %s" % (args.reps, torch.cuda.get_device_name(0)),
                  "# random_genome: 2 n B bases = as many Philox blocks; torch: rand (float64) -> searchsorted -> bincount"]
    lines.append("# %s%-22s %6s %9s %10s %4s %10s %14s %10s %8s %8s"
                 % (args.note + ": " if args.note else "", "cells of", "m", "top cell", "n", "B", "draw Gd/s", "random_genome", "torch",
                    "/genome", "/torch"))
    for hname, tail, point in SHAPES:
        model = RepeatsModel(21, 100, load_hist(hname), tail, max_error=8)
        _, w, _ = bs.model_cells(model, model.defaults if point is None else point)
        model.close()
        m = len(w)
        t = bs.draw_thresholds(w)
        d_t = torch.from_numpy(t.view(np.int64)).to(dev)
        cdf = torch.from_numpy(np.cumsum(w) / np.cumsum(w)[-1]).to(dev)
        for n, B in LOADS:
            out = torch.empty(B * m, dtype=torch.int64, device=dev)
            bases = None if args.kernel_only else torch.empty(2 * n * B, dtype=torch.uint8, device=dev)
            offset = None if args.kernel_only else (torch.arange(B, device=dev, dtype=torch.int64) * m)[:, None]

            def draw():
                bs.draw_histograms_device(d_t.data_ptr(), m, n, B, out.data_ptr(), seed=SEED, stream=stream)

            def genome():
                sim.random_genome_device(bases.data_ptr(), 2 * n * B, SEED, stream=stream)

            def torch_route():
                u = torch.rand((B, n), dtype=torch.float64, device=dev)
                cells = torch.searchsorted(cdf[:m - 1], u, right=True)
                return torch.bincount((cells + offset).reshape(-1), minlength=B * m)

            routes = [("draw", draw)] + ([] if args.kernel_only else [("genome", genome), ("torch", torch_route)])
            for _, fn in routes:  # spin-up: code objects loaded, clocks up, torch's allocator warm
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in routes}
            for _ in range(args.reps):
                for name, fn in routes:
                    ms[name].append(timed_ms(fn))
            assert int(out.sum().item()) == n * B
            rate = {name: n * B / (statistics.median(v) * 1e-3) / 1e9 for name, v in ms.items()}
            g, tr = rate.get("genome", float("nan")), rate.get("torch", float("nan"))
            lines.append("  %-22s %6d %9.3f %10d %4d %10.2f %14.2f %10.2f %8.3f %8.3f"
                         % (hname + (" @optimum" if point else " @defaults"), m, float(np.max(w) / np.cumsum(w)[-1]), n, B,
                            rate["draw"], g, tr, rate["draw"] / g, rate["draw"] / tr))
            print(lines[-1], flush=True)
            del out, bases
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
