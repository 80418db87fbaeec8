"""Build the HIP library in-tree: covest_amd/lib/libcovest_amd.so (gfx950 only).

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container;
the built .so is git-ignored but travels to the GPU box with the repo snapshot.

    python -m covest_amd.build [--force]
"""
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcovest_amd.so")
# (source, extra flags, object name).  K-factored is compiled once per template variant, each into a translation unit
# of its own (csrc/ll_factored.hip, COVEST_FACTORED_VARIANT = the row of csrc/factored_launch.h's table): the HIP runtime
# loads a translation unit's code object when one of its kernels is first launched, so a process only pays for the
# variants it uses.  The finishing kernels and the dispatcher: csrc/ll_factored_launch.hip.
SOURCES = [("host_common.cpp", (), "host_common"), ("tiles_host.cpp", (), "tiles_host"), ("plan_factored.cpp", (), "plan_factored"),
           ("abi_model.cpp", (), "abi_model"), ("abi_grid.cpp", (), "abi_grid"), ("kmer_host.cpp", (), "kmer_host"),
           ("thin_host.cpp", (), "thin_host"), ("abi_tp.cpp", (), "abi_tp"), ("reads_io.cpp", (), "reads_io"), ("ll_direct.hip", (), "ll_direct"),
           ("ll_basic.hip", (), "ll_basic"), ("ll_factored_launch.hip", (), "ll_factored_launch"), ("argmin.hip", (), "argmin"), ("ll_fix.hip", (), "ll_fix"), ("axis_min.hip", (), "axis_min"), ("ll_deriv.hip", (), "ll_deriv"),
           ("kmer_count.hip", (), "kmer_count"), ("kmer_wide.hip", (), "kmer_wide"), ("kmer_bulk.hip", (), "kmer_bulk"), ("thin_hist.hip", (), "thin_hist"),
           ("tp_eval.hip", (), "tp_eval"), ("abi_sim.cpp", (), "abi_sim"), ("sim_reads.hip", (), "sim_reads"),
           ("abi_sample.cpp", (), "abi_sample"), ("sample_reads.hip", (), "sample_reads"),
           ("abi_split.cpp", (), "abi_split"), ("split_reads.hip", (), "split_reads"),
           ("gather_reads.hip", (), "gather_reads"),
           ("abi_dedup.cpp", (), "abi_dedup"), ("dedup_reads.hip", (), "dedup_reads"),
           ("abi_repeat.cpp", (), "abi_repeat"), ("sim_repeats.hip", (), "sim_repeats"),
           ("abi_draw.cpp", (), "abi_draw"), ("draw_hist.hip", (), "draw_hist"),
           ("abi_batch.cpp", (), "abi_batch"), ("ll_batch.hip", (), "ll_batch"),
           ("abi_posterior.cpp", (), "abi_posterior"), ("posterior.hip", (), "posterior"),
           ("abi_lookup.cpp", (), "abi_lookup"), ("kmer_lookup.hip", (), "kmer_lookup"),
           ("abi_join.cpp", (), "abi_join"), ("kmer_join.hip", (), "kmer_join"),
           ("abi_update.cpp", (), "abi_update"),
           ("abi_remove.cpp", (), "abi_remove"), ("kmer_remove.hip", (), "kmer_remove"),
           ("abi_correct.cpp", (), "abi_correct"), ("kmer_correct.hip", (), "kmer_correct"),
           ("abi_influence.cpp", (), "abi_influence"), ("kmer_influence.hip", (), "kmer_influence"),
           ("abi_bootstrap.cpp", (), "abi_bootstrap"), ("bootstrap_weights.hip", (), "bootstrap_weights"),
           ("math_probe.hip", (), "math_probe")]
# (the rows of the table, from the one place that counts them)
FACTORED_VARIANTS = int(re.search(r"kFactoredVariants = (\d+)", open(os.path.join(CSRC, "kernels.h")).read()).group(1))
SOURCES += [("ll_factored.hip", ("-DCOVEST_FACTORED_VARIANT=%d" % v,), "ll_factored_v%d" % v) for v in range(FACTORED_VARIANTS)]
SOURCES += [("ll_basic.hip", ("-DCOVEST_BASIC_VARIANT=%d" % v,), "ll_basic_v%d" % v) for v in range(8)]
MAX_PARALLEL = 8
ARCH = "gfx950"


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "covest_amd.h"))
    deps.append(os.path.abspath(__file__))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra_flags=(), out=None):
    """Compile every HIP source for gfx950 and link the shared library.  `extra_flags` / `out`: an
    experimental variant (e.g. -DCOVEST_EXP_...) linked somewhere else, for A/B runs via COVEST_AMD_LIB."""
    if out is None and not force and not _stale():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, "obj" if out is None else "obj_" + os.path.basename(out))
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = _hipcc()
    common = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
              "-x", "hip"] + list(extra_flags)
    objs = []
    pending = list(SOURCES)
    running = []

    def reap(block_until_below):
        while len(running) >= block_until_below:
            src, p = running.pop(0)
            log, _ = p.communicate()
            if p.returncode != 0:
                for _, q in running:
                    q.kill()
                raise RuntimeError("hipcc failed on %s:\n%s" % (src, log.decode(errors="replace")))
            if verbose and log:
                print(log.decode(errors="replace"))

    for src, flags, name in pending:
        obj = os.path.join(obj_dir, name + ".o")
        cmd = [hipcc] + common + list(flags) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        reap(MAX_PARALLEL)
        running.append((name, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    reap(1)
    target = LIB_PATH if out is None else out
    link = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", target] + objs
    subprocess.check_call(link)
    return target


if __name__ == "__main__":
    # python -m covest_amd.build [--force] [--out path.so -DFLAG ...]
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else None
    flags = [a for a in args if a.startswith("-D") or a.startswith("-m")]
    print(build(force="--force" in args, verbose=out is None, extra_flags=flags, out=out))
