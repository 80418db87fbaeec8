"""The partitioned k-mer counter's arithmetic without a device (DESIGN.md sections 6q, 6ad): two programs of their own,
built with the host compiler under the address and undefined-behaviour sanitizers, and run.
tests/kmer_plan_check.cpp, over covest_amd/csrc/kmer_plan.h, pins the plans of a dozen inputs worked out by hand, the sizes
that follow from pass 0, the tables' sizes against the comparison in double they replace, and walks both launch cuts over
the totals around each multiple of a launch: at small sizes a mistake there loses or double-counts windows silently.
tests/kmer_stages_check.cpp, over kmer_codes.h and kmer_runs.h, checks what the kernels compute in integers: the length of
a run from the waves' masks against a walk over the tile's 256 threads, the pieces of a run, the pair reversals against
the base-by-base loops, the LDS tables' slot, the table paths' launch cuts, and the walk over the launches of a wave a read
(for_each_wave_launch: first read, first byte and workgroups of every launch)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "covest_amd", "csrc")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = shutil.which(name) if name else None
        if exe:
            return exe
    return None


def _build_and_run(tmp_path, name, says):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, name + ".cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and says in run.stdout, run.stdout + run.stderr


def test_kmer_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "kmer_plan_check", "kmer_plan ok")


def test_kmer_stages_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "kmer_stages_check", "kmer_stages ok")
