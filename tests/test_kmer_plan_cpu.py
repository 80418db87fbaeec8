"""The partitioned k-mer counter's arithmetic without a device: tests/kmer_plan_check.cpp -- a
program of its own over covest_amd/csrc/kmer_plan.h -- built with the host compiler under the address and
undefined-behaviour sanitizers, and run.  It pins the plans of a dozen inputs worked out by hand, the sizes that follow
from pass 0, the tables' sizes against the comparison in double they replace, and walks both launch cuts over the totals
around each multiple of a launch: at small sizes a mistake there loses or double-counts windows silently."""
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


def test_kmer_plan_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "kmer_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "kmer_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "kmer_plan ok" in run.stdout, run.stdout + run.stderr
