"""The FASTA / FASTQ parser without a device and without the reader's handle:
tests/reads_parse_check.cpp -- a program of its own over covest_amd/csrc/reads_parse.h -- built with the host compiler
under the address and undefined-behaviour sanitizers, and run.  Every input lies in a heap block of exactly its length,
so a read one byte past the end is a report (a file mapping would hide it).  Each input is parsed whole, cut by cut_span
for 1, 3 and 16 threads and batches of 1, 1000 and 2^22 bases, and -- FASTQ -- by the general grammar; reads, lengths,
batch ends and verdicts are compared with what stands beside the input, and every cut parse with the whole one."""
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


def test_reads_parse_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "reads_parse_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "reads_parse_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "reads_parse_check ok" in run.stdout, run.stdout + run.stderr
