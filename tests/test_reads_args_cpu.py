"""The argument checks the entry points over packed reads share, without a device:
tests/reads_args_check.cpp -- a program of its own over covest_amd/csrc/reads_args.h -- built with the host compiler
under the address and undefined-behaviour sanitizers, and run.  It walks each check at its boundary (the 64-bit reach
of first_read + n_reads and of n_reads * read_len, offsets that stay, descend or start below zero, output offsets
given or not) and asserts the status and the exact text of the message."""
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


def test_reads_args_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "reads_args_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "reads_args_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
