"""The generators' shared layer without a device: tests/tile_image_check.cpp -- a program of its
own over covest_amd/csrc/tile_image.h and sim_philox.h -- built with the host compiler under the address and
undefined-behaviour sanitizers, and run.  It walks the store step's rule over every alignment of the caller's buffer
and the sizes around each tile boundary, and checks the stream helpers and the base code against their definitions."""
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


def test_tile_image_stream_and_base_code_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tile_image_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "tile_image_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
