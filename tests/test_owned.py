"""The owner template behind every HIP resource of the host driver
(csrc/sw_owned.h) on the CPU: tests/native/owned_check.cpp instantiates it
with a counting release function (no HIP) and checks that each owned value
is released exactly once across moves, reset(), release(), self-assignment
and a vector that reallocates and erases its front element."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_owner_releases_each_value_once(tmp_path):
    exe = str(tmp_path / "owned_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "owned_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("owned_check ok"), r.stdout + r.stderr
