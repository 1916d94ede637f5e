"""CPU: the CLI's pure front (csrc/sw_cli.cpp: the flag table, parse and
validate) against tests/golden/cli_flag_cases.json, what the main that checked
its flags inline answered to every subset of up to three of 19 flags before it
touched the library.  tests/native/cli_opts_check.cpp walks the file; it is
built with g++ from sw_cli.cpp alone: no library, no include/ directory, no
GPU runtime."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_flag_cases.json")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_flags_are_answered_as_recorded(tmp_path):
    exe = str(tmp_path / "cli_opts_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "native", "cli_opts_check.cpp"), os.path.join(CSRC, "sw_cli.cpp"),
                    "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("cli_opts_check ok"), r.stdout[-4000:] + r.stderr
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    # the program saw every case of the file, and the file is the recording: 1160 subsets less the few
    # (a query to scan, a database to write) that reach the library
    assert len(cases) > 1100 and ("cases %d:" % len(cases)) in r.stdout, r.stdout[-400:]
    assert all(c["code"] == 1 for c in cases)
