"""swplan::short_rows (csrc/sw_plan.cpp), the rows per strip of a query's last
pass in the two-strips inter kernels, checked on the CPU by
tests/native/short_rows_check.cpp for every query length up to four passes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_short_rows(tmp_path):
    exe = str(tmp_path / "short_rows_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "short_rows_check.cpp"),
                    os.path.join(CSRC, "sw_plan.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("short_rows_check ok"), r.stdout + r.stderr
