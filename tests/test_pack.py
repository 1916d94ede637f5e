"""The packed database layout (csrc/sw_pack.cpp) on the CPU, linked from that
file alone.  tests/native/pack_check.cpp plans and fills small databases
(0 to 129 subjects; lengths around the 8- and 16-column edges; all empty,
all long, none long; equal lengths under shuffled ids; custom ids; every
residue code) and decodes the bytes with the kernels' addressing: every
subject is in exactly one lane or long slot with its residues, every other
byte is the pad, blk_off / blk_groups / blk_cols / blk_res / loff / llen /
lane_ids / lane_len and the totals agree with a recount, and the order is
longest first and stable, under either branch of length_order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack") / "pack_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "pack_check.cpp"),
                    os.path.join(CSRC, "sw_pack.cpp"), "-o", exe, "-lpthread"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("pack_check ok"), r.stdout + r.stderr
    return r.stdout


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_layout_decodes_to_the_subjects(pack_check):
    lines = dict(line.split(": ", 1) for line in pack_check.splitlines() if ": " in line)
    # 129 subjects walk the 12 edge lengths (10 rounds and 9 more); at
    # threshold 9 the 7 lengths 15 .. 40 are long, 70 + 5 subjects of 64
    # bytes each, and the 54 others fill one block as wide as the longest, 9
    assert lines["mixed-n129-t9"] == "n 129, 75 long (4800 bytes), 1 blocks (1024 bytes)"
    # 65 short subjects: a block three groups wide (40 columns) and a block
    # of the shortest subject alone, which is empty: zero groups
    assert lines["mixed-n65-no-long"] == "n 65, 0 long (0 bytes), 2 blocks (3072 bytes)"
    assert lines["mixed-n64-all-long"] == "n 64, 64 long (4096 bytes), 0 blocks (0 bytes)"
    assert lines["mixed-n0-t9"] == "n 0, 0 long (0 bytes), 0 blocks (0 bytes)"
    # a block of zero groups
    assert lines["all-empty"] == "n 70, 0 long (0 bytes), 2 blocks (0 bytes)"
    # a length equal to the threshold is short
    assert lines["one-at-threshold"] == "n 3, 1 long (64 bytes), 1 blocks (1024 bytes)"
    for name in ("equal-lengths-shuffled-ids", "custom-ids", "all-codes"):
        assert name in lines


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_both_sorts_give_one_order(pack_check):
    assert "stable-sort-branch: 129 subjects, same order" in pack_check
