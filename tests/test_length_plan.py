"""The host units at length, on the CPU (tests/native/length_check.cpp):
planning (csrc/sw_plan.cpp), packing (csrc/sw_pack.cpp) and calibration
(csrc/sw_calib.cpp) for the giants of tests/length_support.py in the lane
layout, the long layout, the library's own split and the split at 3,000, for
one subject of 2^30 residues beside them (offsets only) and for queries of
568 to 65,544 and 2^24 rows.  The program is built with
-fsanitize=undefined,signed-integer-overflow -fno-sanitize-recover on the host
side, so it ends at the first int that overflows on the way to a count; it is a
program of its own, run here and nowhere else.  It found two: lpt_plan's
estimate (length + 63) x chunks in int, which overflows from the second chunk
of a 2^30-residue subject on (and at 70,001 residues from 30,652 chunks on),
and rank_table's int32 loop counter, which never ends at max_len =
INT32_MAX (fixed without a case: the table would take 8 GiB)."""
import os
import shutil
import subprocess

import pytest

import length_support as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@pytest.fixture(scope="module")
def length_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("length")
    exe, lengths = str(tmp / "length_check"), str(tmp / "lengths.txt")
    with open(lengths, "w") as f:
        f.write(" ".join(str(len(s)) for s in ls.giants().subs) + "\n")
    san = ["-Xarch_host", "-fsanitize=undefined,signed-integer-overflow", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall"] + san +
                   ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "length_check.cpp")] +
                   [os.path.join(CSRC, f) for f in ("sw_plan.cpp", "sw_pack.cpp", "sw_calib.cpp")] +
                   ["-o", exe, "-lpthread"], check=True, timeout=300)
    r = subprocess.run([exe, lengths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("length_check ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stdout + r.stderr
    return dict(line.split(": ", 1) for line in r.stdout.splitlines() if ": " in line)


def test_layouts(length_check):
    """The layouts the GPU module scans: one 64-lane block 70,016 columns wide;
    everything long; the library's own threshold
    (64: a small database of long subjects); the giants alone long."""
    assert length_check["lanes"] == "threshold 100000, 0 long, 1 blocks, widest 4376 groups"
    assert 4376 * 16 == 70016
    assert length_check["long"] == "threshold 1, 64 long, 0 blocks, widest 0 groups"
    assert length_check["own"].startswith("threshold 64, ")
    assert length_check["split"].startswith("threshold 3000, 7 long, 1 blocks, ")
    assert length_check["huge-lanes"] == "threshold 1073741824, 0 long, 2 blocks, widest 67108864 groups"
    assert length_check["pack-lanes"] == "n 64, 0 long (0 bytes), 1 blocks (%d bytes)" % (70016 * 64)
    assert length_check["pack-long"].startswith("n 64, 64 long (")


def test_kernel_names(length_check):
    """scan_plan's names for G: tests/test_gpu_lengths.py asserts the same."""
    for (layout, sc, qlen), names in ls.NAMES.items():
        line = length_check["%s-%s-q%d" % (layout, sc, qlen)]
        assert line.split(" ri ")[0] == "%s | %s" % (names[0] or "", names[1]), (layout, sc, qlen, line)
    # the longest queries and the 2^30-residue subject plan too, guarded
    for layout in ("lanes", "long", "own", "split", "huge-long", "huge-own", "huge-split-merged", "huge-lanes"):
        for sc in ls.SCORING_NAMES:
            for qlen in (65544, 1 << 24):
                assert "%s-%s-q%d" % (layout, sc, qlen) in length_check


def test_groups(length_check):
    """One hit of a 65,544-row query is over sw_align's direction budget: 64
    hits, 64 groups; the 2^30-residue subject's boundary row (36 GB) is a
    hit-table group of its own, between the group before and the group after."""
    assert length_check["lanes-q65544"] == "align groups 64"     # (the later of the two lines)
    assert length_check["huge-own-q65544"] == "align groups 65"
    assert length_check["huge-own-q568"] == "align groups 3"


def test_calibration(length_check):
    # 70,001 = 2^16 x 1.07: bin 64; 2^30: bin 120; INT32_MAX: bin 123, the last one used
    assert length_check["calibration"].startswith("bins 64 120 123, ")
