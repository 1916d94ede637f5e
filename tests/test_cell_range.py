"""swplan::cell_range (csrc/sw_plan.cpp): the constants of the inter scan's
biased cell, whose 16-bit halves are unsigned integers added by 32-bit integer
ops and compared as fp16.  For each scheme the patterns must stay positive
normal fp16 values, 0x0400 .. 0x7BFF: the lowest one an addition or a maximum
can read, and the highest one of a lane below the guard.  Checked on the CPU
through tests/native/cell_range_check.cpp, linked from sw_plan.cpp alone."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# name: (matrix min, matrix max, gap open, gap extend)
SCHEMES = {
    "blosum62-12-1": (-4, 11, 12, 1),
    "blosum50-linear-2": (-5, 15, 2, 2),
    "blosum62-13-3": (-4, 11, 13, 3),
    # the largest admissible scheme: 2 max S + 27 ge + go = 1023, the API's most negative entry
    "admissible-extreme": (-100, 100, 67, 28),
    # open below extend: go - ge is negative, its dword is -(2^16 + 1)
    "open-below-extend": (-9, 13, 5, 6),
}
LINE = re.compile(r"min_s (-?\d+) max_s (-?\d+) go (\d+) ge (\d+): z (\d+) sat_limit (-?\d+) lowest (-?\d+) "
                  r"guard (-?\d+) top (-?\d+) gog ([0-9a-f]{8}) diff ([0-9a-f]{8}) ([0-9a-f]{8}) ([0-9a-f]{8}) step((?: [0-9a-f]{8}){32})$")


@pytest.fixture(scope="module")
def ranges(tmp_path_factory):
    if shutil.which(HIPCC) is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("cell") / "cell_range_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "cell_range_check.cpp"),
                    os.path.join(CSRC, "sw_plan.cpp"), "-o", exe], check=True, timeout=300)
    args = [str(v) for s in SCHEMES.values() for v in s]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cell_range_check ok (cell 1024..31743)" in r.stdout, r.stdout + r.stderr
    out = {}
    for name, line in zip(SCHEMES, r.stdout.splitlines()):
        m = LINE.match(line)
        assert m, line
        g = m.groups()
        assert tuple(int(x) for x in g[:4]) == SCHEMES[name]
        out[name] = dict(z=int(g[4]), sat_limit=int(g[5]), lowest=int(g[6]), guard=int(g[7]), top=int(g[8]),
                         gog=int(g[9], 16), diff=[int(x, 16) for x in g[10:13]], step=[int(x, 16) for x in g[13].split()])
    return out


def test_extreme_is_the_admission_bound():
    mn, mx, go, ge = SCHEMES["admissible-extreme"]
    assert 2 * mx + 27 * ge + go == 1023 and mn == -100


@pytest.mark.parametrize("name", list(SCHEMES))
def test_cell_range(ranges, name):
    mn, mx, go, ge = SCHEMES[name]
    c = ranges[name]
    z = c["z"]
    # the figures themselves, from the bounds DESIGN §4 states
    assert c["sat_limit"] == 4096 - 28 * ge - 2 * mx
    assert c["lowest"] == z - go - 27 * ge - 2 * max(mx, -mn)
    assert c["guard"] == z + c["sat_limit"]
    assert c["top"] == c["guard"] + 2 * mx + 26 * ge
    # the lowest reachable pattern is a normal fp16 value
    assert c["lowest"] >= 0x0400, c
    # guard + 2 max S + the largest bias stays finite
    assert c["top"] <= 0x7BFF, c
    # every table entry has its two halves equal, and is the value it stands for
    for j, s in enumerate(c["step"]):
        assert s >> 16 == s & 0xffff == j * ge + z, (j, hex(s))
        assert 0x0400 <= (s & 0xffff) <= 0x7BFF
    for s, want in zip(c["diff"], (4 * ge, 8 * ge, 16 * ge)):
        assert s >> 16 == s & 0xffff == want, (hex(s), want)
    # subtracting the dword takes go - ge off both halves, whatever its sign
    assert c["gog"] == (go - ge) * 0x00010001 % 2 ** 32, hex(c["gog"])
    both = 0x30003000
    assert (both - c["gog"]) % 2 ** 32 == (0x3000 - (go - ge)) * 0x00010001
