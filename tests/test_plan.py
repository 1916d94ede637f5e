"""The scan-planning policies (csrc/sw_plan.cpp) on the CPU, linked from that
file alone.  tests/native/plan_check.cpp builds the merged launch's work
table (lpt_plan) for C2's 1/8-share shape under both scorings and for edge
mixes (more tri groups than single-wave blocks, tail pairs beside tris,
pipelined pairs at both ends, every pair pipelined, no long subjects) and
checks it against the kernel's decoding of it (sw_inter_x2.hip x2p_wg,
sw_intra_x2.h's pipelined pair ranges): every 64-subject block and every
long-subject pair is scanned by exactly one entry, longest first.  And it
asks scan_plan for the form of scans over synthetic database shapes: the
conditions every plan meets, and the forms whose routing is known; and for
one scoring on each side of every predicate of the scoring that switches
kernel families, through the real plan_scoring on 625-entry matrices."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "plan_check.cpp"),
                    os.path.join(CSRC, "sw_plan.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("plan_check ok"), r.stdout + r.stderr
    return r.stdout


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_lpt_table_covers_every_block_and_pair_once(plan_check):
    # the 1/8 share's tri table: 275 tri workgroups with spare waves, 4 pipelined pairs
    assert "share8-affine-tri: 888 entries, npipe 4, pipe_tail 1561 of 1561 pairs, spares 275" in plan_check
    # linear scans of quad databases pipeline their last 2 % of pairs (to 8)
    assert "share8-linear-tailpipe: 895 entries, npipe 4, pipe_tail 1529 of 1561 pairs" in plan_check


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_scan_plan_forms(plan_check):
    """The forms plan_check.cpp pins, as the names a handle would report."""
    forms = dict(line.split(": ", 1) for line in plan_check.splitlines() if " | " in line)
    # int16-safe scans of the 1/8-share shape take the merged launch; the
    # linear one in 48-row strips from 97 query rows on
    assert forms["share8-affine-q375"].startswith("sw_inter_x2p<32,8,affine,fp16>+tri")
    assert forms["share8-affine-q375"].endswith("+lpt | sw_intra_x2<6> ri 6 ri2 6")
    assert forms["share8-linear-q375"].startswith("sw_inter_x2p<48,8,linear,fp16>")
    assert "+lpt | " in forms["share8-linear-q375"]
    assert forms["share8-linear-q96"].startswith("sw_inter_x2p<32,8,linear,fp16>") and "+lpt | " in forms["share8-linear-q96"]
    assert forms["share8-linear-q97"].startswith("sw_inter_x2p<48,8,linear,fp16>")
    # one pass: no pair form, no merged launch
    assert forms["share8-one-pass"].startswith("sw_inter_x2s<32,8,linear,fp16> | ")
    # the merged launch at 8 rows per lane; without it the cost model's 12
    assert forms["share8-affine-q1400"].endswith("+lpt | sw_intra_x2<8> ri 12 ri2 8")
    assert forms["share8-affine-q1400-lpt0"] == "sw_inter_x2p<32,8,affine,fp16> | sw_intra_x2<12> ri 12 ri2 12"
    assert forms["share8-span5"].startswith("sw_inter_x2p<32,8,linear,fp16>+int16[0,5) | ")
    assert forms["share8-int32-affine"].startswith("sw_inter<32,8,affine> | sw_intra<")
    assert forms["share8-int32-linear"].startswith("sw_inter<64,8,linear> | sw_intra<")
    assert forms["only-long-affine-q1280"].startswith(" | sw_intra_x2<20> ")


def base(name):
    """A kernel name without what depends on the database's shape: the wave
    groups (x2p), the merged launch's strip height and its suffixes."""
    return name.split(">")[0].replace("sw_inter_x2p", "sw_inter_x2s").replace("<48,", "<32,") + ">"


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_scoring_thresholds(plan_check):
    """One row on each side of every predicate of the scoring that switches
    kernel families (plan_scoring on real matrices, then scan_plan), as the
    names a handle reports; tests/test_gpu_scoring_envelope.py asserts the
    same names on the GPU, so a change of routing is made in both places."""
    forms = dict(line.split(": ", 1) for line in plan_check.splitlines() if " | " in line)
    names = {k: tuple(base(x.split(" ri ")[0]) for x in v.split(" | ")) for k, v in forms.items()
             if k.startswith("env-")}
    f16_lin = ("sw_inter_x2s<32,8,linear,fp16>", "sw_intra_x2<4>")
    f16_aff = ("sw_inter_x2s<32,8,affine,fp16>", "sw_intra_x2<4>")
    i32_lin = ("sw_inter<64,8,linear>", "sw_intra<4,linear>")
    i32_aff = ("sw_inter<32,8,affine>", "sw_intra<4,affine>")
    # S + gap = 127 fits the int8 linear profile; 128 runs the affine kernels on a linear gap
    assert names["env-int8-fits-27"] == f16_lin
    assert names["env-int8-over-28"] == f16_aff
    # 2 max S + 27 ge + go: 1023 fp16 / int16, 1024 int32
    assert names["env-big-go-974-1"] == f16_aff and names["env-big-go-975-1"] == i32_aff
    assert names["env-big-ge-191-30"] == f16_aff and names["env-big-ge-192-30"] == i32_aff
    assert names["env-big-linear-35"] == f16_lin and names["env-big-linear-36"] == i32_lin
    assert names["env-non-positive-12-1"] == f16_aff
    assert names["env-limits-1000-1000"] == i32_aff
    # (qlen + 2) (max S + go) = 32,766 is int16-safe, 32,767 needs the guard
    assert names["env-static-32766-guard0"][0] == "sw_inter_x2s<32,8,affine,fp16>"
    assert names["env-static-32767"][0] == "sw_inter_x2s<32,8,affine,fp16>"
    assert names["env-static-32767-guard0"][0] == "sw_inter<32,8,affine>"
    # 20 rows per lane: long subjects only, 2 max S + 39 ge + go below 1024
    assert forms["long-wide-221-20"].startswith(" | sw_intra_x2<20> ")
    assert forms["long-wide-222-20"].startswith(" | sw_intra_x2<10> ")
    assert forms["long-forced20-221-20"].startswith(" | sw_intra_x2<20> ")
    assert forms["long-forced20-222-20"].startswith(" | sw_intra_x2<6> ")
    assert forms["env-forced20-12-1"].endswith(" | sw_intra_x2<6> ri 6 ri2 6")
