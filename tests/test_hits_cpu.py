"""CPU: the hit table's pure pieces.  tests/native/hits_check.cpp runs the
carried-tuple rules the kernel runs per cell (csrc/sw_hits_rules.h) as a
scalar pass and compares every field with the row the oracle's traceback
(oracle/sw_oracle.c swo_align_linear / swo_align_affine) implies, on random
and tie-heavy pairs over 2 to 4 codes under six scorings, and on pairs over
all 25 codes under six asymmetric scorings at the envelope's edges; injects
three faults that each must be noticed; recovers every subject's residues from its
location (swpack::locate + swk::hit_residue_at) in the bytes the packer
writes; and checks the scratch size and the grouping of hits, the hit
table's and sw_align's.  The CLI's
--hits checks run before any file is read, so they need no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
LIB = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def hits_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hits")
    inc = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
    objs = [str(tmp / "sw_oracle.o")]
    subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-c", os.path.join(ROOT, "oracle", "sw_oracle.c"), "-o", objs[0]],
                   check=True, timeout=300)
    for src in (os.path.join(ROOT, "tests", "native", "hits_check.cpp"), os.path.join(CSRC, "sw_pack.cpp"),
                os.path.join(CSRC, "sw_plan.cpp")):
        objs.append(str(tmp / (os.path.basename(src) + ".o")))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall"] + inc + ["-c", src, "-o", objs[-1]],
                       check=True, timeout=300)
    exe = str(tmp / "hits_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950"] + objs + ["-o", exe, "-lpthread"], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("hits_check ok"), r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


needs_hipcc = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")


@needs_hipcc
def test_carried_tuples_equal_the_oracles_traceback(hits_check):
    m = re.search(r"rules: (\d+) pairs, (\d+) gapped, (\d+) adjacent-runs, (\d+) score-0, faults caught (\d+) (\d+) (\d+)",
                  hits_check)
    assert m, hits_check
    pairs, gapped, adjacent, zero, f1, f2, f3 = map(int, m.groups())
    assert pairs >= 2000 and 3 * gapped >= pairs and adjacent > 0 and zero > 0
    # a last op dropped at a source change, a begin cell from the losing source
    # of a tie, positives counted on entries >= 0: each changes some row
    assert f1 > 0 and f2 > 0 and f3 > 0


@needs_hipcc
def test_carried_tuples_over_all_25_codes(hits_check):
    """The same pass over all 25 codes, sequences up to 200 residues, under
    matrices that are not symmetric (checked natively): entries to +-100, gaps
    of 1 to 1000, an open below the extend, diagonal entries <= 0.  The three
    faults are noticed on these pairs alone."""
    m = re.search(r"rules25: (\d+) pairs, (\d+) gapped, (\d+) adjacent-runs, (\d+) score-0, faults caught (\d+) (\d+) (\d+)",
                  hits_check)
    assert m, hits_check
    pairs, gapped, adjacent, zero, f1, f2, f3 = map(int, m.groups())
    assert pairs >= 1500 and 3 * gapped >= pairs and adjacent > 0
    assert f1 > 0 and f2 > 0 and f3 > 0
    m = re.search(r"rules25-counts: (\d+) identities-over-positives, (\d+) positives-over-identities, (\d+) over-16-bits",
                  hits_check)
    assert m, hits_check
    id_over_pos, pos_over_id, big = map(int, m.groups())
    assert id_over_pos >= 10 and pos_over_id >= 10 and big == 0  # (200 x 100 < 2^15: the GPU test has the large scores)


@needs_hipcc
def test_every_subject_is_read_back_from_its_location(hits_check):
    lines = dict(line.split(": ", 1) for line in hits_check.splitlines() if line.startswith("location-"))
    assert len(lines) == 30  # 0, 1, 63, 64, 65, 129 subjects x five thresholds
    for n in (0, 1, 63, 64, 65, 129):
        for t in ("all-long", "t16", "t64", "none-long", "default"):
            assert lines["location-n%d-%s" % (n, t)].startswith("%d recovered" % n)
    assert lines["location-n129-none-long"] == "129 recovered, 0 long, 3 blocks"
    # threshold 0: every subject but the empty ones (11 of 129) is long
    assert lines["location-n129-all-long"] == "129 recovered, 118 long, 1 blocks"
    assert lines["location-n129-t64"] == "129 recovered, 21 long, 2 blocks"


@needs_hipcc
def test_scratch_and_groups(hits_check):
    assert "groups: 64 bytes per column" in hits_check


@needs_hipcc
def test_align_groups(hits_check):
    """swplan::align_groups (sw_align's launches): tiling, budget, greedy
    maximality and the exact fit are CHECKed natively; a query of 16,383
    against subjects of 16,385, 16,385 and 100 residues makes two launches at
    the default budget (tests/test_gpu_align_rules.py runs that call)."""
    assert "align_groups: budget %d, three-hit ends 1 3\n" % (1 << 30) in hits_check


@needs_hipcc
def test_chunk_rows_constant_is_mirrored(hits_check):
    import sys
    sys.path.insert(0, ROOT)
    import _swpkg
    sw = _swpkg.load()
    assert "chunk_rows: %d\n" % sw.capi.HITS_CHUNK_ROWS in hits_check
    assert "rows_per_lane: %d\n" % sw.capi.HITS_ROWS_PER_LANE in hits_check
    assert "waves: %d\n" % sw.capi.HITS_WAVES in hits_check
    assert sw.capi.HITS_CHUNK_ROWS == 64 * sw.capi.HITS_WAVES * sw.capi.HITS_ROWS_PER_LANE


@pytest.mark.parametrize("flags", [["--hits", "0"], ["--hits", "5000"], ["--hits", "5", "--topk", "5"],
                                   ["--hits", "5", "--pssm", "x"], ["--hits", "5", "--gpus", "2"], ["--hits", "x"]])
def test_cli_rejects_bad_hits_flags(flags):
    """Exit 1 with a message naming --hits, before any file is read (the
    files named here do not exist)."""
    out = subprocess.run([os.path.join(LIB, "main"), "--query", "/nonexistent/q.fasta", "--db", "/nonexistent/db.fasta"]
                         + flags, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--hits" in out.stderr, (out.stdout, out.stderr)


def test_cli_usage_lists_hits():
    out = subprocess.run([os.path.join(LIB, "main"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--hits" in out.stdout
