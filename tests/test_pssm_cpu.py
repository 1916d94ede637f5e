"""CPU: the host side of profile (PSSM) queries without a device: the new
entry points' argument checks, the PSSM text format (pssm.read_pssm, and the
same words from `lib/main --pssm`, which checks the file and the flags before
any GPU is touched), and swplan::plan_scoring_pssm on both sides of each
predicate of the scoring envelope (tests/native/pssm_plan_check.cpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")
CSRC = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"
NCBI20 = "ARNDCQEGHILKMFPSTWYV"


def test_null_and_invalid_arguments(sw):
    L = sw.capi.lib()
    rows = np.zeros(50, dtype=np.int8)
    rp = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))
    out = ctypes.c_void_p()
    n = ctypes.c_int32(7)
    assert L.sw_pssm_create(None, rp, 2, ctypes.byref(out)) == -1
    assert "null" in L.sw_last_error().decode()
    assert L.sw_pssm_create(None, rp, 2, None) == -1
    assert L.sw_pssm_create(None, None, -1, ctypes.byref(out)) == -1
    assert L.sw_pssm_free(None) == 0  # as sw_db_free and sw_destroy
    assert L.sw_pssm_length(None, ctypes.byref(n)) == -1 and n.value == 7
    assert L.sw_scan_pssm(None, None, None, 2, 2, None) == -1
    assert L.sw_scan_pssm_device(None, None, None, 2, 2, None) == -1
    assert L.sw_scan_pssm_topk(None, None, None, 2, 2, 5, None) == -1
    assert L.sw_align_pssm(None, None, None, 2, 2, None, 0, None, None, 0) == -1
    assert "null" in L.sw_last_error().decode()
    assert L.sw_version() >= 200


# ---- the text format ----------------------------------------------------------
def write(tmp_path, text, name="p.pssm"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_read_25_columns(sw, tmp_path):
    rng = np.random.default_rng(5)
    want = rng.integers(-100, 101, size=(7, 25)).astype(np.int8)
    text = "# a comment\n\nsome title line 12\n  " + " ".join(LETTERS) + "\n"
    for i, r in enumerate(want):
        text += "%d %s %s trailing 0.5\n" % (i + 1, "ARNDX*W"[i], " ".join(str(int(x)) for x in r))
    rows, cons = sw.pssm.read_pssm(write(tmp_path, text))
    assert rows.dtype == np.int8 and np.array_equal(rows, want) and cons == "ARNDX*W"
    # without positions and letters: the consensus is the best-scoring column
    text = " ".join(LETTERS.lower()) + "\n" + "\n".join(" ".join(str(int(x)) for x in r) for r in want) + "\n"
    rows, cons = sw.pssm.read_pssm(write(tmp_path, text))
    assert np.array_equal(rows, want) and cons == "".join(LETTERS[int(np.argmax(r))] for r in want)
    # positions without letters: one more token than columns
    text = " ".join(LETTERS) + "\n" + "\n".join("%d " % (i + 1) + " ".join(str(int(x)) for x in r)
                                                 for i, r in enumerate(want)) + "\n"
    assert np.array_equal(sw.pssm.read_pssm(write(tmp_path, text))[0], want)
    # write_pssm round-trips
    path = str(tmp_path / "w.pssm")
    sw.pssm.write_pssm(path, want)
    assert np.array_equal(sw.pssm.read_pssm(path)[0], want)


def ncbi_text(scores, cons):
    head = "\nLast position-specific scoring matrix computed, weighted observed percentages rounded down, " \
           "information per position, and relative weight of gapless real matches to pseudocounts\n"
    head += "            " + "   ".join(NCBI20) + "    " + "   ".join(NCBI20) + "\n"
    body = ""
    for i, r in enumerate(scores):
        body += "%5d %s  " % (i + 1, cons[i]) + " ".join("%3d" % int(x) for x in r) + "  " + \
            " ".join("%3d" % (5 * (k % 3)) for k in range(20)) + "  0.55 1.30\n"
    tail = "\n                      K         Lambda\nStandard Ungapped    0.1334     0.3157\n" \
           "Standard Gapped      0.0410     0.2670\nPSI Ungapped         0.1446     0.3166\n"
    return head + body + tail


def test_read_ncbi_layout(sw, tmp_path):
    rng = np.random.default_rng(6)
    sc = rng.integers(-9, 12, size=(11, 20))
    sc[4, 2], sc[4, 3] = -3, -4     # N, D: floor(-7 / 2) = -4
    sc[5, 5], sc[5, 6] = 7, 2       # Q, E: floor(9 / 2) = 4
    rows, cons = sw.pssm.read_pssm(write(tmp_path, ncbi_text(sc, "MKVLAAGIWQD")))
    assert rows.shape == (11, 25) and cons == "MKVLAAGIWQD"
    assert np.array_equal(rows[:, :20], sc)
    B, J, Z, X, STAR = 20, 21, 22, 23, 24
    assert np.array_equal(rows[:, B], (sc[:, 2] + sc[:, 3]) // 2) and rows[4, B] == -4
    assert np.array_equal(rows[:, Z], (sc[:, 5] + sc[:, 6]) // 2) and rows[5, Z] == 4
    assert np.array_equal(rows[:, J], (sc[:, 9] + sc[:, 10]) // 2)
    assert np.array_equal(rows[:, X], sc.min(axis=1)) and np.array_equal(rows[:, STAR], sc.min(axis=1))


def test_read_file_naming_x(sw, tmp_path):
    cols = "ARNDX"
    text = " ".join(cols) + "\n1 A 5 -1 -2 -3 -7\n2 R -1 6 0 -2 9\n"
    rows, cons = sw.pssm.read_pssm(write(tmp_path, text))
    assert cons == "AR" and rows.shape == (2, 25)
    assert rows[0, :4].tolist() == [5, -1, -2, -3] and rows[1, :4].tolist() == [-1, 6, 0, -2]
    B, X = 20, 23
    assert rows[:, B].tolist() == [-3, -1]       # floor((N + D) / 2): named pair
    others = [c for c in range(4, 25) if c != B]
    assert (rows[0, others] == -7).all() and (rows[1, others] == 9).all()   # X, not the minimum


ERRORS = [
    ("1 2 3\n4 5 6\n", "no header"),
    ("# only a comment\n", "no header"),
    ("A R O\n1 A 1 2 3\n", "unknown residue letter"),
    ("A R N\n1 U 1 2 3\n", "unknown residue letter"),
    ("A R N\n1 A 1 2 3\n2 R 1 2\n", "short row"),
    ("A R N\n1 A 1 x 3\n", "bad entry"),
    ("A R N\n1 A 1 2.5 3\n", "bad entry"),
    ("A R N\n1 A 1 101 3\n", "-100..100"),
    ("A R N\n1 A 1 2 -101\n", "-100..100"),
    ("A R N\n", "no rows"),
    ("A R N\nnot a row\n", "no rows"),
]


@pytest.mark.parametrize("text, word", ERRORS)
def test_read_pssm_errors(sw, tmp_path, text, word):
    with pytest.raises(sw.pssm.PSSMError, match=word.replace(".", r"\.")):
        sw.pssm.read_pssm(write(tmp_path, text))


@pytest.mark.parametrize("text, word", ERRORS)
def test_main_pssm_errors(tmp_path, text, word):
    """The same words from the CLI, exit 1, before the database is read or a
    GPU touched (the database path does not exist)."""
    out = subprocess.run([os.path.join(LIB, "main"), "--pssm", write(tmp_path, text), "--db", "/nonexistent/d.fasta"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and word in out.stderr and "--pssm" in out.stderr, out.stderr
    assert out.stdout == ""


def test_main_pssm_flags(tmp_path):
    good = write(tmp_path, "A R N\n1 A 1 2 3\n")
    main = os.path.join(LIB, "main")

    def run(*args):
        return subprocess.run([main] + list(args), capture_output=True, text=True, timeout=60)
    out = run("--pssm", good, "--query", "q.fasta", "--db", "d.fasta")
    assert out.returncode == 1 and "--pssm" in out.stdout
    out = run("--pssm", good, "--db", "d.fasta", "--matrix", "blosum62")
    assert out.returncode == 1 and "--pssm" in out.stderr
    out = run("--db", "d.fasta")                       # neither --pssm nor --query
    assert out.returncode == 1 and "--pssm" in out.stdout and "--query" in out.stdout
    out = run("--pssm", str(tmp_path / "missing.pssm"), "--db", "d.fasta")
    assert out.returncode == 1 and "--pssm" in out.stderr and "cannot open" in out.stderr
    out = run("--pssm", good, "--db", "d.fasta", "--gap-open", "1001")
    assert out.returncode == 1 and "--gap-open" in out.stderr
    out = run("--pssm", good, "--db", "d.fasta", "--topk", "0")
    assert out.returncode == 1 and "--topk" in out.stderr
    out = run("--pssm", good, "--db", "d.fasta", "--gpus", "2")
    assert out.returncode == 1 and "--pssm" in out.stderr


def test_cpp_and_python_parsers_agree(sw, tmp_path):
    """main --pssm accepts what read_pssm accepts: a file both read passes the
    CLI's file check (it then fails on the missing database, not on --pssm)."""
    rng = np.random.default_rng(8)
    path = write(tmp_path, ncbi_text(rng.integers(-9, 12, size=(9, 20)), "ACDEFGHIK"))
    assert sw.pssm.read_pssm(path)[0].shape == (9, 25)
    out = subprocess.run([os.path.join(LIB, "main"), "--pssm", path, "--db", "/nonexistent/d.swdb"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--pssm" not in out.stderr
    assert out.stdout.startswith("Input profile: 9 positions\n")


# ---- planning -------------------------------------------------------------------
@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_plan_scoring_pssm(tmp_path):
    exe = str(tmp_path / "pssm_plan_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I" + CSRC,
                    "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "native", "pssm_plan_check.cpp"),
                    os.path.join(CSRC, "sw_plan.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("pssm_plan_check ok"), r.stdout + r.stderr
    forms = dict(line.split(": ", 1) for line in r.stdout.splitlines() if " | " in line)
    assert forms["pssm-int8-fits-27"].startswith("sw_inter_x2p<48,8,linear,fp16>")
    assert forms["pssm-int8-over-28"].startswith("sw_inter_x2p<32,8,affine,fp16>")
    assert forms["pssm-big-go-975-1"].startswith("sw_inter<32,8,affine> | sw_intra<")
    assert forms["pssm-big-linear-36"].startswith("sw_inter<64,8,linear> | sw_intra<")
    assert forms["pssm-long-wide-221-20"].startswith(" | sw_intra_x2<20>")
