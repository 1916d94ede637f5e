"""CPU: the host half of the iterated profile search (include/sw_amd.h
"iterated profile search"; csrc/sw_pssm_build.cpp, the PSSM writer of
csrc/swsolver.cpp, the flags of csrc/sw_cli.cpp) without a GPU, against the
numpy model in tests/profile_support.py.

Tolerances: lambda is the lower end of a bisection that stops when the
midpoint equals an end, so the library's and the model's roots differ by the
rounding of a 400-term sum in f (a few 1e-16 relative): relative 1e-12 as the
issue sets.  PSSM entries are compared exactly, after asserting that the
model's unrounded values for the test's own inputs keep 1e-6 from every
half-integer (two correct double evaluations differ by ~1e-13 there).

tests/native/profile_check.cpp is sw_pssm_build.cpp's stand-alone program,
built with -fsanitize=address,undefined and run on its own."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import profile_support as ps
import pssm_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd")
CSRC = os.path.join(PKG, "csrc")
MAIN = os.path.join(PKG, "lib", "main")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


@needs_gxx
def test_native_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "profile_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"] + INC +
                   [os.path.join(ROOT, "tests", "native", "profile_check.cpp"), os.path.join(CSRC, "sw_pssm_build.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("profile_check ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_constants_are_mirrored(sw):
    hdr = open(os.path.join(ROOT, "include", "sw_amd.h")).read()
    for name, val in (("MSA_GAP", 25), ("MSA_NONE", 26), ("PROFILE_CODES", 20), ("PROFILE_ONE", 1 << 30),
                      ("PROFILE_MAX_HITS", 4096)):
        assert "#define SW_%s %d" % (name, val) in hdr
        assert getattr(sw.capi, name) == val
    assert (ps.GAP, ps.NONE, ps.CODES, ps.ONE) == (25, 26, 20, 1 << 30)
    assert ctypes.sizeof(sw.capi.IterRound) == 16 + ctypes.sizeof(sw.capi.Calib)
    assert sw.capi.lib().sw_version() >= 700
    # one table, shared: the model's copy is the package's
    assert np.array_equal(ps.FREQ, sw.synth.SWISSPROT_FREQ)


def test_matrix_lambda(sw):
    """BLOSUM62 and the reference's BLOSUM50 against the model (and the values
    the issue records); the default matrix is BLOSUM50-ref."""
    for mid, recorded in ((sw.MATRIX_BLOSUM62, 0.317222482004459), (sw.MATRIX_BLOSUM50_REF, 0.233396012121760)):
        m = sw.capi.builtin_matrix(mid)
        got, want = sw.capi.matrix_lambda(m), ps.matrix_lambda(m)
        print("lambda", mid, repr(got), repr(want))
        assert got == pytest.approx(want, rel=1e-12, abs=0)
        assert got == pytest.approx(recorded, rel=1e-12, abs=0)
        f = (np.outer(ps.background(), ps.background()) * np.exp(got * m[:20, :20].astype(np.float64))).sum()
        assert f == pytest.approx(1.0, abs=1e-12)
    assert sw.capi.matrix_lambda(None) == sw.capi.matrix_lambda(sw.capi.builtin_matrix(sw.MATRIX_BLOSUM50_REF))


def test_matrix_lambda_unsupported(sw):
    L = sw.capi.lib()
    out = ctypes.c_double(-1.0)
    i8p = ctypes.POINTER(ctypes.c_int8)
    positive = np.full(625, 3, dtype=np.int8)
    flat = sw.capi.builtin_matrix(sw.MATRIX_IDENTITY3).copy().reshape(625)
    flat[flat > 0] = 100  # +100 / -3: a positive expectation
    assert ps.matrix_lambda(positive) is None and ps.matrix_lambda(flat) is None
    for m in (positive, flat, np.full(625, -2, dtype=np.int8)):
        assert L.sw_matrix_lambda(m.ctypes.data_as(i8p), ctypes.byref(out)) == -5  # SW_E_UNSUPPORTED
        assert "lambda" in L.sw_last_error().decode()
    assert out.value == -1.0
    assert L.sw_matrix_lambda(positive.ctypes.data_as(i8p), None) == -1
    bad = np.full(625, 101, dtype=np.int8)
    assert L.sw_matrix_lambda(bad.ctypes.data_as(i8p), ctypes.byref(out)) == -1


def random_msa(rng, nrows, qlen, family=True):
    """Rows as an alignment of a family makes them: a master of codes 0..19,
    rows that copy it with substitutions over a span, gaps inside the span,
    NONE outside, a few ambiguity codes."""
    master = rng.integers(0, 20, size=qlen).astype(np.uint8)
    msa = np.full((nrows, qlen), ps.NONE, dtype=np.uint8)
    msa[0] = master
    for r in range(1, nrows):
        a = int(rng.integers(0, qlen))
        b = int(rng.integers(a, qlen)) + 1
        row = master[a:b].copy() if family else rng.integers(0, 20, size=b - a).astype(np.uint8)
        sub = rng.random(b - a) < 0.4
        row[sub] = rng.integers(0, 25, size=int(sub.sum()))
        row[rng.random(b - a) < 0.08] = ps.GAP
        msa[r, a:b] = row
    return msa


@pytest.mark.parametrize("mid", [1, 0])
@pytest.mark.parametrize("shape", [(1, 7), (2, 40), (9, 130), (300, 64), (4097, 33)])
def test_pssm_from_counts_equals_model(sw, mid, shape):
    nrows, qlen = shape
    rng = np.random.default_rng(1000 * nrows + qlen + mid)
    m = sw.capi.builtin_matrix(mid)
    msa = random_msa(rng, nrows, qlen)
    cnt, weight, wsum = ps.tables(msa)
    assert int(wsum.max()) < 2 ** 43
    prior = pssm_support.derived(np.where(msa[0] < 25, msa[0], 0), m)
    for pseudo in (10.0, 0.5, 1000.0):
        want, raw = ps.pssm_from_counts(cnt, wsum, prior, m, pseudo)
        margin = ps.half_margin(raw)
        print("half-integer margin", shape, mid, pseudo, margin)
        assert margin > 1e-6, "the model's own values are too close to a rounding edge for these inputs"
        got = sw.capi.pssm_from_counts(cnt, wsum, prior, m, pseudo)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert np.array_equal(got[:, 20:], prior[:, 20:])


@pytest.mark.parametrize("mid", [0, 1, 2, 3])
def test_one_row_gives_the_derived_table(sw, mid):
    """A profile built from the query alone is the table the query stands for:
    alpha = 0 for the 20 counted codes (the unrounded entry is the matrix's to
    ~2e-15), and the five ambiguity codes are never counted: the prior row."""
    m = sw.capi.builtin_matrix(mid)
    q = np.arange(25, dtype=np.uint8)
    msa = q.reshape(1, 25)
    cnt, weight, wsum = ps.tables(msa)
    assert cnt[:20].sum() == 20 and not cnt[20:].any() and int(weight[0]) == ps.ONE
    want = pssm_support.derived(q, m)
    model, raw = ps.pssm_from_counts(cnt, wsum, want, m)
    assert np.nanmax(np.abs(raw[:20] - m[:20, :20])) < 1e-12
    assert np.array_equal(model, want)
    assert np.array_equal(sw.capi.pssm_from_counts(cnt, wsum, want, m), want)
    # the prior's columns 20..24 are carried, whatever they hold
    other = want.copy()
    other[:, 20:] = 7
    assert np.array_equal(sw.capi.pssm_from_counts(cnt, wsum, other, m)[:20], other[:20])


def test_pseudo_range_and_arguments(sw):
    m = sw.capi.builtin_matrix(1)
    cnt, weight, wsum = ps.tables(np.arange(20, dtype=np.uint8).reshape(1, 20))
    prior = pssm_support.derived(np.arange(20), m)
    for ok in (1e-9, 10, 1000.0):
        sw.capi.pssm_from_counts(cnt, wsum, prior, m, ok)
    for bad in (0.0, -1.0, 1000.0001, float("inf"), float("nan")):
        with pytest.raises(sw.SWError, match="-1.*pseudo"):
            sw.capi.pssm_from_counts(cnt, wsum, prior, m, bad)
    L = sw.capi.lib()
    assert L.sw_pssm_from_counts(None, None, 3, None, None, 10.0, None) == -1
    assert L.sw_pssm_from_counts(None, None, 0, None, None, 10.0, None) == 0  # no position
    assert L.sw_pssm_from_counts(None, None, -1, None, None, 10.0, None) == -1
    with pytest.raises(sw.SWError, match="-5"):
        sw.capi.pssm_from_counts(cnt, wsum, prior, np.full(625, 3, dtype=np.int8))
    # the device entry points check their arguments before any device is touched
    assert L.sw_pssm_rows(None, None) == -1
    assert L.sw_msa_pssm(None, None, None, 2, 2, None, None, 0, None, None) == -1
    assert L.sw_profile_counts(None, None, None, 2, 2, None, None, 0, None, None, None) == -1
    assert L.sw_profile_counts_msa(None, None, 1, 0, None, None, None) == -1
    assert L.sw_pssm_refine(None, None, None, 2, 2, None, None, 10.0, None, 0, None) == -1
    assert L.sw_search_iter(None, None, None, 0, None, 1, 1e-3, 1, 10.0, 1, 1.0, None, None, None, None, None, None,
                            None, None, None, None) == -1


# ---- the PSSM writer (include/sw_solver_ext.h) -------------------------------------
@needs_gxx
def test_writer_and_reader_round_trip(sw, tmp_path):
    """tests/native/pssm_io_check.cpp: write then read is the identity in C++
    (rows and consensus); the package's reader reads the same file."""
    exe = str(tmp_path / "pssm_io_check")
    lib = os.path.join(PKG, "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + INC +
                   [os.path.join(ROOT, "tests", "native", "pssm_io_check.cpp"), os.path.join(CSRC, "swsolver.cpp"),
                    "-L" + lib, "-lswamd", "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("pssm_io_check ok"), r.stdout[-4000:] + r.stderr[-4000:]
    rows, cons = sw.read_pssm(str(tmp_path / "table.pssm"))
    i, c = np.meshgrid(np.arange(60), np.arange(25), indexing="ij")
    assert np.array_equal(rows, ((31 * i + 17 * c) % 201 - 100).astype(np.int8))
    assert cons == "".join("ARNDCQEGHILKMFPSTWYVBJZX*"[k % 25] for k in range(60))


# ---- main's flags: every check is made before a file is read -----------------------
BASE = ["--query", "q.fasta", "--db", "d.fasta"]


@pytest.mark.parametrize("flags, msg", [
    (["--iterations", "3", "--pssm", "p.txt"], "--iterations cannot be combined with --pssm"),
    (["--iterations", "3", "--queries", "qs.fasta", "--topk", "5"], "--iterations cannot be combined with --queries"),
    (["--iterations", "3", "--hits", "5"], "--iterations cannot be combined with --hits"),
    (["--iterations", "3", "--gpus", "2"], "--iterations cannot be combined with --gpus N > 1"),
    (["--iterations", "3", "--make-db", "out.swdb"], "--iterations cannot be combined with --make-db"),
    (["--iterations", "0"], "--iterations must be an integer in 1..1000"),
    (["--iterations", "x"], "--iterations must be an integer in 1..1000"),
    (["--iterations", "2", "--topk", "4097"], "K an integer in 1..4096"),
    (["--iterations", "2", "--inclusion-evalue", "0"], "--inclusion-evalue must be a number > 0"),
    (["--iterations", "2", "--max-evalue", "-1"], "--max-evalue must be a number > 0"),
    (["--inclusion-evalue", "1e-3"], "--inclusion-evalue needs --iterations"),
    (["--write-pssm", "out.pssm"], "--write-pssm needs --iterations"),
    (["--max-evalue", "1"], "--max-evalue needs --rank evalue"),
])
def test_main_iteration_flag_conflicts(flags, msg):
    out = subprocess.run([MAIN] + BASE + flags, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and msg in out.stderr, out.stderr
    assert "Input" not in out.stdout  # no file was read


def test_main_iteration_flags_accepted():
    """--gpus 1 is no conflict, and a well-formed command line gets as far as
    the files (which do not exist)."""
    out = subprocess.run([MAIN] + BASE + ["--iterations", "3", "--gpus", "1", "--inclusion-evalue", "1e-4", "--topk",
                                          "4096", "--max-evalue", "10", "--write-pssm", "o.pssm"],
                         capture_output=True, text=True, timeout=60)
    assert "Input buffer" in out.stdout, out.stderr  # past every flag check: the (missing) query was read
    for flag in ("--iterations", "--inclusion-evalue", "--write-pssm", "--max-evalue", "--topk", "--gpus"):
        assert flag not in out.stderr, out.stderr
