"""CPU: the ranking by E-value's host half (include/sw_amd.h "ranking by
E-value"; csrc/sw_calib.cpp rank_table, rank_min; csrc/sw_plan.cpp
ranked_groups) and the CLI's flag checks, without a GPU.

Tolerances (from the definitions, not from the code under test): adj[L] is
llround(4096 c ln L), so two `log` implementations can differ by 1 at a
rounding tie: +-1 against numpy.  The cutoff is applied to an integer r at
1/4096 of a score unit: r and r_min together carry under 2/4096 of a score
unit of rounding, under 1e-4 in z for any sigma >= 5 and 1.3e-4 in ln E; the
issue's 1e-3 either side of max_evalue holds with room.

tests/native/rank_check.cpp is the stand-alone program of the same functions,
built with -fsanitize=address,undefined and run on its own."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import rank_support as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
LIB = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


def calib(sw, a=19.6, c=4.13, sigma=6.2, n_db=570000, status=0, qlen=300):
    k = sw.capi.Calib()
    k.size, k.status, k.qlen, k.fits = ctypes.sizeof(sw.capi.Calib), status, qlen, 2
    k.n_db = k.n_fit = n_db
    k.a, k.c, k.sigma = a, c, sigma
    return k


@needs_gxx
def test_native_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rank_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"] + INC +
                   [os.path.join(ROOT, "tests", "native", "rank_check.cpp"), os.path.join(CSRC, "sw_calib.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("rank_check ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_constants_are_mirrored(sw):
    hdr = open(os.path.join(ROOT, "include", "sw_amd.h")).read()
    assert "#define SW_RANK_SCALE 4096\n" in hdr
    assert "#define SW_RANK_FLOOR (-4294967295LL)" in hdr and "#define SW_RANK_NONE 4294967296LL" in hdr
    assert (sw.capi.RANK_SCALE, sw.capi.RANK_FLOOR, sw.capi.RANK_NONE) == (rs.SCALE, rs.R_FLOOR, rs.R_NONE)
    assert rs.R_FLOOR == -2 ** 32 + 1 and rs.R_CEIL == rs.R_NONE - 1
    assert sw.capi.lib().sw_version() >= 600


def test_adj_table(sw):
    """Against llround(4096 c ln L) recomputed in numpy within +-1; exact 0 at
    L = 0, 1; monotone for c > 0; zeros when degenerate; int32 saturation."""
    max_len = 36000
    for c in (4.13, 0.37, 11.0):
        adj = sw.capi.sig_rank_table(calib(sw, c=c), max_len)
        assert adj.dtype == np.int32 and len(adj) == max_len + 1
        assert adj[0] == 0 and adj[1] == 0
        want = np.rint(4096.0 * c * np.log(np.arange(1, max_len + 1, dtype=np.float64))).astype(np.int64)
        assert np.abs(adj[1:].astype(np.int64) - want).max() <= 1
        assert np.all(np.diff(adj[1:].astype(np.int64)) >= 0)
    neg = sw.capi.sig_rank_table(calib(sw, c=-2.5), 1000)
    assert neg[0] == 0 and neg[1] == 0 and np.all(np.diff(neg[1:].astype(np.int64)) <= 0) and neg[1000] < 0
    assert not sw.capi.sig_rank_table(calib(sw, status=sw.capi.CALIB_DEGENERATE), 500).any()
    assert not sw.capi.sig_rank_table(calib(sw, sigma=0.0), 500).any()
    assert sw.capi.sig_rank_table(calib(sw), 0).tolist() == [0]
    up = sw.capi.sig_rank_table(calib(sw, c=1e6), 100)
    down = sw.capi.sig_rank_table(calib(sw, c=-1e6), 100)
    assert up[0] == up[1] == 0 and np.all(up[2:] == 2 ** 31 - 1)
    assert down[0] == down[1] == 0 and np.all(down[2:] == -2 ** 31)


def test_rank_min_special_cases(sw):
    cal = calib(sw)
    assert sw.capi.sig_rank_min(cal, None) == rs.R_FLOOR
    assert sw.capi.sig_rank_min(cal, float("inf")) == rs.R_FLOOR
    assert sw.capi.sig_rank_min(cal, 570000) == rs.R_FLOOR and sw.capi.sig_rank_min(cal, 1e7) == rs.R_FLOOR
    deg = calib(sw, c=0.0, sigma=0.0, n_db=1000, status=sw.capi.CALIB_DEGENERATE)
    assert sw.capi.sig_rank_min(deg, 1000) == rs.R_FLOOR and sw.capi.sig_rank_min(deg, 1e9) == rs.R_FLOOR
    assert sw.capi.sig_rank_min(deg, 999.9) == rs.R_NONE and sw.capi.sig_rank_min(deg, 1e-5) == rs.R_NONE
    L = sw.capi.lib()
    r = ctypes.c_int64(0)
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        assert L.sw_sig_rank_min(ctypes.byref(cal), bad, ctypes.byref(r)) == -1
    assert L.sw_sig_rank_min(None, 1.0, ctypes.byref(r)) == -1 and L.sw_sig_rank_min(ctypes.byref(cal), 1.0, None) == -1
    assert L.sw_sig_rank_min(ctypes.byref(sw.capi.Calib()), 1.0, ctypes.byref(r)) == -1  # size 0: not sw_calib_fit's
    assert L.sw_sig_rank_table(ctypes.byref(cal), -1, None) == -1
    assert L.sw_sig_topk_device(None, None, None, None, 0, 0, 5, None, None) == -1
    assert L.sw_scan_hits_ranked(None, None, None, 0, None, 5, 1.0, None, None, None, None, None) == -1


@pytest.mark.parametrize("fit", [(19.6, 4.13, 6.2, 570000), (31.0, 0.8, 9.5, 300), (8.0, 6.5, 5.0, 20001)])
def test_rank_min_agrees_with_the_evalue(sw, fit):
    """Hand-made (s, L): with r >= r_min, sw_calib_sig's E <= max_evalue
    (1 + 1e-3); with r <= r_min - 2, E > max_evalue (1 - 1e-3)."""
    a, c, sigma, n_db = fit
    cal = calib(sw, a, c, sigma, n_db)
    adj = sw.capi.sig_rank_table(cal, 40000)
    lens = np.array([1, 2, 3, 17, 100, 290, 1000, 5000, 35213, 40000], dtype=np.int64)
    s, L = [v.ravel() for v in np.meshgrid(np.arange(1, 1400, 3), lens, indexing="ij")]
    r = rs.rank_values(s, L, adj)
    e = np.array([sw.capi.calib_sig(cal, int(si), int(Li))[0] for si, Li in zip(s, L)])
    prev = rs.R_NONE
    for max_e in (1e-40, 1e-9, 1e-3, 0.5, 1.0, 10.0, n_db * 0.5, n_db * (1 - 1e-9)):
        r_min = sw.capi.sig_rank_min(cal, max_e)
        assert rs.R_FLOOR < r_min < rs.R_NONE and r_min <= prev
        prev = r_min
        above, below = r >= r_min, r <= r_min - 2
        print("max_evalue %g: r_min %d, %d above, %d below" % (max_e, r_min, above.sum(), below.sum()))
        assert above.any() and below.any()
        assert np.all(e[above] <= max_e * (1 + 1e-3))
        assert np.all(e[below] > max_e * (1 - 1e-3))
        # the closed form: r_min / 4096 = a + sigma z_min
        t = -math.log(-math.log1p(-max_e / n_db))
        z_min = (t - 0.5772156649015329) / (math.pi / math.sqrt(6))
        assert abs(r_min - 4096 * (a + sigma * z_min)) <= 1 + 1e-9 * abs(r_min)


def test_restatement_orders_by_significance(sw):
    """rank_support on its own ground: r orders (s, L) as z does, ties go to
    the lower id, the floor cases, both saturations."""
    cal = calib(sw)
    adj = sw.capi.sig_rank_table(cal, 3000).astype(np.int64)
    s = np.array([60, 60, 60, 0, -5, 90, 60, 2 ** 20 + 5, 60], dtype=np.int64)
    L = np.array([100, 1000, 100, 50, 50, 3000, 0, 7, 5000], dtype=np.int64)
    ids = np.array([4, 9, 2, 30, 1, 7, 8, 3, 11], dtype=np.int64)
    r = rs.rank_values(s, L, adj)
    assert r[0] == r[2] == 60 * 4096 - adj[100] and r[1] == 60 * 4096 - adj[1000] < r[0]
    assert r[3] == r[4] == r[6] == rs.R_FLOOR and r[7] == (2 ** 20 - 1) * 4096 - adj[7]
    assert r[8] == 60 * 4096 - adj[3000]  # lengths past the table take its last entry
    z = [sw.capi.calib_sig(cal, int(a), int(b))[2] for a, b in zip(s[[0, 1, 5]], L[[0, 1, 5]])]
    assert (z[0] > z[1]) == (r[0] > r[1]) and (z[2] > z[0]) == (r[5] > r[0])
    sel, n = rs.ranked(s, L, ids, adj, rs.R_FLOOR, 12)
    assert n == 9 and rs.key_ids(sel).tolist()[:4] == [3, 7, 2, 4] and rs.key_ids(sel).tolist()[-3:] == [1, 8, 30]
    assert np.all(sel[9:] == rs.PAD)
    sel, n = rs.ranked(s, L, ids, adj, int(r[1]), 2)
    assert n == 5 and rs.key_ids(sel).tolist() == [3, 7]
    big = np.array([0, -2 ** 31, 2 ** 31 - 1], dtype=np.int32)
    assert rs.rank_values([2 ** 31 - 1, 1, 1], [1, 0, 2], big).tolist() == [rs.R_CEIL, rs.R_FLOOR, 4096 - (2 ** 31 - 1)]
    assert rs.keys([rs.R_FLOOR], [2 ** 31 - 1])[0] > rs.PAD


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not found")
def test_ranked_groups(tmp_path):
    """nq = 0, 1, 5 with budgets below one row, exactly two rows, more than nq
    rows, and the default, against the restatement."""
    exe = str(tmp_path / "rank_groups_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall"] + INC +
                   [os.path.join(ROOT, "tests", "native", "rank_groups_check.cpp"), os.path.join(CSRC, "sw_plan.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2] == "rank_groups_check ok", r.stdout + r.stderr
    got = {}
    for ln in lines[:-2]:
        nq, slots, budget, g = [int(v) for v in ln.split()]
        assert g == rs.ranked_groups(nq, slots, budget), ln
        got[nq, slots, budget] = g
    row = 4 * 901
    assert [got[nq, 901, row - 1] for nq in (0, 1, 5)] == [1, 1, 1]        # below one row
    assert [got[nq, 901, 2 * row] for nq in (0, 1, 5)] == [1, 1, 2]        # exactly two rows
    assert [got[nq, 901, 2 * row - 1] for nq in (0, 1, 5)] == [1, 1, 1]
    assert [got[nq, 901, 6 * row] for nq in (0, 1, 5)] == [1, 1, 5]        # more than nq rows
    assert [got[nq, 901, 0] for nq in (0, 1, 5)] == [1, 1, 5]              # the default: 256 MiB
    assert got[1000, 570000, 0] == (256 << 20) // (4 * 570000) == 117 and got[7, 0, 0] == 7


def test_cli_rank_flags_are_checked_before_any_file_is_read():
    """The files named here do not exist: exit 1 on the flags alone."""
    main = os.path.join(LIB, "main")
    base = [main, "--db", "/nonexistent/db.fasta"]
    one, many = ["--query", "/nonexistent/q.fasta"], ["--queries", "/nonexistent/qs.fasta"]
    cases = [
        (one + ["--rank", "evalue"], ("--rank", "--hits", "--evalue")),
        (one + ["--hits", "5", "--rank", "evalue"], ("--rank", "--evalue")),
        (one + ["--topk", "5", "--rank", "evalue"], ("--rank", "--hits")),
        (many + ["--hits", "5", "--rank", "evalue"], ("--rank", "--evalue")),
        (one + ["--hits", "5", "--evalue", "--rank", "score"], ("--rank", "evalue")),
        (one + ["--hits", "5", "--evalue", "--max-evalue", "10"], ("--max-evalue", "--rank evalue")),
        (many + ["--hits", "5", "--evalue", "--max-evalue", "10"], ("--max-evalue", "--rank evalue")),
        (one + ["--max-evalue", "10"], ("--max-evalue", "--rank evalue")),
        (one + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "0"], ("--max-evalue", "> 0")),
        (one + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "-3"], ("--max-evalue", "> 0")),
        (one + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "ten"], ("--max-evalue", "> 0")),
        (one + ["--hits", "5", "--evalue", "--rank", "evalue", "--max-evalue", "nan"], ("--max-evalue", "> 0")),
    ]
    for extra, words in cases:
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and all(w in out.stderr for w in words), (extra, out.stdout, out.stderr)
        assert "cannot open" not in out.stderr.lower() and "nonexistent" not in out.stderr
