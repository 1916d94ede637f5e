"""CPU: the calibration of E-values and bit scores (include/sw_amd.h,
csrc/sw_calib.cpp) without a GPU.  The count tables are built in numpy from
oracle scores; sw_calib_fit and sw_calib_sig run through ctypes and are
compared with the numpy restatement in tests/calib_support.py.

Tolerances (from the arithmetic, not from the code under test): a, c and
sigma are double sums of at most 65,408 terms over a regression whose
abscissae span about 0 to 21, so relative 1e-9 is far above their rounding;
E's exponent amplifies the error of a z in the hundreds, so relative 1e-6
where E > 1e-300; bits is linear in z: absolute 1e-6.

tests/native/calib_check.cpp is sw_calib.cpp's stand-alone program, built
with -fsanitize=address,undefined and run on its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import calib_support as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "csrc")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")


@pytest.fixture(scope="module")
def calib_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("calib") / "calib_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"] + INC +
                   [os.path.join(ROOT, "tests", "native", "calib_check.cpp"), os.path.join(CSRC, "sw_calib.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


@needs_gxx
def test_native_check_under_sanitizers(calib_check):
    r = subprocess.run([calib_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("calib_check ok"), r.stdout[-4000:] + r.stderr[-4000:]


@needs_gxx
def test_length_bin(calib_check):
    """Every L in 1..70,000 and 2^k - 1, 2^k, 5 * 2^(k-2) for k <= 30 against
    the numpy restatement (bit lengths, no floats); monotone in L."""
    r = subprocess.run([calib_check, "bins"], capture_output=True, text=True, timeout=120, check=True)
    got = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 2)
    want_L = list(range(1, 70001))
    for k in range(2, 31):
        want_L += [2 ** k - 1, 2 ** k, 5 * 2 ** (k - 2)]
    want_L.append(2 ** 31 - 1)
    assert got[:, 0].tolist() == want_L
    assert np.array_equal(got[:, 1], cs.length_bin(got[:, 0]))
    assert np.array_equal(cs.length_bin_fast(got[:, 0]), got[:, 1])
    assert cs.length_bin([1, 2, 3, 4, 5, 7, 8]).tolist() == [0, 4, 6, 8, 9, 11, 12]
    order = np.argsort(got[:, 0], kind="stable")
    assert np.all(np.diff(got[order, 1]) >= 0) and got[:, 1].max() == 123 < cs.LBINS


def test_constants_are_mirrored(sw):
    hdr = open(os.path.join(ROOT, "include", "sw_amd.h")).read()
    for name, val in (("LBINS", 128), ("SBINS", 512), ("CLIPPED", 1), ("FEW", 2), ("DEGENERATE", 4)):
        assert "#define SW_CALIB_%s %d\n" % (name, val) in hdr
        assert getattr(sw.capi, "CALIB_" + name) == val
    assert (cs.LBINS, cs.SBINS, cs.CLIPPED, cs.FEW, cs.DEGENERATE) == (128, 512, 1, 2, 4)
    assert sw.capi.lib().sw_version() >= 500


def compare_fit(sw, H, qlen):
    got = sw.capi.calib_fit(H, qlen)
    want = cs.fit(H, qlen)
    for f in ("status", "qlen", "fits", "n_db", "n_fit", "n_clipped"):
        assert getattr(got, f) == want[f], (f, got.as_dict(), want)
    assert got.n_skipped == 0
    for f in ("a", "c", "sigma"):
        assert getattr(got, f) == pytest.approx(want[f], rel=1e-9, abs=0), (f, got.as_dict(), want)
    return got, want


def compare_sig(sw, got, want, scores, lengths):
    for s, L in zip(scores, lengths):
        e, bits, z = sw.capi.calib_sig(got, int(s), int(L))
        we, wb, wz = cs.sig(want, int(s), int(L))
        print("score %d len %d: E %.6g (%.6g) bits %.6f (%.6f) z %.4f" % (s, L, e, we, bits, wb, z))
        if we > 1e-300:
            assert e == pytest.approx(we, rel=1e-6, abs=0)
        else:
            assert e <= 1e-300 * (1 + 1e-6)
        assert abs(bits - wb) <= 1e-6


@pytest.fixture(scope="module")
def unrelated(sw, oracle):
    """synth.database(20000) against synth.query(375): the scores under
    BLOSUM62 11/1 and under the reference's BLOSUM50 with linear gap 2."""
    r, o = sw.synth.database(20000)
    q = sw.synth.query(375)
    b62 = oracle.scan(q, r, o, oracle.matrix(oracle.MATRIX_BLOSUM62), 11, 1)
    ref = oracle.scan(q, r, o, oracle.matrix(oracle.MATRIX_BLOSUM50_REF), 2, 2)
    b62.setflags(write=False)
    ref.setflags(write=False)
    return np.diff(o), b62, ref


def test_fit_and_significance_match_numpy(sw, unrelated):
    L, b62, ref = unrelated
    rng = np.random.default_rng(5)
    for scores in (b62, ref):
        got, want = compare_fit(sw, cs.table(scores, L), 375)
        pick = rng.choice(len(L), 40, replace=False)
        compare_sig(sw, got, want, scores[pick], L[pick])
        # the tail: z in the hundreds, E far below 1 and below 1e-300, and the trivial rows
        compare_sig(sw, got, want, [200, 510, 2000, 100000, 2 ** 31 - 1, 0, -3, 40], [300, 35, 5000, 12, 7, 300, 300, 0])


def test_unrelated_sequences_are_calibrated(sw, unrelated):
    """All unrelated: E <= 10 is expected of 10 subjects (the oracle alone
    gives 14 here); [2, 30] is a Poisson(10) count's range with room for the
    fit's own error.  No clipping under BLOSUM62 11/1."""
    L, b62, _ = unrelated
    cal = sw.capi.calib_fit(cs.table(b62, L), 375)
    e = np.array([sw.capi.calib_sig(cal, int(s), int(n))[0] for s, n in zip(b62, L)])
    n10, n1 = int((e <= 10).sum()), int((e <= 1).sum())
    print("E <= 10: %d, E <= 1: %d; %s" % (n10, n1, cal.as_dict()))
    assert 2 <= n10 <= 30
    assert not cal.status & cs.CLIPPED and cal.status == 0
    assert cal.n_db == 20000 and cal.n_clipped == 0
    assert np.allclose(e, cs.evalues(cs.fit(cs.table(b62, L), 375), b62, L), rtol=1e-6, atol=0)


def test_scores_that_grow_with_length_are_flagged(sw, unrelated):
    """The reference's BLOSUM50 with gap 2/2: scores grow with the subject's
    length and 3,496 of the 20,000 clip; no local statistic exists there."""
    L, _, ref = unrelated
    cal = sw.capi.calib_fit(cs.table(ref, L), 375)
    assert cal.n_clipped == int((ref >= 511).sum()) == 3496
    assert cal.status & cs.CLIPPED


def test_planted_relatives(sw, oracle):
    """Five mutated copies of the query (every 4th residue replaced) among
    5,000 random subjects: each is found (E < 1e-6), each leaves the fit, and
    an unrelated subject's E moves by less than a factor of 2."""
    q = sw.synth.query(375)
    r, o = sw.synth.database(5000, shard=3)
    rng = np.random.default_rng(11)
    copies = []
    for _ in range(5):
        c = q.copy()
        pos = np.arange(int(rng.integers(0, 4)), len(c), 4)
        c[pos] = (c[pos] + rng.integers(1, 20, size=len(pos))) % 20
        copies.append(c)
    r2 = np.concatenate([r] + copies)
    o2 = np.concatenate([o, o[-1] + np.cumsum([len(c) for c in copies])])
    mat = oracle.matrix(oracle.MATRIX_BLOSUM62)
    s2 = oracle.scan(q, r2, o2, mat, 11, 1)
    L2 = np.diff(o2)
    with_, _ = compare_fit(sw, cs.table(s2, L2), 375)
    without, _ = compare_fit(sw, cs.table(s2[:5000], L2[:5000]), 375)
    assert with_.n_db == 5005 and with_.n_fit <= with_.n_db - 5 and with_.status == 0
    for k in range(5000, 5005):
        e = sw.capi.calib_sig(with_, int(s2[k]), int(L2[k]))[0]
        print("copy %d: score %d E %.3g" % (k - 5000, s2[k], e))
        assert e < 1e-6
    e_with = cs.evalues(cs.fit(cs.table(s2, L2), 375), s2[:5000], L2[:5000])
    e_without = cs.evalues(cs.fit(cs.table(s2[:5000], L2[:5000]), 375), s2[:5000], L2[:5000])
    ratio = e_with / e_without
    print("E ratio with / without the copies: %.4f .. %.4f" % (ratio.min(), ratio.max()))
    assert ratio.max() < 2 and ratio.min() > 0.5


def test_edge_tables(sw):
    D = cs.DEGENERATE
    zero = np.zeros((cs.LBINS, cs.SBINS), dtype=np.uint32)
    one_bin = zero.copy()
    one_bin[33, 20:60] = 50
    one_score = zero.copy()
    one_score[20:50, 37] = 100
    clipped = zero.copy()
    clipped[20:50, 511] = 100
    for name, H, mean in (("zero", zero, 0.0), ("one bin", one_bin, 39.5), ("one score", one_score, 37.0),
                          ("clipped", clipped, 0.0)):
        got, want = compare_fit(sw, H, 100)
        assert got.status & D, name
        assert (got.a, got.c, got.sigma) == (mean, 0.0, 0.0), name
        for s, L in ((50, 300), (0, 300), (400, 10), (50, 0)):
            assert sw.capi.calib_sig(got, s, L) == (float(got.n_db), 0.0, 0.0), name
    assert sw.capi.calib_fit(clipped, 100).status & cs.CLIPPED
    assert sw.capi.calib_fit(zero, 100).status & cs.FEW and sw.capi.calib_fit(one_bin, 100).status & cs.FEW


def test_clip_column_never_enters_the_fit(sw, unrelated):
    L, b62, _ = unrelated
    H = cs.table(b62, L)
    base = sw.capi.calib_fit(H, 375)
    H2 = H.copy()
    H2[40:44, 511] = 17
    more = sw.capi.calib_fit(H2, 375)
    assert (more.a, more.c, more.sigma, more.n_fit, more.fits) == (base.a, base.c, base.sigma, base.n_fit, base.fits)
    assert more.n_clipped == 68 and more.n_db == base.n_db + 68 and not more.status & cs.CLIPPED


def test_argument_errors(sw):
    L = sw.capi.lib()
    cal, s = sw.capi.Calib(), sw.capi.Sig()
    import ctypes
    assert L.sw_calib_fit(None, 10, ctypes.byref(cal)) == -1
    assert L.sw_calib_sig(None, 10, 10, ctypes.byref(s)) == -1
    assert L.sw_calib_sig(ctypes.byref(cal), 10, 10, ctypes.byref(s)) == -1  # size 0: not sw_calib_fit's
    assert L.sw_score_hist(None, None, None, None) == -1
    assert L.sw_scan_hits_sig(None, None, None, 0, None, 5, None, None, None, None) == -1
    with pytest.raises(sw.SWError):
        sw.capi.calib_fit(np.zeros(10, dtype=np.uint32), 5)
