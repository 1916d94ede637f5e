"""The biased cell of the two-strips inter kernels as integers (sw_inter_x2.hip
x2s_pass; swplan::cell_range): each 16-bit half holds true + bias + Z, sums and
differences are 32-bit integer ops on the dword, and fp16 only compares.  The
cases here are the ones where a carry or a borrow could cross bit 16 or a value
could leave the positive normal fp16 patterns: the two strips pulling opposite
ways, the largest admissible scheme with the API's most negative entries, the
rows a short pass leaves out parked over a 2,000-column block, and a lane that
wraps all 16 bits.  Every score is compared for equality with the oracle."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; ")


def pack(subs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in subs])]).astype(np.int64)
    return np.concatenate(subs).astype(np.uint8), offs


def check(sw, oracle, handle, q, res, offs, m, go, ge):
    db = sw.Database(handle, res, offs, long_threshold=100000)
    try:
        assert db.stats()["n_long"] == 0
        got = db.scan(q, m, go, ge)
        k = handle.last_kernel()
    finally:
        db.close()
    assert ",fp16>" in k, k
    want = oracle.scan(q, res, offs, mat=m, gap_open=go, gap_extend=ge)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (k, bad[:10], got[bad[:10]], want[bad[:10]])
    return want, k


@pytest.mark.parametrize("scoring", [(1, 12, 1), (0, 2, 2), (1, 5, 6)],
                         ids=["blosum62-12-1", "blosum50-linear-2", "open-below-extend"])
def test_strips_pull_opposite_ways(sw, oracle, handle, knobs, scoring):
    """Query W x 32, P x 32, W x 32: in the first pass the low strip (rows of W)
    and the high strip (rows of P) take the matrix's largest and most negative
    entries against the same column at the same time, so the low half's sign
    extension borrows while the high half grows, and the other way round; the
    last pass (32 rows left) takes the short form.  (Open 5 below extend 6:
    go - ge is negative, and its subtraction must add 1 to BOTH halves.)"""
    mid, go, ge = scoring
    knobs(inter_i16_span=0, intra_i16_first=0)
    W, P, C = (int(sw.encode(c)[0]) for c in "WPC")
    q = np.array([W] * 32 + [P] * 32 + [W] * 32, dtype=np.uint8)
    rng = np.random.default_rng(81)
    subs = [rng.choice([W, P, C], size=int(n)).astype(np.uint8) for n in rng.integers(24, 121, size=126)]
    subs += [np.full(120, W, dtype=np.uint8), np.full(120, P, dtype=np.uint8)]
    res, offs = pack(subs)
    want, _ = check(sw, oracle, handle, q, res, offs, sw.capi.builtin_matrix(mid), go, ge)
    assert want.max() > 32 * 11  # the W runs align past one strip


def extreme_matrix():
    """2 max S + 27 ge + go = 1023 with go 67, ge 28: diagonal 30 .. 100, the
    rest down to -100 (the API's bounds)."""
    rng = np.random.default_rng(82)
    m = rng.integers(-100, 41, size=(25, 25))
    np.fill_diagonal(m, rng.integers(30, 101, size=25))
    m[0, 0], m[3, 17], m[17, 3] = 100, -100, -100
    m = np.ascontiguousarray(m, dtype=np.int8)
    assert m.max() == 100 and m.min() == -100
    return m, 67, 28


@pytest.mark.parametrize("qlen", [64, 119])
def test_admissible_extreme(sw, oracle, handle, knobs, qlen):
    m, go, ge = extreme_matrix()
    assert 2 * int(m.max()) + 27 * ge + go == 1023
    knobs(inter_i16_span=0, intra_i16_first=0)
    rng = np.random.default_rng(83 + qlen)
    q = rng.integers(0, 25, size=qlen).astype(np.uint8)
    subs = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(20, 260, size=190)]
    # near-copies of the query: scores up to the guard, with every gap length's penalty
    subs += [np.delete(q, slice(10, 10 + k)) for k in (1, 2, 5)] + [q[: qlen // 3]]
    res, offs = pack(subs)
    check(sw, oracle, handle, q, res, offs, m, go, ge)


@pytest.mark.parametrize("form", ["single", "pairs"])
@pytest.mark.parametrize("scoring", [(1, 13, 3), (1, 12, 1)], ids=["ge3", "ge1"])
def test_parked_rows_over_a_wide_block(sw, oracle, handle, knobs, scoring, form):
    """A 119-row query's last pass runs 28 rows per strip; the rows left out
    stay parked for the 250 sub-groups of a 2,000-column block (rebased with
    the others they would wrap and borrow from the other half)."""
    mid, go, ge = scoring
    knobs(inter_i16_span=0, intra_i16_first=0, lpt=0, pair_width=0 if form == "single" else 16)
    q = sw.synth.query(119, shard=84)
    rng = np.random.default_rng(85)
    lens = rng.integers(2000, 2041, size=64)
    subs = [sw.synth.residues(int(n), shard=86 + i) for i, n in enumerate(lens)]
    subs[5] = np.concatenate([subs[5][:1900], q])[: int(lens[5])]  # the query's head at the block's far end
    res, offs = pack(subs)
    want, k = check(sw, oracle, handle, q, res, offs, sw.capi.builtin_matrix(mid), go, ge)
    assert ("sw_inter_x2p" in k) == (form == "pairs"), k
    assert want[5] > 200


def test_lane_wraps_all_16_bits(sw, oracle, handle, knobs, capfd):
    """Diagonal 40, a 2,047-residue single-letter query and one subject of
    2,000 copies of that letter: true score 80,000, so the lane's 16-bit halves
    run through the NaN and negative patterns and wrap.  Its block is flagged
    and re-scored like any other (fp16 -> int16 -> int32), and the 63 other
    lanes of the block are untouched."""
    m = np.full((25, 25), -3, dtype=np.int8)
    np.fill_diagonal(m, 40)
    go, ge = 12, 1
    knobs(rescue_stats=1, inter_i16_span=0, intra_i16_first=0)
    A = int(sw.encode("A")[0])
    q = np.full(2047, A, dtype=np.uint8)
    rng = np.random.default_rng(87)
    subs = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(100, 400, size=63)]
    subs.insert(17, np.full(2000, A, dtype=np.uint8))
    res, offs = pack(subs)
    capfd.readouterr()
    want, _ = check(sw, oracle, handle, q, res, offs, m, go, ge)
    found = RESCUE.findall(capfd.readouterr().err)
    assert want[17] == 80000 and np.delete(want, 17).max() < 4096 - 28 * ge - 2 * 40
    assert found, "no rescue: line"
    flagged, again = map(int, found[-1])
    assert flagged == 1 and again == 1, found[-1]
