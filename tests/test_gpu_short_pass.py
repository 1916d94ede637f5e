"""The short last pass of the two-strips inter kernels (sw_inter_x2.hip
x2s_pass; swplan::short_rows): a query's last pass runs R - 4 rows per strip
instead of R where two strips of that height hold the rows it has left.  Every
score bit-exact against the oracle, for query lengths around every boundary
of Re, four scorings, block widths 8 .. > 1,024 columns, single waves, pairs,
quads and tris, the separate launches and the merged one, with the maxima on
the rows next to the strips' new edges and a block that crosses the fp16
guard band."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QLENS = (1, 3, 4, 5, 8, 9, 56, 57, 63, 64, 65, 68, 69, 120, 121, 128, 129, 144, 375, 376, 377, 384, 385)
QLENS_LINEAR_96 = (96, 97, 185, 192, 193)  # the merged launch's 96-row passes under linear gaps
# (matrix id, gap open, gap extend): BLOSUM62 12/1 and 14/3, BLOSUM50 linear 2, BLOSUM62 linear 5
SCORINGS = ((1, 12, 1), (1, 14, 3), (0, 2, 2), (1, 5, 5))
LONG = 1500
# the kernel forms: sw_opts overrides
FORMS = {
    "single": dict(lpt="0", pair_width="0"),
    "pairs": dict(lpt="0", pair_width="16"),
    "lpt-singles": dict(lpt="1", pair_width="1024", quad_width="0", tri_width="0"),
    "lpt-quads": dict(lpt="1", pair_width="16", quad_width="16", tri_width="0"),
    "lpt-tris": dict(lpt="1", pair_width="16", quad_width="0", tri_width="16"),
}


def short_rows(qlen, rows):
    """Re (rows per strip of the last pass) and the last pass's first row."""
    s0 = (qlen - 1) // rows * rows
    left = qlen - s0
    return (rows // 2 - 4 if (left + 1) // 2 <= rows // 2 - 4 else rows // 2), s0


def edge_cuts(qlen):
    """Prefix lengths whose best cell lies on the low strip's bottom row of
    the short pass, one row before and one after (64- and 96-row passes)."""
    cuts = set()
    for rows in (64, 96):
        re_, s0 = short_rows(qlen, rows)
        cuts.update(c for c in (s0 + re_ - 1, s0 + re_, s0 + re_ + 1) if 0 < c <= qlen)
    return cuts


_state = {}


def _database(sw):
    """Blocks 8, 16, 24, 32, 40, 56, 64 and 72 columns wide, a few hundred, over 1,024, a
    few long subjects (the merged launch needs some), and copies of the
    query's prefixes: the whole query (best cell on its last row) and the
    prefixes ending on and next to the short pass's strip edge."""
    if "db" not in _state:
        q0 = sw.synth.query(385, shard=5)
        lens = []
        for w in (8, 16, 24, 32, 40):
            lens += [w - k % 8 for k in range(64)]
        # around the single-wave blocks' switch to the short pass (64 columns):
        # two blocks' worth per width, so one block of each is whole whatever
        # the planted subjects do to the packing
        for w in (56, 64, 72):
            lens += [w - k % 8 for k in range(128)]
        lens += [150 + (k * 37) % 150 for k in range(128)]
        lens += [1030 + k for k in range(64)]
        lens += [1600 + 20 * k for k in range(6)]
        res = sw.synth.residues(int(sum(lens)), shard=17)
        cuts = set()
        for n in QLENS + QLENS_LINEAR_96:
            cuts.add(n)
            cuts.update(edge_cuts(n))
        planted = [q0[:c] for c in sorted(cuts)]
        r = np.concatenate([res] + planted)
        o = np.concatenate([[0], np.cumsum(lens + [len(p) for p in planted])]).astype(np.int64)
        _state["db"] = (q0, r, o)
    return _state["db"]


def _want(sw, oracle, q, r, o, scoring, key):
    """The oracle's scores, computed once per (database, query, scoring)."""
    k = (key, len(q), scoring)
    if k not in _state:
        mid, go, ge = scoring
        _state[k] = oracle.scan(q, r, o, mat=sw.capi.builtin_matrix(mid), gap_open=go, gap_extend=ge)
    return _state[k]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("scoring", SCORINGS)
def test_short_last_pass(sw, oracle, handle, knobs, scoring, form):
    mid, go, ge = scoring
    knobs(inter_i16_span="0", intra_i16_first="0", **FORMS[form])
    q0, r, o = _database(sw)
    db = sw.Database(handle, r, o, long_threshold=LONG)
    m = sw.capi.builtin_matrix(mid)
    qlens = QLENS + (QLENS_LINEAR_96 if go == ge else ())
    merged = 0
    try:
        for qlen in qlens:
            q = q0[:qlen]
            got = db.scan(q, m, go, ge)
            merged += "+lpt" in handle.last_kernel()
            want = _want(sw, oracle, q, r, o, scoring, "prefix")
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (qlen, handle.last_kernel(), bad[:10], got[bad[:10]], want[bad[:10]])
    finally:
        db.close()
    # the merged launch takes every query of two passes or more
    if form.startswith("lpt"):
        assert merged == sum(n > 64 for n in qlens), merged
    else:
        assert merged == 0


@pytest.mark.parametrize("lpt", ["0", "1"])
@pytest.mark.parametrize("scoring", SCORINGS)
def test_short_pass_guard_band(sw, oracle, handle, knobs, scoring, lpt):
    """A near-copy of a tryptophan-rich query scores past the fp16 guard band
    (W-W is the matrices' largest entry, 11 or 15): its block, flagged
    by a short last pass, is re-scored by the rescue chain (lpt 0) and by the
    merged launch's drain (lpt 1)."""
    mid, go, ge = scoring
    knobs(inter_i16_span="0", intra_i16_first="0", lpt=lpt, pair_width="64")
    _, r, o = _database(sw)
    w = int(sw.encode("W")[0])
    m = sw.capi.builtin_matrix(mid)
    for qlen in (375, 377):
        q = np.full(qlen, w, dtype=np.uint8)
        q[::125] = int(sw.encode("A")[0])
        near = q.copy()
        near[qlen // 2] = int(sw.encode("G")[0])
        r2 = np.concatenate([r, near, q[:200]])
        o2 = np.concatenate([o, [o[-1] + qlen, o[-1] + qlen + 200]]).astype(np.int64)
        db = sw.Database(handle, r2, o2, long_threshold=LONG)
        try:
            got = db.scan(q, m, go, ge)
            assert ("+lpt" in handle.last_kernel()) == (lpt == "1"), handle.last_kernel()
            want = _want(sw, oracle, q, r2, o2, scoring, "guard")
            # the fp16 form's limit (sw_capi.cpp inter_args): at or past it the lane flags its block
            assert want[-2] >= 4096 - 28 * ge - 2 * int(np.max(m)), want[-2]
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (qlen, handle.last_kernel(), bad[:10], got[bad[:10]], want[bad[:10]])
        finally:
            db.close()
