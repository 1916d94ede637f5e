"""GPU: the column-0 image of the affine fp16 inter scan (sw_inter_x2.hip X2Lds
hi0; tests/test_col0_image.py has the arithmetic), score for score against the
CPU oracle.

H is no longer rebased between the 8-column sub-groups: column 0's high-strip
reads take an image 8 ge lower in both halves.  A mistake shows where a
diagonal or a gap run crosses a sub-group's first column (columns 7|8, 15|16)
in either strip, at a row group's first row (whose profile entries carry - 16
ge too: rows 15|16 and 31|32 of a strip pair, with the strips' delay line at
32), at a pass's first sub-group, at a chain's restaging and in the short last
pass.  So:

  blocks    8, 16, 24 columns (1 to 3 sub-groups, never chained), 40 (chained
            at full height), 64 and 72 (the short last pass on its own after
            the chain), two blocks of 64 subjects each
  queries   64 rows (one pass), 65 (two), 119 (the last pass short, 2 x 28
            rows), 128 (the last pass full), 375 (five full passes and a short)
  scorings  BLOSUM62 12/1 and 13/3; the admission bound 2 max S + 27 ge + go =
            1023 (entries -100 .. 100, 67/28) and open below extend (-9 .. 13,
            5/6) of tests/test_cell_range.py; a position-specific table, 12/1
  forms     single waves; pairs and quads (separate launch), tris and the
            merged launch with its in-launch drain, through sw_opts

Subjects: pieces of the query laid so that the diagonal through (row seam,
column seam) is theirs: unbroken, with 2 or 3 foreign residues inserted across
the column seam (a gap run along the row), or with 2 or 3 query rows left out
across the row seam (a gap run down the column); row seams at every strip,
row-group and pass edge of the five queries, the short passes' included.
Under the admission-bound scoring the 64- and 72-column copies pass the fp16
guard: their blocks flag and are re-scored, which the test asserts from the
library's rescue statistics; under BLOSUM62 12/1 a near-copy of a
tryptophan-rich query does (test_guard_band).  No tolerance anywhere."""
import re

import numpy as np
import pytest

import seam_support as ss
from pssm_support import PssmOracle, derived

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 24, 40, 64, 72)
QLENS = (64, 65, 119, 128, 375)
PER_WIDTH = 128            # two blocks of each width
LONG = 100                 # long threshold: the merged launch needs long subjects
ROW_SEAMS = (16, 32, 48, 64, 80, 92, 96, 108, 112, 128, 336, 348, 352, 364)
COL_SEAMS = (8, 16)
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged")

_LPT = dict(lpt=1, intra_x2_rows=4, tail_pairs=0, lpt_persist=0, lpt_pipe=0, lpt_pipe_tail=0)
FORMS = {
    "single": dict(lpt=0, coop_width=0, pair_width=0),
    "pair": dict(lpt=0, coop_width=0, pair_width=8, pair_group=2),
    "quad": dict(lpt=0, coop_width=0, pair_width=8, pair_group=4),
    "tri": dict(_LPT, pair_width=8, quad_width=0, tri_width=8),
    # 64 and 72 columns by groups (72: quads), the narrower blocks one per wave inside the launch
    "merged": dict(_LPT, pair_width=64, quad_width=72, tri_width=0),
}
SCORINGS = ("b62-12-1", "b62-13-3", "admission-bound", "open-below-extend", "pssm-12-1")


class Env:
    pass


def _subjects(q):
    """PER_WIDTH subjects per width, each w - 7 .. w residues long (so every
    block of the class is w columns wide), then four long ones."""
    foreign = np.array([4, 8, 14, 17], dtype=np.uint8)  # C, H, P, W: not in the query
    subs = []
    for w in WIDTHS:
        plans = []
        for rs in ROW_SEAMS:
            for cs in COL_SEAMS:
                c = cs if cs < w else w // 2
                plans.append(("diag", rs, c, 0))
                for L in (2, 3):
                    plans.append(("col", rs, c, L))
                    plans.append(("row", rs, c, L))
        assert len(plans) >= PER_WIDTH
        for k in range(PER_WIDTH):
            kind, rs, c, L = plans[(k * 37) % len(plans)]
            n = w - k % 8 if k else w
            r0 = rs - c  # query row of subject column 0
            if kind == "diag" or n < c + 4:
                s = q[r0:r0 + n]
            elif kind == "col":
                # subject columns c - 1 .. c + L - 2 stand against gaps
                s = np.concatenate([q[r0:r0 + c - 1], foreign[(np.arange(L) + k) % 4], q[r0 + c - 1:r0 + n - L]])
            else:
                # query rows rs - 1 .. rs + L - 2 stand against gaps, at subject column c - 1
                s = np.concatenate([q[r0:rs - 1], q[rs - 1 + L:rs - 1 + L + n - (c - 1)]])
            assert len(s) == n, (w, kind, rs, c, L, len(s), n)
            subs.append(s)
    for k in range(4):
        s = q[40 * k:40 * k + 180].copy()
        s[60 + k] = foreign[k]
        subs.append(s)
    return subs


@pytest.fixture(scope="module")
def env(sw, oracle, handle, tmp_path_factory):
    e = Env()
    e.q = ss.build().q2[:480]  # no residue twice in a row; rows past 375 only feed the subjects
    subs = _subjects(e.q)
    e.res = np.concatenate(subs).astype(np.uint8)
    e.offs = np.zeros(len(subs) + 1, dtype=np.int64)
    e.offs[1:] = np.cumsum([len(s) for s in subs])
    e.inter = np.array([len(s) < LONG for s in subs])
    b62 = np.asarray(sw.capi.builtin_matrix(1), dtype=np.int8).reshape(25, 25)
    W, C = int(sw.encode("W")[0]), int(sw.encode("C")[0])

    def extremes(m, lo, hi):
        m = m.copy()
        m[W, W] = hi
        m[W, C] = m[C, W] = lo
        assert m.max() == hi and m.min() == lo
        return np.ascontiguousarray(m, dtype=np.int8)

    adm = extremes(np.clip(b62.astype(np.int64) * 9, -100, 100).astype(np.int8), -100, 100)
    assert 2 * 100 + 27 * 28 + 67 == 1023
    e.scorings = {"b62-12-1": (b62, 12, 1), "b62-13-3": (b62, 13, 3), "admission-bound": (adm, 67, 28),
                  "open-below-extend": (extremes(b62, -9, 13), 5, 6), "pssm-12-1": (b62, 12, 1)}
    e.db = sw.Database(handle, e.res, e.offs, long_threshold=LONG)
    st = e.db.stats()
    assert st["n_long"] == 4 and st["n_blocks"] == len(WIDTHS) * PER_WIDTH // 64, st
    pso = PssmOracle(tmp_path_factory.mktemp("pssm"))
    cache = {}

    def table(qlen):
        """A position-specific table: the query's rows under BLOSUM62, the
        query's own residue 0, 1 or 2 higher by position."""
        rows = derived(e.q[:qlen], b62).astype(np.int64)
        rows[np.arange(qlen), e.q[:qlen]] += np.arange(qlen) % 3
        return np.ascontiguousarray(rows, dtype=np.int8)

    def want(name, qlen):
        if (name, qlen) not in cache:
            m, go, ge = e.scorings[name]
            if name.startswith("pssm"):
                w = pso.scan(table(qlen), e.res, e.offs, gap_open=go, gap_extend=ge)
            else:
                w = oracle.scan(e.q[:qlen], e.res, e.offs, mat=m, gap_open=go, gap_extend=ge)
            w.setflags(write=False)
            cache[(name, qlen)] = w
        return cache[(name, qlen)]

    e.table, e.want = table, want
    yield e
    e.db.close()


def _scan(sw, env, handle, name, qlen):
    m, go, ge = env.scorings[name]
    if name.startswith("pssm"):
        t = env.table(qlen)
        p = sw.Pssm(handle, t)
        try:
            return env.db.scan_pssm(p, go, ge), int(t.max())
        finally:
            p.close()
    return env.db.scan(env.q[:qlen], m, go, ge), int(m.max())


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("scoring", SCORINGS)
def test_col0_image(sw, env, handle, knobs, capfd, scoring, form):
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    knobs(**FORMS[form])
    ge = env.scorings[scoring][2]
    flagged_any = False
    for qlen in QLENS:
        want = env.want(scoring, qlen)
        capfd.readouterr()
        got, max_s = _scan(sw, env, handle, scoring, qlen)
        found = RESCUE.findall(capfd.readouterr().err)
        name = handle.last_kernel()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (scoring, form, qlen, name, bad[:10], got[bad[:10]], want[bad[:10]])
        # the form that was meant ran (groups and the merged launch need two passes)
        if form == "single" or qlen <= 64:
            assert name.startswith("sw_inter_x2s<32,8,affine,fp16>"), (form, qlen, name)
        else:
            assert name.startswith("sw_inter_x2p<32,8,affine,fp16>"), (form, qlen, name)
            assert name.endswith("+lpt+drain") == (form in ("tri", "merged")), (form, qlen, name)
            assert ("+tri" in name) == (form == "tri"), (form, qlen, name)
        # a lane flags its block exactly when its true maximum reaches the guard
        assert found, "no rescue: line"
        limit = 4096 - 28 * ge - 2 * max_s
        crossed = bool(want[env.inter].max() >= limit)
        assert (int(found[-1]) > 0) == crossed, (scoring, form, qlen, found[-1], int(want[env.inter].max()), limit)
        flagged_any |= crossed
    assert flagged_any == (scoring == "admission-bound"), scoring


@pytest.mark.parametrize("form", ["single", "merged"])
def test_guard_band(sw, oracle, env, handle, knobs, capfd, form):
    """BLOSUM62 12/1: a near-copy of a tryptophan-rich 375-row query (W-W = 11,
    the largest entry) passes the fp16 guard, 4096 - 28 - 22: its lane flags
    and the block is re-scored (the rescue launches; the merged launch's
    drain), the probes of the other blocks beside it."""
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    knobs(**dict(FORMS[form], pair_width=64))
    m, go, ge = env.scorings["b62-12-1"]
    w = int(sw.encode("W")[0])
    q = np.full(375, w, dtype=np.uint8)
    q[::125] = int(sw.encode("A")[0])
    near = q.copy()
    near[187] = int(sw.encode("G")[0])
    keep = env.offs[-5]  # the short subjects
    # (the last one is long: the merged launch needs a long subject)
    r = np.concatenate([env.res[:keep], near[:90], near, env.q[:450]])
    o = np.concatenate([env.offs[:-4], keep + np.cumsum([90, 375, 450])]).astype(np.int64)
    db = sw.Database(handle, r, o, long_threshold=400)
    try:
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        found = RESCUE.findall(capfd.readouterr().err)
        name = handle.last_kernel()
    finally:
        db.close()
    want = oracle.scan(q, r, o, mat=m, gap_open=go, gap_extend=ge)
    assert want[-2] >= 4096 - 28 * ge - 2 * int(m.max()), int(want[-2])
    assert np.array_equal(got, want), (form, name, np.nonzero(got != want)[0][:10])
    assert name.endswith("+lpt+drain") == (form == "merged"), name
    assert found and int(found[-1]) >= 1, found
