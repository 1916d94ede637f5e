"""GPU traceback (csrc/sw_align.hip, all four kernels: a sequence or a PSSM
under linear or affine gaps): the tie rules, the ops buffer's contract and the
grouping of hits into launches.

Every alignment is compared field for field with oracle.align (a PSSM derived
from (query, matrix) scores as the pair does, so its alignment is the
oracle's too), and a positive score with the score of its own path.  The
inputs are the tie set of tests/align_support.py, which tests/
test_align_inputs.py shows can tell the tie rules apart, the same alphabets
past one pass of the 256-thread workgroup, gap runs on the rows where passes
meet, unlike hits in one call, short and absent ops buffers, and the smallest
call that needs two launches at the 1 GiB budget."""
import time

import numpy as np
import pytest

from align_support import SCORINGS, TIE_GROUPS, periodic, scoring
from conftest import path_score
from hits_support import pack, seam_query, seam_subjects
from pssm_support import derived

pytestmark = pytest.mark.gpu

NUMBERS = ("score", "q_begin", "q_end", "s_begin", "s_end")


def check(oracle, q, s, mat, go, ge, al, what):
    want = oracle.align(q, s, mat, go, ge)
    assert al == want, (what, al, want)
    if al["score"] > 0:
        assert path_score(q, s, mat, go, ge, al) == al["score"], what
    return want


def both_forms(sw, handle, db, q, ids, mat, go, ge):
    """(sw_align's, sw_align_pssm's on the derived table) alignments."""
    p = sw.Pssm(handle, derived(q, mat))
    try:
        return db.align(q, ids, mat, go, ge), db.align_pssm(p, ids, go, ge)
    finally:
        p.close()


# ---- 1. the tie set ------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_dbs(sw, handle):
    """letters -> (database of every subject of TIE_GROUPS[letters], first id of each group)."""
    dbs = {}
    for letters, groups in TIE_GROUPS.items():
        subs = [s for _, ss in groups for s in ss]
        first = np.concatenate([[0], np.cumsum([len(ss) for _, ss in groups])])
        dbs[letters] = (sw.Database(handle, *pack(subs)), first)
    yield dbs
    for db, _ in dbs.values():
        db.close()


@pytest.mark.parametrize("name", sorted(SCORINGS))
def test_tie_set(sw, oracle, handle, tie_dbs, name):
    mat, go, ge = scoring(name)
    db, first = tie_dbs[SCORINGS[name][0]]
    gapped = 0
    for g, (q, subs) in enumerate(TIE_GROUPS[SCORINGS[name][0]]):
        ids = list(range(first[g], first[g + 1]))
        for form, got in zip(("sequence", "pssm"), both_forms(sw, handle, db, q, ids, mat, go, ge)):
            assert len(got) == len(subs)
            for k, (s, al) in enumerate(zip(subs, got)):
                check(oracle, q, s, mat, go, ge, al, (name, form, g, k))
                gapped += "I" in al["ops"] or "D" in al["ops"]
    assert gapped > 20


# ---- 2. ties past one pass of the workgroup --------------------------------------
MOTIFS = {2: [0, 1, 1, 0, 1], 3: [0, 1, 2, 1, 0, 2, 2]}


@pytest.mark.parametrize("qlen", [255, 256, 257, 513])
def test_ties_past_one_pass(sw, oracle, handle, qlen):
    """Few letters at query lengths around one and two passes of the 256
    threads, subjects shorter than, as long as and longer than the query; and
    periodic inputs, whose equal maxima lie a period apart: a repeated motif
    against one motif (rows that different threads and passes own), one motif
    against the repeat (one row, different columns), repeat against repeat."""
    for letters in (2, 3):
        rng = np.random.default_rng(1000 * letters + qlen)
        rand = lambda n: rng.integers(0, letters, size=n).astype(np.uint8)
        motif = periodic(MOTIFS[letters], 1)
        rep_q, rep_s = periodic(motif, qlen)[:qlen], periodic(motif, 600)[:600]
        subs = [rand(1), rand(2), rand(200), rand(qlen), rand(600), motif, rep_s, rep_q]
        queries = [rand(qlen), rep_q, motif]
        subs[3][:] = np.where(rng.random(qlen) < 0.1, subs[3], queries[0])  # a relative of the random query
        db = sw.Database(handle, *pack(subs))
        ids = list(range(len(subs)))
        for name in sorted(SCORINGS):
            if SCORINGS[name][0] != letters:
                continue
            mat, go, ge = scoring(name)
            for qi, q in enumerate(queries):
                for form, got in zip(("sequence", "pssm"), both_forms(sw, handle, db, q, ids, mat, go, ge)):
                    for k, al in enumerate(got):
                        check(oracle, q, subs[k], mat, go, ge, al, (name, form, qlen, qi, k))
            # the repeat against one motif: the first of the equal maxima, in the first period's rows
            al = db.align(rep_q, [5], mat, go, ge)[0]
            assert al["score"] == len(motif) * SCORINGS[name][1] and al["q_end"] == len(motif)
        db.close()


# ---- 3. gap runs across the rows where passes meet ----------------------------------
@pytest.mark.parametrize("go,ge", [(11, 1), (5, 5)])
def test_gap_runs_across_pass_rows(sw, oracle, handle, go, ge):
    """Copies of a 600-residue query with 1, 2 and 5 rows deleted or columns
    inserted so that the run starts on, crosses and ends on rows 255, 256,
    257, 512 and 513 (hits_support.seam_subjects), BLOSUM62."""
    q = seam_query(600, 20266)
    subs = seam_subjects(q, [255, 256, 257, 512, 513])
    assert len(subs) >= 40
    mat = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, *pack(subs))
    got = db.align(q, list(range(len(subs))), mat, go, ge)
    db.close()
    runs = 0
    for k, al in enumerate(got):
        check(oracle, q, subs[k], mat, go, ge, al, (go, ge, k))
        gaps = al["ops"].replace("M", "")
        runs += gaps in ("I" * (600 - len(subs[k])), "D" * (len(subs[k]) - 600))
    assert runs > len(subs) // 2, "the planted run is the alignment's only gap"


# ---- 4. one call, unlike hits ---------------------------------------------------------
@pytest.mark.parametrize("threshold", [16, 4096, None])
def test_unlike_hits_in_one_call(sw, oracle, handle, threshold):
    """Subjects of 0, 1, 3, 17, 700 and 1 residues under result ids with gaps
    between them, asked for with repeats and out of database order, from the
    long layout (threshold 16: the subjects of 17 and 700), the inter layout
    (4096) and the library's own split."""
    rng = np.random.default_rng(41)
    q = rng.integers(0, 20, size=60).astype(np.uint8)
    subs = [rng.integers(0, 20, size=n).astype(np.uint8) for n in (0, 1, 3, 17, 700, 1)]
    subs[1][0], subs[5][0] = q[7], q[30]
    subs[3][2:14] = q[20:32]
    subs[4][300:357] = np.concatenate([q[:25], q[28:]])  # the query with three rows deleted
    rids = np.array([4, 9, 10, 25, 31, 77], dtype=np.int32)
    db = sw.Database(handle, *pack(subs), ids=rids, long_threshold=threshold)
    st = db.stats()
    assert st["n_subjects"] == 6
    if threshold == 16:
        assert st["n_long"] == 2 and st["n_blocks"] == 1  # both layouts hold subjects
    if threshold == 4096:
        assert st["n_long"] == 0 and st["n_blocks"] == 1
    ask = [31, 4, 77, 25, 31, 9, 10, 4, 31]
    at = {int(r): k for k, r in enumerate(rids)}
    mat = sw.capi.builtin_matrix(1)
    for go, ge in ((5, 5), (11, 1)):
        for form, got in zip(("sequence", "pssm"), both_forms(sw, handle, db, q, ask, mat, go, ge)):
            assert len(got) == len(ask)
            for rid, al in zip(ask, got):
                check(oracle, q, subs[at[rid]], mat, go, ge, al, (threshold, go, ge, form, rid))
            assert got[0] == got[4] == got[8] and got[1] == got[7]
            assert got[1] == {"score": 0, "q_begin": 0, "q_end": 0, "s_begin": 0, "s_end": 0, "ops": ""}
            assert "III" in got[0]["ops"] and got[0]["score"] > 200
    db.close()


# ---- 5. the ops buffer --------------------------------------------------------------------
@pytest.mark.parametrize("form", ["linear", "affine", "pssm"])
def test_ops_contract(sw, oracle, handle, form):
    """ops_stride below a path's length: the slot holds the path's first
    ops_stride ops (it replays from the begin cell), ops_len is the full
    length and the numbers do not change; no buffer at all: the same numbers
    and ops_len.  Three hits of different path lengths in one call."""
    go, ge = (5, 5) if form == "linear" else (11, 1)
    q = seam_query(120, 77)
    ins = np.array([4, 4, 4], dtype=np.uint8)  # C: not in seam_query's alphabet
    # a row deleted five rows in, so that the first 7 ops of that path are not its last 7
    subs = [q[30:50].copy(), np.concatenate([q[:5], q[6:60], q[64:]]), np.concatenate([q[10:70], ins, q[70:80]])]
    mat = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, *pack(subs))
    ids = [1, 0, 2]
    p = sw.Pssm(handle, derived(q, mat))

    def run(**kw):
        return db.align_pssm(p, ids, go, ge, **kw) if form == "pssm" else db.align(q, ids, mat, go, ge, **kw)

    full = run()
    for k, al in zip(ids, full):
        check(oracle, q, subs[k], mat, go, ge, al, (form, k))
    lens = [len(al["ops"]) for al in full]
    assert len(set(lens)) == 3 and min(lens) > 8, lens
    assert all("I" in al["ops"] or "D" in al["ops"] for al in full[::2])
    none = run(ops=False)
    for al, want in zip(none, full):
        assert al == dict(want, ops=None, ops_len=len(want["ops"]))
    for stride in (1, 7, min(lens) - 1, min(lens), max(lens) + 1):
        got = run(ops_stride=stride)
        for al, want in zip(got, full):
            assert al["ops_len"] == len(want["ops"]), (form, stride)
            assert [al[f] for f in NUMBERS] == [want[f] for f in NUMBERS], (form, stride)
            assert al["ops"] == want["ops"][:stride], (form, stride, al["ops"], want["ops"])
    # a slot holding the end of its path instead would show at strides 7 and min(lens) - 1
    for stride in (7, min(lens) - 1):
        assert any(al["ops"][:stride] != al["ops"][-stride:] for al in full), stride
    p.close()
    db.close()


# ---- 6. two launches at the real budget ------------------------------------------------------
def edited(q, rng, sub_phase, indels):
    """q with a substitution at every 50th residue from sub_phase and the
    indels [(position, rows deleted, columns inserted)] (descending positions)."""
    s = q.copy()
    at = np.arange(sub_phase, len(s), 50)
    s[at] = (s[at] + 1 + rng.integers(0, 19, size=len(at))) % 20
    for pos, cut, put in indels:
        s = np.concatenate([s[:pos], rng.integers(0, 20, size=put).astype(np.uint8), s[pos + cut:]])
    return s


def test_two_launches_at_the_budget(sw, oracle, handle):
    """A query of 16,383 residues against subjects A and B of 16,385 and C of
    102: a direction array of 536,887,296 bytes for A and for B, just over
    half of 2^30, so sw_align runs {A} and then {B, C} (swplan::align_groups;
    tests/test_hits_cpu.py test_align_groups), the second launch's results,
    ops and subjects at offsets past the first's.  A and B are the query under
    different substitutions and indels, so neither's path scores on the
    other.  The paths of A and B are checked by their own scores against the
    scan and the score-only oracle: the oracle's traceback of 268 M cells
    would need 4 bytes per cell."""
    rng = np.random.default_rng(16383)
    q = rng.integers(0, 20, size=16383).astype(np.uint8)
    a = edited(q, rng, 13, [(14000, 9, 0), (9000, 0, 9), (5000, 3, 0), (2000, 0, 5)])
    b = edited(q, rng, 37, [(15000, 2, 0), (11000, 0, 1), (7000, 0, 7), (3000, 4, 0)])
    c = np.concatenate([q[7000:7060], q[7062:7104]])
    subs = [a, b, c]
    assert [len(s) for s in subs] == [16385, 16385, 102]
    mat = sw.capi.builtin_matrix(1)
    go, ge = 11, 1
    res, offs = pack(subs)
    db = sw.Database(handle, res, offs)
    want = oracle.scan(q, res, offs, mat, go, ge)
    scores = db.scan(q, mat, go, ge)
    t0 = time.perf_counter()
    got = db.align(q, [0, 1, 2], mat, go, ge)
    print("sw_align, 16,383 x (16,385, 16,385, 102), two launches: %.2f s" % (time.perf_counter() - t0))
    db.close()
    for k, al in enumerate(got):
        assert al["score"] == scores[k] == want[k], (k, al["score"], scores[k], want[k])
        assert path_score(q, subs[k], mat, go, ge, al) == al["score"], k
    assert got[2] == oracle.align(q, c, mat, go, ge)
    for al in got[:2]:
        assert "I" in al["ops"] and "D" in al["ops"] and al["score"] > 60000 and len(al["ops"]) > 16000
    assert got[0]["ops"] != got[1]["ops"]
