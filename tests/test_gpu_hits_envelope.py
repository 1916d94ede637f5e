"""GPU: the hit table (csrc/sw_hits.hip) and the traceback (csrc/sw_align.hip)
over all 25 residue codes at the edges of the scoring envelope, field by field
against the CPU oracle.

sw_hits builds its own LDS profile in stored-code order and counts identities
on stored codes; it carries nine words per DP value across lanes, waves (the
LDS rings) and chunks (device memory), and reduces the best cell by (value,
row, column) across threads, waves and chunks.  The inputs
(tests/hits_envelope_support.py) are the ones tests/test_hits_envelope_inputs.py
shows to tell a transposed or mis-mapped profile, 16-bit values, a wrong
reduction order and a tuple dropped at a subject-column seam from the right
kernel: matrices that are not symmetric with entries to +-100, gaps to 1000
and an open below the extend, identities that are not positives, queries of
40 rows to three chunks, about 150 subjects.

The oracle's alignments are computed once per (scoring, query).  No tolerance
anywhere: every comparison is == on whole row dicts or alignments."""
import numpy as np
import pytest

import hits_envelope_support as hes
from conftest import path_score
from hits_envelope_support import SCORINGS
from hits_support import row_of

pytestmark = pytest.mark.gpu

LAYOUTS = {"lanes": 4096, "long": 16, "split": None}  # long_threshold


@pytest.fixture(scope="module")
def env(sw, oracle, handle):
    e = hes.build_inputs(sw)
    e.want = hes.Want(oracle, e)
    e.ids = list(range(len(e.subs)))
    e.db = {name: sw.Database(handle, e.res, e.offs, long_threshold=t) for name, t in LAYOUTS.items()}
    st = {name: d.stats() for name, d in e.db.items()}
    assert st["lanes"]["n_long"] == 0 and st["lanes"]["n_blocks"] >= 3
    assert st["long"]["n_long"] == sum(len(s) > 16 for s in e.subs) > len(e.subs) - 20
    assert 0 < st["split"]["n_long"] < len(e.subs)
    yield e
    for d in e.db.values():
        d.close()


def top_ids(rows, k):
    """The oracle's k best ids: score descending, id ascending."""
    return sorted(range(len(rows)), key=lambda i: (-rows[i]["score"], i))[:k]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("scname", list(SCORINGS))
def test_rows(env, handle, scname, layout):
    """Every subject's row under every query, from the lane layout, the long
    layout and the library's split; the scores are the scan's (d100-40-28 in
    the long layout: the planted copy of the 1,100-row query scores 110,000,
    past fp16's largest number in sw_intra_x2, which has to flag it)."""
    mk, go, ge = SCORINGS[scname]
    m, db = env.mats[mk], env.db[layout]
    for qi, q in enumerate(env.queries):
        want = env.want.rows(scname, qi)
        got = db.hit_stats(q, env.ids, m, go, ge)
        assert len(got) == len(want)
        for k, (row, w) in enumerate(zip(got, want)):
            assert row == w, (scname, layout, len(q), k, row, w)
        scores = db.scan(q, m, go, ge)
        assert scores.tolist() == [w["score"] for w in want], (scname, layout, len(q))
        if (scname, layout) == ("d100-40-28", "long"):
            assert handle.last_intra_kernel().startswith("sw_intra_x2<"), handle.last_intra_kernel()
    if mk == "nonpos":
        assert not any(w["score"] for w in want)


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_align_agrees(env, scname):
    """sw_align on ALL subjects, two rows past the first wave seam and at
    three chunks: the oracle's alignment, the hit table's row, and a path
    that scores what is reported (a run's further residues at min(open,
    extend): with open below extend the recurrence re-opens from H)."""
    mk, go, ge = SCORINGS[scname]
    m, db = env.mats[mk], env.db["split"]
    for qi in (1, len(env.queries) - 1):
        q = env.queries[qi]
        got = db.align(q, env.ids, m, go, ge)
        rows = db.hit_stats(q, env.ids, m, go, ge)
        for k, (al, w, row) in enumerate(zip(got, env.want.als(scname, qi), rows)):
            assert al == w, (scname, len(q), k, al, w)
            assert row == row_of(al, q, env.subs[k], m, k), (scname, len(q), k, row, al)
            if al["score"]:
                assert path_score(q, env.subs[k], m, go, min(go, ge), al) == al["score"], (scname, len(q), k)


@pytest.mark.parametrize("scname", ["asym-1-4", "pm100-1000-1000", "d100-40-28"])
def test_batch(env, scname):
    """One sw_hit_stats_batch launch over all five queries, neighbouring hits
    of different queries (one-chunk beside multi-chunk hits); sw_scan_hits and
    sw_scan_batch_hits: the oracle's 25 best ids and their rows."""
    mk, go, ge = SCORINGS[scname]
    m, db = env.mats[mk], env.db["split"]
    nq = len(env.queries)
    pairs = [(qi, k) for k in env.ids for qi in range(nq)]
    assert all(a[0] != b[0] for a, b in zip(pairs, pairs[1:]))
    got = db.hit_stats_batch(env.queries, pairs, m, go, ge)
    assert len(got) == len(pairs)
    for row, (qi, k) in zip(got, pairs):
        assert row == env.want.rows(scname, qi)[k], (scname, qi, k, row)
    batch = db.scan_batch_hits(env.queries, 25, m, go, ge)
    assert len(batch) == nq
    for qi, q in enumerate(env.queries):
        want = env.want.rows(scname, qi)
        top = [want[i] for i in top_ids(want, 25)]
        assert db.scan_hits(q, 25, m, go, ge) == top, (scname, qi)
        assert batch[qi] == top, (scname, qi)


def test_custom_ids(sw, handle, env):
    """Result ids that are not the subjects' positions (3 k + 5)."""
    mk, go, ge = SCORINGS["asym-7-3"]
    m = env.mats[mk]
    rids = np.array([3 * k + 5 for k in env.ids], dtype=np.int32)
    db = sw.Database(handle, env.res, env.offs, ids=rids)
    for qi, q in enumerate(env.queries):
        want = [dict(w, id=int(rids[k])) for k, w in enumerate(env.want.rows("asym-7-3", qi))]
        assert db.hit_stats(q, rids, m, go, ge) == want, qi
        back = db.hit_stats(q, rids[::-1], m, go, ge)
        assert back == want[::-1], qi
        top = [want[i] for i in top_ids(want, 25)]
        assert db.scan_hits(q, 25, m, go, ge) == top, qi
    with pytest.raises(sw.capi.SWError):
        db.hit_stats(env.queries[0], [4], m, go, ge)  # not an id of this database
    db.close()
