"""GPU: the hit table (sw_hit_stats / sw_scan_hits, csrc/sw_hits.hip).  Every
row is compared with the row the oracle's traceback implies
(tests/hits_support.py: spans, ops length, identities and positives by
replaying the ops, runs for gap_opens, all-zero for a score of 0), and with
Database.align on the same ids where the case says so."""
import os
import subprocess

import numpy as np
import pytest

import align_support
from conftest import GOLDEN, REPO
from hits_support import FIELDS, expected, pack, row_of, seam_query, seam_subjects

pytestmark = pytest.mark.gpu
LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")

# (matrix id, open, extend)
SCORINGS = {"b50-linear-2": (0, 2, 2), "b62-11-1": (1, 11, 1), "b62-12-1": (1, 12, 1), "id3-linear-2": (2, 2, 2)}


def check_rows(oracle, got, q, subs, ids_of, mat, go, ge):
    """got[k] is the row of subject ids_of[k] = (result id, subject index)."""
    assert len(got) == len(ids_of)
    for row, (rid, k) in zip(got, ids_of):
        want = expected(oracle, q, subs[k], mat, go, ge, rid)
        assert row == want, (rid, k, row, want)


@pytest.mark.parametrize("threshold", [None, 64, 4096])
@pytest.mark.parametrize("name", sorted(SCORINGS))
def test_top_hits_and_ends(sw, oracle, handle, name, threshold):
    """Top hits plus the first and last subject of a 400-subject database,
    with the subjects in the long layout (64), the inter layout (4096) and
    the library's own split: equal to the oracle's rows, to the scan's scores
    and to Database.align field for field."""
    mid, go, ge = SCORINGS[name]
    r, o = sw.synth.database(400, shard=31 + mid)
    subs = [r[o[i]:o[i + 1]] for i in range(400)]
    q = sw.synth.query(300, shard=5 + go)
    m = sw.capi.builtin_matrix(mid)
    db = sw.Database(handle, r, o, long_threshold=threshold)
    st = db.stats()
    if threshold == 64:
        assert st["n_long"] > 300
    if threshold == 4096:
        assert st["n_long"] < 10 and st["n_blocks"] >= 6
    scores = db.scan(q, m, go, ge)
    ids, _ = sw.capi.topk(scores, 25)
    ids = [int(i) for i in ids] + [0, 399]
    got = db.hit_stats(q, ids, m, go, ge)
    check_rows(oracle, got, q, subs, [(i, i) for i in ids], m, go, ge)
    als = db.align(q, ids, m, go, ge)
    for row, al, i in zip(got, als, ids):
        assert row["score"] == scores[i]
        assert row == row_of(al, q, subs[i], m, i), (i, row, al)
    db.close()


@pytest.mark.parametrize("threshold", [4096, 16])
def test_layout_edges(sw, oracle, handle, threshold):
    """Lanes 0 and 63 and a partly filled last block; lengths 1, 15, 16, 17,
    33 around the 16-column groups; an empty subject; custom ids; an unknown
    id; an empty query; no ids."""
    rng = np.random.default_rng(17)
    lens = [(1, 15, 16, 17, 33)[k % 5] for k in range(130)]
    lens[77] = 0
    subs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lens]
    res, offs = pack(subs)
    rids = np.array([3 * k + 5 for k in range(130)], dtype=np.int32)
    db = sw.Database(handle, res, offs, ids=rids, long_threshold=threshold)
    st = db.stats()
    if threshold == 4096:
        assert st["n_long"] == 0 and st["n_blocks"] == 3  # 64 + 64 + 2 lanes
    else:
        assert st["n_long"] == 52  # the subjects of 17 and 33 residues
    q = rng.integers(0, 4, size=40).astype(np.uint8)
    m = sw.capi.builtin_matrix(2)
    for go, ge in ((2, 2), (3, 1)):
        got = db.hit_stats(q, rids, m, go, ge)
        check_rows(oracle, got, q, subs, [(int(rids[k]), k) for k in range(130)], m, go, ge)
        assert got[77] == dict(dict.fromkeys(FIELDS, 0), id=int(rids[77]))
        assert any(row["gaps"] for row in got)
    with pytest.raises(sw.capi.SWError):
        db.hit_stats(q, [4])  # not an id of this database
    empty = db.hit_stats(np.zeros(0, np.uint8), rids[:3], m)
    assert empty == [dict(dict.fromkeys(FIELDS, 0), id=int(rids[k]), s_len=lens[k]) for k in range(3)]
    assert db.hit_stats(q, [], m) == []
    db.close()


@pytest.mark.parametrize("go,ge", [(5, 5), (12, 1)])
@pytest.mark.parametrize("rows", ["C-1", "C", "C+1", "2C+3"])
def test_seams(sw, oracle, handle, rows, go, ge):
    """Gap runs across the lane seams (rows RI t, t = 1, 2, 32, 63, of the
    first and the last wave of every chunk), the wave seams (the LDS rings) and
    the chunk seams (the boundary row in device memory): the smallest inputs
    in which a tuple dropped at a hand-over changes gap_opens, length or a
    begin cell while the score stays right."""
    C, ri, waves = sw.capi.HITS_CHUNK_ROWS, sw.capi.HITS_ROWS_PER_LANE, sw.capi.HITS_WAVES
    wrows = 64 * ri  # query rows of a wave
    qlen = {"C-1": C - 1, "C": C, "C+1": C + 1, "2C+3": 2 * C + 3}[rows]
    q = seam_query(qlen, 20260 + qlen)
    seams = []
    for c0 in range(0, qlen, C):
        seams += [c0 + w0 + ri * t for w0 in (0, (waves - 1) * wrows) for t in (1, 2, 32, 63)]
        seams += [c0 + w * wrows for w in range(1, waves)]
    seams += list(range(C, qlen, C))
    subs = seam_subjects(q, [s for s in seams if s < qlen])
    res, offs = pack(subs)
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, res, offs)
    ids = list(range(len(subs)))
    got = db.hit_stats(q, ids, m, go, ge)
    check_rows(oracle, got, q, subs, [(i, i) for i in ids], m, go, ge)
    assert sum(row["gap_opens"] == 1 and row["gaps"] in (1, 2, 5) for row in got) > len(subs) // 2
    db.close()


def test_ties(sw, oracle, handle):
    """200 subjects over a 2-letter alphabet against tie-heavy queries."""
    rng = np.random.default_rng(3)
    subs = [rng.integers(0, 2, size=int(rng.integers(1, 61))).astype(np.uint8) for _ in range(200)]
    res, offs = pack(subs)
    m = sw.capi.builtin_matrix(2)
    ids = list(range(200))
    for thr in (4096, 8):
        db = sw.Database(handle, res, offs, long_threshold=thr)
        for go, ge in ((2, 2), (3, 3), (3, 1)):
            q = rng.integers(0, 2, size=int(rng.integers(20, 61))).astype(np.uint8)
            check_rows(oracle, db.hit_stats(q, ids, m, go, ge), q, subs, [(i, i) for i in ids], m, go, ge)
        db.close()


@pytest.mark.parametrize("name", sorted(align_support.SCORINGS))
def test_tie_set(sw, oracle, handle, name):
    """The traceback's tie set (tests/align_support.py; tests/
    test_align_inputs.py shows that its pairs tell the tie rules apart, which
    test_ties' scorings, with 2 gap >= |mismatch|, cannot for left before up):
    every row from both layouts."""
    mat, go, ge = align_support.scoring(name)
    groups = align_support.TIE_GROUPS[align_support.SCORINGS[name][0]]
    for thr in (4096, 8):
        for q, subs in groups[::2] if thr == 8 else groups:
            db = sw.Database(handle, *pack(subs), long_threshold=thr)
            ids = list(range(len(subs)))
            check_rows(oracle, db.hit_stats(q, ids, mat, go, ge), q, subs, [(i, i) for i in ids], mat, go, ge)
            db.close()


def test_size(sw, oracle, handle):
    """A query of three chunks against three subjects of about 12,000
    residues, one with a planted copy of the query with indels."""
    rng = np.random.default_rng(8)
    q = sw.synth.query(1500, shard=12)
    r = sw.synth.residues(36000, shard=4)
    subs = [r[:11950].copy(), r[11950:24010].copy(), r[24010:36000].copy()]
    planted = np.concatenate([q[:400], q[430:900], rng.integers(0, 20, size=25).astype(np.uint8), q[900:]])
    subs[1][5000:5000 + len(planted)] = planted
    res, offs = pack(subs)
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, res, offs)
    got = db.hit_stats(q, [0, 1, 2], m, 11, 1)
    check_rows(oracle, got, q, subs, [(i, i) for i in range(3)], m, 11, 1)
    assert got[1]["gap_opens"] >= 2 and got[1]["length"] > 1400
    db.close()


def test_scan_hits(sw, oracle, handle):
    r, o = sw.synth.database(400, shard=77)
    q = sw.synth.query(200, shard=6)
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, r, o)
    keys = db.scan_topk(q, 25, m, 11, 1)
    ids = [int(i) for i in sw.capi.decode_keys(keys)[0]]
    got = db.scan_hits(q, 25, m, 11, 1)
    assert [row["id"] for row in got] == ids
    assert got == db.hit_stats(q, ids, m, 11, 1)
    subs = [r[o[i]:o[i + 1]] for i in range(400)]
    check_rows(oracle, got, q, subs, [(i, i) for i in ids], m, 11, 1)
    assert len(db.scan_hits(q, 1000, m, 11, 1)) == 400
    for k in (0, 4097):
        with pytest.raises(sw.capi.SWError):
            db.scan_hits(q, k, m, 11, 1)
    db.close()


def test_scan_hits_4096(sw, handle):
    """k = 4096 on 5,000 short subjects equals Database.align on the same ids."""
    rng = np.random.default_rng(5)
    q = sw.synth.query(120, shard=2)
    subs = [rng.integers(0, 20, size=int(rng.integers(1, 201))).astype(np.uint8) for _ in range(5000)]
    for k in range(0, 5000, 50):  # some related subjects
        a = int(rng.integers(0, 60))
        piece = np.concatenate([q[a:a + 20], q[a + 23:a + 60]])
        subs[k] = np.concatenate([subs[k][:50], piece])[:200]
    res, offs = pack(subs)
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, res, offs)
    got = db.scan_hits(q, 4096, m, 11, 1)
    assert len(got) == 4096
    ids = [row["id"] for row in got]
    als = db.align(q, ids, m, 11, 1)
    for row, al in zip(got, als):
        assert row == row_of(al, q, subs[row["id"]], m, row["id"])
    assert any(row["gaps"] for row in got)
    db.close()


def test_synthetic_database(sw, oracle, handle):
    """A database generated on the device: the rows of the top 20 equal the
    oracle's on the residues regenerated by synth.counter_residues."""
    seed, base, n = 11, 5000, 3000
    db = sw.Database.synthetic(handle, seed, n, id_base=base)
    q = sw.synth.query(250, shard=3)
    m = sw.capi.builtin_matrix(1)
    got = db.scan_hits(q, 20, m, 11, 1)
    assert len(got) == 20
    L, lut = sw.capi.synth_tables()
    for row in got:
        gid = np.array([base + row["id"]], dtype=np.int64)
        n_res = int(sw.synth.counter_lengths(seed, gid, L)[0])
        s = sw.synth.counter_residues(seed, int(gid[0]), n_res, lut)
        assert row == expected(oracle, q, s, m, 11, 1, row["id"])
    db.close()


def test_cli_hits(sw, handle):
    """main --hits 10 prints what scan_hits returns (the C++ layer's
    smith_waterman_cuda_hits under the flags' scoring)."""
    recs = []
    for line in open(GOLDEN + "/subset111.fasta"):
        if line.startswith(">"):
            recs.append("")
        else:
            recs[-1] += line.strip()
    subs = [sw.encode(s) for s in recs]
    res, offs = pack(subs)
    from conftest import read_query
    q = sw.encode(read_query("P01008"))
    db = sw.Database(handle, res, offs)
    want = db.scan_hits(q, 10, sw.capi.builtin_matrix(1), 11, 1)
    db.close()
    out = subprocess.run([os.path.join(LIB, "main"), "--query", GOLDEN + "/queries/P01008.fasta", "--db",
                          GOLDEN + "/subset111.fasta", "--hits", "10", "--matrix", "blosum62", "--gap-open", "11",
                          "--gap-extend", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [ln.split("\t") for ln in out.stdout.split("\n") if ln.count("\t") == len(FIELDS) - 1]
    assert [dict(zip(FIELDS, map(int, r))) for r in rows] == want
    assert not [ln for ln in out.stdout.split("\n") if ln and ln[0].isdigit() and ":" in ln], "no id:score lines"
