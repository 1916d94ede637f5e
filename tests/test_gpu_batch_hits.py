"""GPU: batches of queries through the hit table (sw_scan_batch_topk,
sw_hit_stats_batch, sw_scan_batch_hits; csrc/sw_hits.hip with the query a
property of the hit).  Rows are compared with the rows the oracle's traceback
implies (tests/hits_support.py) and, where a case says so, with the
single-query calls.  The shapes are the smallest at which the mixed launch
can go wrong: queries of 0, 1, one chunk +- 1 and three chunks side by side,
two multi-chunk queries on one subject, an empty subject, duplicated pairs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO, read_query
from hits_support import FIELDS, expected, pack

pytestmark = pytest.mark.gpu
LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")
I64_MIN = np.iinfo(np.int64).min

# (matrix id, open, extend)
SCORINGS = {"b50-linear-2": (0, 2, 2), "b62-11-1": (1, 11, 1)}


def zero_row(rid, s_len=0):
    return dict(dict.fromkeys(FIELDS, 0), id=int(rid), s_len=int(s_len))


# ---- 1. mixed lengths in one launch -------------------------------------------
def layout_edges_subjects():
    """The 130 subjects of test_gpu_hits.test_layout_edges."""
    rng = np.random.default_rng(17)
    lens = [(1, 15, 16, 17, 33)[k % 5] for k in range(130)]
    lens[77] = 0
    subs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lens]
    rids = np.array([3 * k + 5 for k in range(130)], dtype=np.int32)
    return subs, rids


@pytest.fixture(scope="module")
def mixed(sw, oracle):
    """Queries, subjects and the oracle's rows of all 7 x 130 pairs under both gap models."""
    C = sw.capi.HITS_CHUNK_ROWS
    qlens = [0, 1, 40, C - 1, C, C + 1, 2 * C + 3]
    queries = [sw.synth.query(n, shard=60 + i) if n else np.zeros(0, np.uint8) for i, n in enumerate(qlens)]
    subs, rids = layout_edges_subjects()
    m = sw.capi.builtin_matrix(2)
    want = {(go, ge): [[expected(oracle, q, s, m, go, ge, rid) if len(q) and len(s) else zero_row(rid, len(s))
                        for s, rid in zip(subs, rids)] for q in queries]
            for go, ge in ((2, 2), (3, 1))}
    return queries, subs, rids, m, want


@pytest.mark.parametrize("threshold", [4096, 16])
def test_mixed_lengths_in_one_launch(sw, handle, mixed, threshold):
    queries, subs, rids, m, want = mixed
    res, offs = pack(subs)
    db = sw.Database(handle, res, offs, ids=rids, long_threshold=threshold)
    rng = np.random.default_rng(23)
    pairs = [(qi, k) for qi in range(len(queries)) for k in range(130)]
    order = list(rng.permutation(len(pairs))) + list(rng.integers(0, len(pairs), size=20))  # 20 duplicated pairs
    rng.shuffle(order)
    asked = [pairs[i] for i in order]
    for (go, ge), rows in want.items():
        got = db.hit_stats_batch(queries, [(qi, int(rids[k])) for qi, k in asked], m, go, ge)
        assert len(got) == len(asked) == 7 * 130 + 20
        for row, (qi, k) in zip(got, asked):
            assert row == rows[qi][k], (go, ge, qi, k, row, rows[qi][k])
        for row, (qi, k) in zip(got, asked):
            if qi == 0 or k == 77:  # the empty query, the empty subject
                assert row == zero_row(rids[k], len(subs[k]))
        assert any(row["score"] for row, (qi, k) in zip(got, asked) if qi == 6)
    db.close()


# ---- 2. the same subject under two multi-chunk queries --------------------------
def plant(q, lo, hi, del_at, ins_at):
    """q[lo:hi] without its 5 residues from del_at, with 5 foreign residues before ins_at."""
    assert lo <= min(del_at, ins_at) and max(del_at + 5, ins_at) <= hi and abs(del_at - ins_at) > 5
    parts = sorted([(del_at, "del"), (ins_at, "ins")])
    out, at = [], lo
    for pos, what in parts:
        out.append(q[at:pos])
        if what == "del":
            at = pos + 5
        else:
            out.append(((q[pos:pos + 5] + 7) % 20).astype(np.uint8))  # differs from the residues it displaces
            at = pos
    out.append(q[at:hi])
    return np.concatenate(out)


def test_two_multi_chunk_queries_on_the_same_subjects(sw, oracle, handle):
    """Every subject is scored by both queries in one launch: each (query,
    subject) pair has its own boundary row.  The planted copies carry their gap
    runs on, across or just before row C, so the alignment's counters cross the
    chunk seam through that row."""
    C = sw.capi.HITS_CHUNK_ROWS
    qa, qb = sw.synth.query(C + 1, shard=71), sw.synth.query(2 * C + 3, shard=72)
    pieces = [plant(qa, 10, C + 1, C - 60, C - 30),       # both runs in chunk 0, the tail crosses row C
              plant(qa, 10, C + 1, C - 100, C - 8),       # an insertion 8 rows above the seam
              plant(qa, 10, C + 1, C - 15, C - 200),      # a deletion ending 10 rows above the seam
              plant(qb, C - 300, C + 300, C - 2, C + 150),  # rows C-1 .. C+3 deleted: the run crosses row C
              plant(qb, C - 300, C + 300, C - 150, C),      # columns inserted between rows C and C + 1
              plant(qb, C - 350, C + 250, C - 5, C + 1)]    # the deleted run ends on row C
    subs = []
    for k, p in enumerate(pieces):
        pad = max(700 - len(p), 40)
        junk = sw.synth.residues(pad, shard=80 + k)
        subs.append(np.concatenate([junk[:pad // 2], p, junk[pad // 2:]]))
    assert all(650 <= len(s) <= 760 for s in subs)
    res, offs = pack(subs)
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, res, offs)
    queries = [qa, qb]
    pairs = [(qi, k) for k in range(6) for qi in (0, 1)]
    got = db.hit_stats_batch(queries, pairs, m, 11, 1)
    for row, (qi, k) in zip(got, pairs):
        want = expected(oracle, queries[qi], subs[k], m, 11, 1, k)
        assert row == want, (qi, k, row, want)
    for qi in (0, 1):
        single = db.hit_stats(queries[qi], list(range(6)), m, 11, 1)
        assert single == [row for row, (pq, _) in zip(got, pairs) if pq == qi]
    assert any(row["gap_opens"] >= 2 for row in got)
    # the planted pairs end beyond the first chunk
    assert sum(row["q_end"] > C and row["gap_opens"] >= 1 for row in got) >= 4
    db.close()


# ---- 3, 4. scan_batch_topk, scan_batch_hits -------------------------------------
@pytest.fixture(scope="module")
def searched(sw):
    r, o = sw.synth.database(400, shard=77)
    subs = [r[o[i]:o[i + 1]] for i in range(400)]
    queries = [sw.synth.query(200, shard=6), sw.synth.query(700, shard=7), np.zeros(0, np.uint8),
               np.random.default_rng(9).integers(0, 2, size=30).astype(np.uint8), subs[7].copy()]
    return r, o, subs, queries


@pytest.mark.parametrize("name", sorted(SCORINGS))
def test_scan_batch_topk(sw, handle, searched, name):
    mid, go, ge = SCORINGS[name]
    r, o, subs, queries = searched
    m = sw.capi.builtin_matrix(mid)
    db = sw.Database(handle, r, o)
    keys = db.scan_batch_topk(queries, 25, m, go, ge)
    assert keys.shape == (5, 25) and keys.dtype == np.int64
    scores = db.scan_batch(queries, m, go, ge)
    for qi, q in enumerate(queries):
        assert np.array_equal(keys[qi], db.scan_topk(q, 25, m, go, ge)), qi
        ids, vals = sw.capi.decode_keys(keys[qi])
        wi, wv = sw.capi.topk(scores[qi], 25)
        assert np.array_equal(ids, wi) and np.array_equal(vals, wv), qi
    assert list(sw.capi.decode_keys(keys[2])[0]) == list(range(25))  # the empty query: all 0, ids ascending
    assert sw.capi.decode_keys(keys[4])[0][0] == 7                   # the copy of subject 7
    big = db.scan_batch_topk(queries, 1000, m, go, ge)
    assert big.shape == (5, 1000) and np.all(big[:, 400:] == I64_MIN) and np.all(big[:, :400] != I64_MIN)
    assert np.array_equal(big[:, :25], keys)
    for k in (0, 4097):
        with pytest.raises(sw.capi.SWError):
            db.scan_batch_topk(queries, k, m, go, ge)
    none = db.scan_batch_topk([], 25, m, go, ge)
    assert none.shape == (0, 25)
    db.close()


@pytest.mark.parametrize("name", sorted(SCORINGS))
def test_scan_batch_hits(sw, oracle, handle, searched, name):
    mid, go, ge = SCORINGS[name]
    r, o, subs, queries = searched
    m = sw.capi.builtin_matrix(mid)
    db = sw.Database(handle, r, o)
    got = db.scan_batch_hits(queries, 25, m, go, ge)
    assert len(got) == 5 and all(len(rows) == 25 for rows in got)
    for qi, q in enumerate(queries):
        assert got[qi] == db.scan_hits(q, 25, m, go, ge), qi
        for row in got[qi][:5]:
            assert row == expected(oracle, q, subs[row["id"]], m, go, ge, row["id"]), (qi, row)
    assert got[2] == [zero_row(i, len(subs[i])) for i in range(25)]
    assert got[4][0]["id"] == 7 and got[4][0]["identities"] == len(subs[7]) == got[4][0]["length"]
    big = db.scan_batch_hits(queries, 1000, m, go, ge)
    assert [len(rows) for rows in big] == [400] * 5
    assert [rows[:25] for rows in big] == got
    assert db.scan_batch_hits([], 25, m, go, ge) == []
    for k in (0, 4097):
        with pytest.raises(sw.capi.SWError):
            db.scan_batch_hits(queries, k, m, go, ge)
    db.close()


# ---- 5. errors leave the handle usable ------------------------------------------
def test_errors_then_plain_calls(sw, oracle, handle, searched):
    r, o, subs, queries = searched
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, r, o)
    for pairs in ([(0, 1), (-1, 2)], [(len(queries), 3)], [(0, 400)], [(1, -1)]):
        with pytest.raises(sw.capi.SWError):
            db.hit_stats_batch(queries, pairs, m, 11, 1)
    assert db.hit_stats_batch(queries, [], m, 11, 1) == []
    q = queries[0]
    scores = db.scan(q, m, 11, 1)
    assert np.array_equal(scores, oracle.scan(q, r, o, m, 11, 1))
    for row in db.scan_hits(q, 5, m, 11, 1):
        assert row == expected(oracle, q, subs[row["id"]], m, 11, 1, row["id"])
    db.close()


# ---- 6. a database generated on the device ----------------------------------------
def test_synthetic_database(sw, handle):
    db = sw.Database.synthetic(handle, 11, 3000, id_base=5000)
    queries = [sw.synth.query(250, shard=3), sw.synth.query(600, shard=4)]
    m = sw.capi.builtin_matrix(1)
    got = db.scan_batch_hits(queries, 10, m, 11, 1)
    assert [len(rows) for rows in got] == [10, 10]
    for q, rows in zip(queries, got):
        assert rows == db.scan_hits(q, 10, m, 11, 1)
        assert all(row["score"] > 0 for row in rows)
    db.close()


# ---- 7. the CLI ------------------------------------------------------------------
def parse_blocks(stdout):
    """[(index, name, length, lines)] of a --queries run."""
    blocks = []
    for ln in stdout.split("\n"):
        if ln.startswith("# query "):
            _, _, idx, name, length = ln.split(" ")
            blocks.append((int(idx), name, int(length), []))
        elif ln.startswith("=" * 80):
            break
        elif blocks and ln:
            blocks[-1][3].append(ln)
    return blocks


def test_cli_queries(sw, handle, tmp_path):
    recs = []
    for line in open(GOLDEN + "/subset111.fasta"):
        if line.startswith(">"):
            recs.append("")
        else:
            recs[-1] += line.strip()
    subs = [sw.encode(s) for s in recs]
    res, offs = pack(subs)
    seqs = [read_query("P01008"), read_query("P02232"), read_query("P01008")[:60]]
    names = ["sp|P01008|ANT3_HUMAN", "P02232", "head60"]
    fasta = tmp_path / "queries.fasta"
    fasta.write_text(">%s Antithrombin-III\n%s\n\n>%s\n%s\n>%s first residues\n%s\n" % (
        names[0], "\n".join(seqs[0][i:i + 60] for i in range(0, len(seqs[0]), 60)), names[1], seqs[1], names[2], seqs[2]))
    m = sw.capi.builtin_matrix(1)
    db = sw.Database(handle, res, offs)
    want_rows = [db.scan_hits(sw.encode(s), 5, m, 11, 1) for s in seqs]
    want_keys = [sw.capi.decode_keys(db.scan_topk(sw.encode(s), 5, m, 11, 1)) for s in seqs]
    db.close()
    swdb = str(tmp_path / "subset111.swdb")
    made = subprocess.run([os.path.join(LIB, "main"), "--db", GOLDEN + "/subset111.fasta", "--make-db", swdb],
                          capture_output=True, text=True, timeout=300)
    assert made.returncode == 0, made.stderr
    base = [os.path.join(LIB, "main"), "--queries", str(fasta), "--matrix", "blosum62", "--gap-open", "11", "--gap-extend", "1"]
    outs = {}
    for dbname, dbpath in (("fasta", GOLDEN + "/subset111.fasta"), ("swdb", swdb)):
        for mode in ("--hits", "--topk"):
            out = subprocess.run(base + ["--db", dbpath, mode, "5"], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            assert "Input queries: 3 sequences, %d residues" % sum(map(len, seqs)) in out.stdout
            assert "Query length: %d chars." % sum(map(len, seqs)) in out.stdout
            blocks = parse_blocks(out.stdout)
            assert [(b[0], b[1], b[2]) for b in blocks] == [(i, names[i], len(seqs[i])) for i in range(3)]
            outs[dbname, mode] = [b[3] for b in blocks]
    for dbname in ("fasta", "swdb"):
        for qi in range(3):
            rows = [dict(zip(FIELDS, map(int, ln.split("\t")))) for ln in outs[dbname, "--hits"][qi]]
            assert rows == want_rows[qi], (dbname, qi)
            pairs = [tuple(map(int, ln.split(":"))) for ln in outs[dbname, "--topk"][qi]]
            assert pairs == list(zip(map(int, want_keys[qi][0]), map(int, want_keys[qi][1]))), (dbname, qi)
    assert outs["fasta", "--hits"] == outs["swdb", "--hits"] and outs["fasta", "--topk"] == outs["swdb", "--topk"]


# ---- 8. the single forms are the batch forms of one query ---------------------------
def raw(obj):
    return bytes(memoryview(obj).cast("B"))


@pytest.mark.parametrize("name", sorted(SCORINGS))
def test_single_forms_equal_one_query_batches(sw, handle, name):
    """sw_scan_hits_sig against sw_scan_batch_hits_sig and sw_scan_topk against
    sw_scan_batch_topk at nq = 1, byte for byte: rows, sig, calib, nhits and
    keys.  k is larger than the 130 subjects, so the slots past nhits (the
    caller's bytes, here a pattern) and the keys' padding are compared too."""
    capi = sw.capi
    L = capi.lib()
    mid, go, ge = SCORINGS[name]
    subs, rids = layout_edges_subjects()
    res, offs = pack(subs)
    db = sw.Database(handle, res, offs, ids=rids)
    q = np.random.default_rng(31).integers(0, 4, size=40).astype(np.uint8)
    qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    qoffs = np.array([0, len(q)], dtype=np.int64)
    op = qoffs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    scoring = capi._ScoringArg(capi.builtin_matrix(mid), go, ge)
    k = 200
    got = {}
    for form in ("single", "batch"):
        hits, sigs, cal, nhits = (capi.Hit * k)(), (capi.Sig * k)(), capi.Calib(), ctypes.c_int32(-7)
        keys = np.full(k, 0x5a5a5a5a5a5a5a5a, dtype=np.int64)
        for buf in (hits, sigs, cal):
            ctypes.memset(ctypes.addressof(buf), 0xa5, ctypes.sizeof(buf))
        kp = keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        if form == "single":
            rc = L.sw_scan_hits_sig(handle.ptr, db.ptr, qp, len(q), scoring.ptr(), k, hits, sigs, ctypes.byref(nhits),
                                    ctypes.byref(cal))
            rk = L.sw_scan_topk(handle.ptr, db.ptr, qp, len(q), scoring.ptr(), k, kp)
        else:
            rc = L.sw_scan_batch_hits_sig(handle.ptr, db.ptr, qp, op, 1, scoring.ptr(), k, hits, sigs,
                                          ctypes.byref(nhits), ctypes.byref(cal))
            rk = L.sw_scan_batch_topk(handle.ptr, db.ptr, qp, op, 1, scoring.ptr(), k, kp)
        assert (rc, rk) == (0, 0), (form, L.sw_last_error())
        got[form] = (raw(hits), raw(sigs), raw(cal), nhits.value, keys.tobytes())
    assert got["single"][3] == 130
    for what, a, b in zip(("rows", "sig", "calib", "nhits", "keys"), got["single"], got["batch"]):
        assert a == b, what
    rows = (capi.Hit * k).from_buffer_copy(got["single"][0])
    assert any(rows[i].score > 0 for i in range(130)) and raw(rows)[130 * ctypes.sizeof(capi.Hit):] == \
        b"\xa5" * (70 * ctypes.sizeof(capi.Hit))
    keys = np.frombuffer(got["single"][4], dtype=np.int64)
    assert np.all(keys[130:] == I64_MIN) and np.all(keys[:130] != I64_MIN)
    db.close()
