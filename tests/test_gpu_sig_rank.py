"""GPU: the ranking by E-value (include/sw_amd.h "ranking by E-value";
csrc/sw_sigkeys.hip sw_sig_keys, sw_sig_gather; sw_sig_topk_device and the
_ranked scan forms; main --rank evalue).  Keys and counts must equal the numpy
restatement (tests/rank_support.py) exactly, with the adjustment table taken
from the library (sw_sig_rank_table), so a last-bit difference between two
`log` implementations cannot make a test flaky; scores come from the oracle.

(tests/test_gpu_rank.py is the score ranking's: sw_topk_device.)"""
import os
import subprocess

import numpy as np
import pytest

import calib_support as cs
import rank_support as rs
from conftest import GOLDEN, REPO, read_query
from hits_support import FIELDS, pack

pytestmark = pytest.mark.gpu
LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")
CALIB_FIELDS = ("size", "status", "qlen", "fits", "n_db", "n_fit", "n_clipped", "n_skipped", "a", "c", "sigma")
FILL = 0x7f7f7f7f
SCORINGS = [(11, 1), (6, 6)]


def same_calib(a, b):
    return [getattr(a, f) for f in CALIB_FIELDS] == [getattr(b, f) for f in CALIB_FIELDS]


def device_scores(db, q, m, go, ge):
    """A torch int32 buffer of n_out slots pre-filled with 0x7f7f7f7f, after
    sw_scan_device (which writes only the slots a subject maps to)."""
    import torch
    d = torch.full((max(db.n_out, 1),), FILL, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    db.scan_device(q, d.data_ptr(), m, go, ge)
    torch.cuda.synchronize()
    return d


def cutoffs(r, k):
    """r_min values taken from the restated r so that 0, 1, k - 1, k, k + 1
    subjects pass (as far as the database and ties allow), and no cutoff."""
    srt = np.sort(np.asarray(r, dtype=np.int64))[::-1]
    out = {rs.R_FLOOR, int(srt[0]) + 1}
    for m in (1, k - 1, k, k + 1):
        if 1 <= m <= len(srt):
            out.add(int(srt[m - 1]))
    return sorted(out)


@pytest.fixture(scope="module")
def edge(sw, oracle):
    """tests/test_gpu_calib.py's edge database: about 300 subjects at the
    length bin's edges (0, 1, 2, 3, 4, 5, 7, 8, and 2^k - 1, 2^k, 5 * 2^(k-2)
    for k <= 11), three copies of a 120-residue query among them, result ids
    3 * perm(i) + 1, and the oracle's scores per (query, scoring), with each
    scan's calibration (the fit of the numpy table of those scores)."""
    rng = np.random.default_rng(2026)
    lens = [0, 1, 2, 3, 4, 5, 7, 8]
    for k in range(2, 12):
        lens += [2 ** k - 1, 2 ** k, 5 * 2 ** (k - 2)]
    lens = lens + [0] + [int(v) for v in rng.choice(lens[1:], 300 - 3 - len(lens) - 1)]
    q120 = sw.synth.query(120, shard=41)
    subs = [sw.synth.residues(n, shard=1000 + i) if n else np.zeros(0, np.uint8) for i, n in enumerate(lens)]
    subs += [q120.copy() for _ in range(3)]
    order = rng.permutation(len(subs))
    subs = [subs[i] for i in order]
    res, offs = pack(subs)
    ids = (3 * rng.permutation(len(subs)) + 1).astype(np.int32)
    queries = {0: np.zeros(0, np.uint8), 40: sw.synth.query(40, shard=42), 120: q120, 600: sw.synth.query(600, shard=43)}
    m = oracle.matrix(oracle.MATRIX_BLOSUM62)
    L = np.diff(offs)
    want, cal = {}, {}
    for go, ge in SCORINGS:
        for n, q in queries.items():
            s = oracle.scan(q, res, offs, m, go, ge) if n else np.zeros(len(subs), np.int32)
            s.setflags(write=False)
            want[n, go, ge] = s
            cal[n, go, ge] = sw.capi.calib_fit(cs.table(s, L), n)
            cal[n, go, ge].n_skipped = int((L == 0).sum())
    e = {"res": res, "offs": offs, "ids": ids, "L": L, "queries": queries, "m": m, "want": want, "cal": cal}
    # the fixture's condition: what the feature does that a score ranking cannot
    adj = sw.capi.sig_rank_table(cal[600, 11, 1], int(L.max()))
    by_r = rs.key_ids(rs.ranked(want[600, 11, 1], L, ids, adj, rs.R_FLOOR, 12)[0])
    by_s = sw.capi.decode_keys(sw.dist.local_topk(np.asarray(want[600, 11, 1]), ids, 12))[0]
    e["differ"] = len(set(by_r.tolist()) ^ set(int(v) for v in by_s)) // 2
    assert e["differ"] >= 3, (by_r, by_s)
    return e


@pytest.mark.parametrize("go,ge", SCORINGS)
def test_edge_database(sw, handle, edge, go, ge):
    """Both layouts hold subjects; every query length; k at 1, 12, n, n + 5
    (padding) and 4096; cutoffs that pass exactly 0, 1, k - 1, k, k + 1
    subjects; an adjustment table shorter than the longest subject."""
    L, ids, n = edge["L"], edge["ids"], len(edge["L"])
    db = sw.Database(handle, edge["res"], edge["offs"], ids=ids, long_threshold=64)
    st = db.stats()
    assert st["n_long"] > 50 and st["n_blocks"] >= 1 and db.n_out > 2 * n
    for qn, q in edge["queries"].items():
        want, cal = edge["want"][qn, go, ge], edge["cal"][qn, go, ge]
        d = device_scores(db, q, edge["m"], go, ge)
        got = d.cpu().numpy()
        # (an empty query's scan zeroes the whole row; any other writes the mapped slots only)
        assert np.array_equal(got[ids], want) and int((got == FILL).sum()) == (db.n_out - n if qn else 0)
        H = db.score_hist(d.data_ptr())
        fit = sw.capi.calib_fit(H, qn)
        fit.n_skipped = 2
        assert same_calib(fit, cal)
        for max_len in (int(L.max()), 100):
            adj = sw.capi.sig_rank_table(cal, max_len)
            r = rs.rank_values(want, L, adj)
            for k in ((1, 12, n, n + 5, 4096) if max_len > 100 else (12,)):
                for r_min in cutoffs(r, k):
                    keys, count = db.sig_topk(d.data_ptr(), adj, r_min, k)
                    wk, wc = rs.select(rs.keys(r, ids, r_min), k), rs.count(r, r_min)
                    assert count == wc and np.array_equal(keys, wk), (qn, max_len, k, r_min, count, wc)
        if qn == 0:
            assert cal.status & cs.DEGENERATE and np.all(r == rs.R_FLOOR)
    db.close()


def test_hand_written_scores(sw, handle):
    """Scores -2^31 .. INT32_MAX, lengths including 0 and one past the table,
    adjustments INT32_MIN and INT32_MAX (both ends of r's range), equal r
    values broken by id, result ids with gaps and the unmapped slots holding
    0x7f7f7f7f."""
    import torch
    i32 = np.iinfo(np.int32)
    adj = np.array([0, 0, i32.min, 100, 4096, i32.max, 7, -4096, 0, 12345], dtype=np.int32)
    case = [(-2 ** 31, 1), (-1, 2), (0, 3), (1, 3), (2 ** 20 - 1, 2), (2 ** 20, 2), (i32.max, 5), (1, 5), (50, 0),
            (5, 4), (3, 7), (7, 4000), (1, 2), (i32.max, 2), (2 ** 20 - 1, 8), (2 ** 20, 1), (9, 9), (9, 10), (1, 1)]
    s = np.array([c[0] for c in case], dtype=np.int32)
    L = np.array([c[1] for c in case], dtype=np.int64)
    n = len(case)
    ids = (3 * np.random.default_rng(4).permutation(n) + 1).astype(np.int32)
    res, offs = pack([np.zeros(v, np.uint8) for v in L])
    db = sw.Database(handle, res, offs, ids=ids)
    slots = np.full(db.n_out, FILL, dtype=np.int32)
    slots[ids] = s
    d = torch.from_numpy(slots).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    r = rs.rank_values(s, L, adj)
    assert (r == rs.R_CEIL).sum() == 3 and (r == rs.R_FLOOR).sum() == 4 and r[7] == 4096 - i32.max
    assert r[9] == r[10] == 4 * 4096 and r[16] == r[17] == r[11] + 2 * 4096  # ties; lengths past the table
    for k in (1, 5, n, n + 3, 4096):
        for r_min in (rs.R_FLOOR, rs.R_FLOOR + 1, 4096 - i32.max, 4 * 4096, 4 * 4096 + 1, rs.R_CEIL, rs.R_NONE):
            keys, count = db.sig_topk(d.data_ptr(), adj, r_min, k)
            assert count == rs.count(r, r_min), (k, r_min)
            assert np.array_equal(keys, rs.select(rs.keys(r, ids, r_min), k)), (k, r_min)
    keys, count = db.sig_topk(d.data_ptr(), adj, rs.R_FLOOR, n)
    got = rs.key_ids(keys).tolist()
    assert count == n and got[:3] == sorted(ids[[4, 5, 13]].tolist()) and got[-4:] == sorted(ids[[0, 1, 2, 8]].tolist())
    lo, hi = sorted([int(ids[9]), int(ids[10])])  # equal r: the lower id first, next to each other
    assert got.index(lo) + 1 == got.index(hi)
    db.close()


def test_many_workgroups(sw, handle):
    """Database.synthetic(70000), a 40-residue query: 69 workgroups of the
    key pass (the last one partly filled) add to one counter; keys against the restatement of the
    downloaded scores; a cutoff that about 1,000 subjects pass (more than k)."""
    n = 70000
    db = sw.Database.synthetic(handle, 7, n)
    d = device_scores(db, sw.synth.query(40, shard=42), sw.capi.builtin_matrix(1), 11, 1)
    scores = d.cpu().numpy()[:n]
    L = sw.capi.synth_lengths(7, 0, n)
    cal = sw.capi.calib_fit(db.score_hist(d.data_ptr()), 40)
    assert cal.status == 0
    adj = sw.capi.sig_rank_table(cal, int(L.max()))
    ids = np.arange(n)
    r = rs.rank_values(scores, L, adj)
    r1000 = int(np.sort(r)[::-1][999])
    for k, r_min in ((100, rs.R_FLOOR), (100, r1000), (4096, r1000), (4096, rs.R_FLOOR), (1, rs.R_NONE)):
        keys, count = db.sig_topk(d.data_ptr(), adj, r_min, k)
        assert count == rs.count(r, r_min), (k, r_min)
        assert np.array_equal(keys, rs.select(rs.keys(r, ids, r_min), k)), (k, r_min)
    assert 1000 <= rs.count(r, r1000) < 1100 and rs.count(r, rs.R_FLOOR) == n
    db.close()


def expected_rows(sw, db, edge, qn, go, ge, k, max_evalue):
    """What scan_hits_ranked must return, from the restatement."""
    cal, L, ids = edge["cal"][qn, go, ge], edge["L"], edge["ids"]
    adj = sw.capi.sig_rank_table(cal, int(L.max()))
    r_min = sw.capi.sig_rank_min(cal, max_evalue)
    sel, n_pass = rs.ranked(edge["want"][qn, go, ge], L, ids, adj, r_min, k)
    rows = db.hit_stats(edge["queries"][qn], rs.key_ids(sel).astype(np.int32), edge["m"], go, ge)
    for row in rows:
        row["evalue"], row["bits"], row["z"] = sw.capi.calib_sig(cal, row["score"], row["s_len"])
    return rows, n_pass


@pytest.mark.parametrize("go,ge", SCORINGS)
def test_scan_hits_ranked(sw, handle, edge, go, ge):
    """Rows equal hit_stats of the ids the restatement selects, sig equals
    calib_sig of each row, the calibration is scan_hits_sig's, E-values do not
    decrease along the rows (relative 1e-3: the key's resolution)."""
    m, n = edge["m"], len(edge["L"])
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    for qn in (600, 120, 40):
        q, cal = edge["queries"][qn], edge["cal"][qn, go, ge]
        _, sig_cal = db.scan_hits_sig(q, 12, m, go, ge)
        assert same_calib(sig_cal, cal)
        e12 = None
        for k, max_e in ((12, None), (n + 5, None), (12, 5.0), (4096, 0.5 * cal.n_db), (3, 1e-30)):
            rows, got_cal, n_pass = db.scan_hits_ranked(q, k, max_e, m, go, ge)
            want, want_pass = expected_rows(sw, db, edge, qn, go, ge, k, max_e)
            assert same_calib(got_cal, cal) and n_pass == want_pass and rows == want, (qn, k, max_e)
            assert len(rows) == min(k, n_pass)
            e = np.array([r["evalue"] for r in rows])
            assert np.all(e[1:] >= e[:-1] * (1 - 1e-3))
            if max_e is not None:
                assert np.all(e <= max_e * (1 + 1e-3))
            else:
                assert n_pass == n
            e12 = e if (k, max_e) == (12, None) else e12
        by_score, _ = db.scan_hits_sig(q, 12, m, go, ge)
        if (qn, go, ge) == (600, 11, 1):  # the fixture's condition, on the device
            a, b = set(r["id"] for r in by_score), set(r["id"] for r in db.scan_hits_ranked(q, 12, None, m, go, ge)[0])
            assert len(a ^ b) // 2 == edge["differ"] >= 3
    rows, cal0, n_pass = db.scan_hits_ranked(edge["queries"][0], 12, None, m, go, ge)
    assert cal0.status & cs.DEGENERATE and n_pass == n and [r["id"] for r in rows] == sorted(edge["ids"].tolist())[:12]
    rows, _, n_pass = db.scan_hits_ranked(edge["queries"][0], 12, cal0.n_db - 0.5, m, go, ge)
    assert rows == [] and n_pass == 0
    with pytest.raises(sw.SWError):
        db.scan_hits_ranked(edge["queries"][40], 12, 0.0, m, go, ge)
    with pytest.raises(sw.SWError):
        db.scan_hits_ranked(edge["queries"][40], 4097, None, m, go, ge)
    db.close()
    empty = sw.Database(handle, np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert empty.scan_hits_ranked(edge["queries"][40], 5, None, m, go, ge)[::2] == ([], 0)
    empty.close()


def test_planted_hit_alone_passes_the_cutoff(sw, handle):
    """A mutated copy of the query among 20,000 synthetic subjects
    (tests/test_gpu_calib.py's): E <= 1e-3 is that subject alone."""
    q = sw.synth.query(375)
    r, o = sw.synth.database(20000)
    copy = q.copy()
    copy[::4] = (copy[::4] + 7) % 20
    db = sw.Database(handle, np.concatenate([r, copy]), np.concatenate([o, [o[-1] + len(copy)]]))
    rows, cal, n_pass = db.scan_hits_ranked(q, 10, 1e-3, sw.capi.builtin_matrix(1), 11, 1)
    assert len(rows) == n_pass == 1 and rows[0]["id"] == 20000 and rows[0]["evalue"] < 1e-6
    assert cal.status == 0 and cal.n_db == 20001
    rows, _, n_pass = db.scan_hits_ranked(q, 10, None, sw.capi.builtin_matrix(1), 11, 1)
    assert n_pass == 20001 and len(rows) == 10 and rows[0]["id"] == 20000
    db.close()


def test_batch(sw, handle, edge):
    """(empty, 40, 600) with score_bytes forcing one row, two rows and the
    default: the three runs identical, and equal to the single calls."""
    m, k = edge["m"], 12
    queries = [edge["queries"][n] for n in (0, 40, 600)]
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    row = 4 * db.n_out
    assert [rs.ranked_groups(3, db.n_out, b) for b in (1, 2 * row, 0)] == [1, 2, 3]
    for max_e in (None, 20.0):
        runs = [db.scan_batch_hits_ranked(queries, k, max_e, m, 11, 1, score_bytes=b) for b in (1, 2 * row, 0)]
        for rows, calibs, n_pass in runs[1:]:
            assert rows == runs[0][0] and n_pass == runs[0][2]
            assert all(same_calib(a, b) for a, b in zip(calibs, runs[0][1]))
        rows, calibs, n_pass = runs[0]
        for qi, q in enumerate(queries):
            srows, scal, spass = db.scan_hits_ranked(q, k, max_e, m, 11, 1)
            assert rows[qi] == srows and same_calib(calibs[qi], scal) and n_pass[qi] == spass, (qi, max_e)
        assert calibs[0].status & cs.DEGENERATE and not calibs[2].status & cs.DEGENERATE
        if max_e is None:
            assert [r["id"] for r in rows[0]] == sorted(edge["ids"].tolist())[:k] and n_pass[0] == len(edge["L"])
        else:
            assert rows[0] == [] and n_pass[0] == 0 and 0 < n_pass[2] < len(edge["L"])
    assert db.scan_batch_hits_ranked([], k, None, m, 11, 1) == ([], [], [])
    db.close()


def test_pssm(sw, handle, edge):
    """The table derived from a sequence gives the sequence form's ids,
    scores and significances."""
    m, q = edge["m"], edge["queries"][600]
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    p = sw.Pssm(handle, np.asarray(m, dtype=np.int8).reshape(25, 25)[q])
    for go, ge in SCORINGS:
        for k, max_e in ((20, None), (4096, 3.0), (len(edge["L"]) + 5, None)):
            rows, cal, n_pass = db.scan_pssm_topk_ranked(p, k, max_e, go, ge)
            want, wcal, wpass = db.scan_hits_ranked(q, k, max_e, m, go, ge)
            assert same_calib(cal, wcal) and n_pass == wpass and len(rows) == len(want)
            assert rows == [{f: w[f] for f in ("id", "score", "evalue", "bits", "z")} for w in want], (go, ge, k, max_e)
    p.close()
    db.close()


def test_layout_independence(sw, handle, edge, tmp_path):
    """The same keys after the long threshold is changed and restored, and
    for the database saved and loaded (another subject order)."""
    q, m = edge["queries"][600], edge["m"]
    adj = sw.capi.sig_rank_table(edge["cal"][600, 11, 1], int(edge["L"].max()))
    r = rs.rank_values(edge["want"][600, 11, 1], edge["L"], adj)
    r_min = int(np.sort(r)[::-1][40])
    want = [(rs.select(rs.keys(r, edge["ids"], c), 30), rs.count(r, c)) for c in (rs.R_FLOOR, r_min)]

    def check(d):
        scores = device_scores(d, q, m, 11, 1)  # (kept alive: sig_topk takes its address)
        for (wk, wc), c in zip(want, (rs.R_FLOOR, r_min)):
            keys, count = d.sig_topk(scores.data_ptr(), adj, c, 30)
            assert count == wc and np.array_equal(keys, wk)

    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    check(db)
    for thr in (4096, 1, 64):
        db.set_long_threshold(thr)
        check(db)
    path = str(tmp_path / "edge.swdb")
    db.save(path)
    db.close()
    db2 = sw.Database.load(handle, path)
    assert not np.array_equal(db2.subjects()[0], edge["L"])
    check(db2)
    db2.close()


def test_shared_buffers(sw, handle, edge):
    """The ranked forms share the handle's score row and top-K workspace with
    the other calls: ranked call, scan_topk(k = 4096), ranked batch, scan, each
    equal to what a fresh handle gives."""
    m = edge["m"]
    queries = [edge["queries"][n] for n in (600, 0, 40)]

    def steps(h):
        db = sw.Database(h, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
        out = [lambda: db.scan_hits_ranked(queries[0], 12, 50.0, m, 11, 1),
               lambda: db.scan_topk(queries[0], 4096, m, 11, 1),
               lambda: db.scan_batch_hits_ranked(queries, 7, None, m, 11, 1, score_bytes=1),
               lambda: db.scan(queries[2], m, 11, 1)]
        return db, out

    def plain(v):
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, sw.capi.Calib):
            return [getattr(v, f) for f in CALIB_FIELDS]
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        return v

    db, seq = steps(handle)
    got = [plain(f()) for f in seq]
    db.close()
    for i in range(len(got)):
        fresh = sw.Handle(0, env_opts=False)
        fdb, fseq = steps(fresh)
        assert plain(fseq[i]()) == got[i], i
        fdb.close()
        fresh.close()
    assert np.array_equal(np.array(got[3])[edge["ids"]], edge["want"][40, 11, 1])


CLI = [os.path.join(LIB, "main"), "--query", GOLDEN + "/queries/P01008.fasta", "--db", GOLDEN + "/subset111.fasta",
       "--matrix", "blosum62", "--gap-open", "11", "--gap-extend", "1", "--hits", "5", "--evalue", "--rank", "evalue"]


@pytest.mark.parametrize("cut", [False, True])
def test_cli_rank_evalue(sw, handle, cut):
    """main --hits 5 --evalue --rank evalue [--max-evalue X]: the 14 columns of
    scan_hits_ranked's rows, and '# significant <n_pass> shown <nhits>' after
    the calibration line.  The cutoff is taken just above the third row's
    E-value, so it keeps some subjects and not all."""
    recs = []
    for line in open(GOLDEN + "/subset111.fasta"):
        if line.startswith(">"):
            recs.append("")
        else:
            recs[-1] += line.strip()
    res, offs = pack([sw.encode(s) for s in recs])
    db = sw.Database(handle, res, offs)
    q, m = sw.encode(read_query("P01008")), sw.capi.builtin_matrix(1)
    max_e = db.scan_hits_ranked(q, 5, None, m, 11, 1)[0][2]["evalue"] * 1.01 if cut else None
    want, cal, n_pass = db.scan_hits_ranked(q, 5, max_e, m, 11, 1)
    db.close()
    out = subprocess.run(CLI + (["--max-evalue", repr(max_e)] if max_e else []), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    rows = [ln.split("\t") for ln in lines if ln.count("\t") == 13]
    assert len(rows) == len(want) == min(5, n_pass) and len(want) >= 1
    for r, w in zip(rows, want):
        assert [int(v) for v in r[:12]] == [w[f] for f in FIELDS]
        assert r[12] == "%.3g" % w["evalue"] and r[13] == "%.1f" % w["bits"]
    cline = "# calibration %.6g %.6g %.6g %d %d %d" % (cal.a, cal.c, cal.sigma, cal.n_fit, cal.n_clipped, cal.status)
    sline = "# significant %d shown %d" % (n_pass, len(want))
    assert lines.index(cline) + 1 == lines.index(sline) == lines.index("\t".join(rows[0])) - 1
    assert not cal.status & cs.DEGENERATE and (3 <= n_pass < 111 if cut else n_pass == 111)
