"""GPU: the calibration's count table (sw_score_hist, csrc/sw_calib.hip) and
the calls that carry it (sw_scan_hits_sig, sw_scan_batch_hits_sig,
sw_scan_pssm_topk_calib, main --evalue).  Every table must equal np.add.at
over the oracle's scores and the subjects' lengths exactly
(tests/calib_support.py): integers, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import calib_support as cs
from conftest import GOLDEN, REPO, read_query
from hits_support import FIELDS, pack

pytestmark = pytest.mark.gpu
LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")
CALIB_FIELDS = ("size", "status", "qlen", "fits", "n_db", "n_fit", "n_clipped", "n_skipped", "a", "c", "sigma")


def device_table(sw, db, q, m, go, ge, fill=0):
    """(table, scores): sw_scan_device into a torch buffer pre-filled with
    `fill`, then the synchronous sw_score_hist of it."""
    import torch
    scores = torch.full((max(db.n_out, 1),), fill, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    db.scan_device(q, scores.data_ptr(), m, go, ge)
    H = db.score_hist(scores.data_ptr())
    return H, scores.cpu().numpy()[:db.n_out]


def same_calib(a, b):
    return [getattr(a, f) for f in CALIB_FIELDS] == [getattr(b, f) for f in CALIB_FIELDS]


@pytest.fixture(scope="module")
def edge(sw, oracle):
    """About 300 subjects at the bin function's edges (0, 1, 2, 3, 4, 5, 7, 8,
    and 2^k - 1, 2^k, 5 * 2^(k-2) for k <= 11), three copies of a 120-residue
    query among them, result ids 3 * perm(i) + 1 (two of three slots map to no
    subject), and the oracle's scores per (query, scoring)."""
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
    want = {}
    for go, ge in ((11, 1), (6, 6)):
        for n, q in queries.items():
            s = oracle.scan(q, res, offs, m, go, ge) if n else np.zeros(len(subs), np.int32)
            s.setflags(write=False)
            want[n, go, ge] = s
    return {"res": res, "offs": offs, "ids": ids, "L": np.diff(offs), "queries": queries, "m": m, "want": want}


@pytest.mark.parametrize("go,ge", [(11, 1), (6, 6)])
def test_edge_database(sw, handle, edge, go, ge):
    """Both layouts hold subjects (long_threshold 64); every query length and
    both gap models; the clip column of the 120-residue query's scan holds
    exactly its three copies; the table's sum is n minus the empty subjects."""
    L, ids = edge["L"], edge["ids"]
    db = sw.Database(handle, edge["res"], edge["offs"], ids=ids, long_threshold=64)
    st = db.stats()
    assert st["n_long"] > 50 and st["n_blocks"] >= 1
    for n, q in edge["queries"].items():
        want = edge["want"][n, go, ge]
        H, scores = device_table(sw, db, q, edge["m"], go, ge)
        assert np.array_equal(scores[ids], want)
        assert np.array_equal(H, cs.table(want, L)), n
        assert int(H.sum()) == len(L) - int((L == 0).sum()) == len(L) - 2
        if n == 120:
            assert int(H[:, 511].sum()) == 3 and H[cs.length_bin([120])[0], 511] == 3
            assert sorted(want)[-3] > 511 >= sorted(want)[-4]
        if n == 0:
            assert int(H[:, 0].sum()) == len(L) - 2
    db.close()


def test_unmapped_slots_are_not_counted(sw, handle, edge):
    """The score buffer pre-filled with 0x7f7f7f7f: sw_scan_device writes only
    the slots some subject maps to, and the table counts only those."""
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    for _ in range(2):  # whatever scans of this shape allocate is allocated, their adaptive routes settled
        db.scan(edge["queries"][40], edge["m"], 11, 1)
    bytes0 = db.stats()["device_bytes"]
    H, scores = device_table(sw, db, edge["queries"][40], edge["m"], 11, 1, fill=0x7f7f7f7f)
    # the table's inputs went up once, on first use: the ids and the lengths, 4 bytes per subject each
    assert db.stats()["device_bytes"] == bytes0 + 8 * len(edge["L"])
    assert int((scores == 0x7f7f7f7f).sum()) == db.n_out - len(edge["L"]) > 0
    assert np.array_equal(H, cs.table(edge["want"][40, 11, 1], edge["L"]))
    assert int(H[:, 511].sum()) == 0
    db.close()


def test_hand_written_scores(sw, handle):
    """Negatives land in column 0; 511, 512 and INT32_MAX in column 511."""
    import torch
    lens = np.array([1, 2, 3, 5, 8, 13, 100, 100, 100, 100, 101, 4000, 4000, 5000, 0, 77], dtype=np.int64)
    subs = [np.zeros(n, np.uint8) for n in lens]
    res, offs = pack(subs)
    db = sw.Database(handle, res, offs)
    s = np.array([-1, -2 ** 31, 0, 510, 511, 512, 2 ** 31 - 1, -5, 510, 511, 512, 37, 2 ** 31 - 1, 1, 300, 511],
                 dtype=np.int32)
    d = torch.from_numpy(s).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    bytes0 = db.stats()["device_bytes"]
    H = db.score_hist(d.data_ptr())
    assert db.stats()["device_bytes"] == bytes0 + 4 * len(lens)  # the lengths (the ids are 0 .. n-1: not needed)
    assert np.array_equal(H, cs.table(s, lens))
    b100 = cs.length_bin([100])[0]
    assert H[b100, 0] == 1 and H[b100, 510] == 1 and H[b100, 511] == 3 and cs.length_bin([101])[0] == b100
    assert int(H.sum()) == 15 and int(H[:, 511].sum()) == 7 and int(H[:, 0].sum()) == 4
    # the asynchronous form into a device table of the caller's
    t = torch.full((cs.LBINS, cs.SBINS), 7, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert db.score_hist(d.data_ptr(), t.data_ptr()) is None
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), H)
    db.close()


def test_repack_and_file(sw, handle, edge, tmp_path):
    """The table does not depend on the layout: the same after the long
    threshold is changed and restored, and for the database saved and loaded
    (a .swdb file holds the subjects in length order)."""
    q, m = edge["queries"][600], edge["m"]
    want = cs.table(edge["want"][600, 11, 1], edge["L"])
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    assert np.array_equal(device_table(sw, db, q, m, 11, 1)[0], want)
    for thr in (4096, 1, 64):
        db.set_long_threshold(thr)
        assert np.array_equal(device_table(sw, db, q, m, 11, 1)[0], want), thr
    path = str(tmp_path / "edge.swdb")
    db.save(path)
    db.close()
    db2 = sw.Database.load(handle, path)
    assert not np.array_equal(db2.subjects()[0], edge["L"])  # another subject order
    assert np.array_equal(device_table(sw, db2, q, m, 11, 1)[0], want)
    db2.close()


def test_contention_one_counter(sw, handle, oracle):
    """5,000 identical subjects: one counter, equal to 5,000."""
    q = sw.synth.query(40, shard=42)
    s = sw.synth.residues(90, shard=77)
    res, offs = pack([s] * 5000)
    m = oracle.matrix(oracle.MATRIX_BLOSUM62)
    score = int(oracle.score(q, s, m, 11, 1))
    db = sw.Database(handle, res, offs)
    H, _ = device_table(sw, db, q, m, 11, 1)
    assert H[cs.length_bin([90])[0], score] == 5000 and int(H.sum()) == 5000
    db.close()


def test_contention_many_workgroups(sw, handle):
    """Database.synthetic(70000), a 40-residue query: 18 workgroups flush into
    the same few rows; against the table of the downloaded scores."""
    n = 70000
    db = sw.Database.synthetic(handle, 7, n)
    H, scores = device_table(sw, db, sw.synth.query(40, shard=42), sw.capi.builtin_matrix(1), 11, 1)
    L = sw.capi.synth_lengths(7, 0, n)
    assert np.array_equal(H, cs.table(scores, L)) and int(H.sum()) == n
    # (log-normal lengths, sigma 0.657: +-3 sigma alone span 5.7 octaves, 22 bins)
    assert (H.sum(axis=1) > 0).sum() >= 20 and H.max() > 500
    db.close()


def test_batch(sw, handle, edge):
    """Three queries (empty, 40, 600) in one call: each calibration equals the
    single-query call's and the fit of the single scan's table, the rows equal
    sw_scan_batch_hits's, and sig[q][i] is sw_calib_sig of the row exactly."""
    m, k = edge["m"], 12
    queries = [edge["queries"][n] for n in (0, 40, 600)]
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    rows, calibs = db.scan_batch_hits_sig(queries, k, m, 11, 1)
    plain = db.scan_batch_hits(queries, k, m, 11, 1)
    assert len(rows) == len(calibs) == 3
    for qi, q in enumerate(queries):
        assert [{f: r[f] for f in FIELDS} for r in rows[qi]] == plain[qi] and len(rows[qi]) == k
        single_rows, single = db.scan_hits_sig(q, k, m, 11, 1)
        assert same_calib(calibs[qi], single) and rows[qi] == single_rows
        H, _ = device_table(sw, db, q, m, 11, 1)
        fit = sw.capi.calib_fit(H, len(q))
        fit.n_skipped = 2
        assert same_calib(calibs[qi], fit), (calibs[qi].as_dict(), fit.as_dict())
        assert calibs[qi].n_db == len(edge["L"]) - 2 and calibs[qi].qlen == len(q)
        for r in rows[qi]:
            assert (r["evalue"], r["bits"], r["z"]) == sw.capi.calib_sig(calibs[qi], r["score"], r["s_len"])
    assert calibs[0].status & cs.DEGENERATE and not calibs[1].status & cs.DEGENERATE
    assert all(r["evalue"] == calibs[0].n_db and r["bits"] == 0 for r in rows[0])
    db.close()


def test_planted_hit_is_significant(sw, handle):
    """End to end on the device: a mutated copy of the query among 20,000
    synthetic subjects ranks first with E < 1e-6; no unrelated row behind it
    looks significant (the CPU test counts 1 subject of the 20,000 with E <= 1)."""
    q = sw.synth.query(375)
    r, o = sw.synth.database(20000)
    copy = q.copy()
    copy[::4] = (copy[::4] + 7) % 20
    res = np.concatenate([r, copy])
    offs = np.concatenate([o, [o[-1] + len(copy)]])
    db = sw.Database(handle, res, offs)
    rows, cal = db.scan_hits_sig(q, 10, sw.capi.builtin_matrix(1), 11, 1)
    print(cal.as_dict(), [(r_["id"], r_["score"], r_["evalue"]) for r_ in rows])
    assert rows[0]["id"] == 20000 and rows[0]["evalue"] < 1e-6 and rows[0]["bits"] > 100
    assert cal.status == 0 and cal.n_db == 20001 and cal.n_fit < cal.n_db
    assert all(0.01 < r_["evalue"] <= cal.n_db for r_ in rows[1:])
    db.close()


def test_pssm(sw, handle, edge):
    """The table derived from a sequence (rows[i] = matrix[q[i]]) gives the
    sequence scan's keys and calibration."""
    m, q = edge["m"], edge["queries"][600]
    db = sw.Database(handle, edge["res"], edge["offs"], ids=edge["ids"], long_threshold=64)
    p = sw.Pssm(handle, np.asarray(m, dtype=np.int8).reshape(25, 25)[q])
    for go, ge in ((11, 1), (6, 6)):
        keys, cal = db.scan_pssm_topk_calib(p, 20, go, ge)
        assert np.array_equal(keys, db.scan_topk(q, 20, m, go, ge))
        rows, want = db.scan_hits_sig(q, 20, m, go, ge)
        assert same_calib(cal, want) and cal.n_skipped == 2 and cal.qlen == 600
        ids, scores = sw.capi.decode_keys(keys)
        assert [int(s) for s in scores] == [r["score"] for r in rows]
    p.close()
    db.close()


CLI = [os.path.join(LIB, "main"), "--query", GOLDEN + "/queries/P01008.fasta", "--db", GOLDEN + "/subset111.fasta",
       "--matrix", "blosum62", "--gap-open", "11", "--gap-extend", "1"]


def test_cli_evalue(sw, handle):
    """main --hits 5 --evalue: 14 columns, the last two sw_scan_hits_sig's
    evalue (%.3g) and bits (%.1f), and the calibration line before the rows."""
    recs = []
    for line in open(GOLDEN + "/subset111.fasta"):
        if line.startswith(">"):
            recs.append("")
        else:
            recs[-1] += line.strip()
    res, offs = pack([sw.encode(s) for s in recs])
    db = sw.Database(handle, res, offs)
    want, cal = db.scan_hits_sig(sw.encode(read_query("P01008")), 5, sw.capi.builtin_matrix(1), 11, 1)
    db.close()
    out = subprocess.run(CLI + ["--hits", "5", "--evalue"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    rows = [ln.split("\t") for ln in lines if ln.count("\t") == 13]
    assert len(rows) == 5 and not [ln for ln in lines if ln.count("\t") == 11]
    for r, w in zip(rows, want):
        assert [int(v) for v in r[:12]] == [w[f] for f in FIELDS]
        assert r[12] == "%.3g" % w["evalue"] and r[13] == "%.1f" % w["bits"]
    cline = [ln for ln in lines if ln.startswith("# calibration ")]
    assert cline == ["# calibration %.6g %.6g %.6g %d %d %d" % (cal.a, cal.c, cal.sigma, cal.n_fit, cal.n_clipped,
                                                                cal.status)]
    assert lines.index(cline[0]) < lines.index("\t".join(rows[0]))
    assert "warning" not in out.stderr


def test_cli_evalue_warns_when_scores_clip(sw):
    """The reference's own scoring (BLOSUM50, gap 2): scores grow with length,
    the calibration says so and the CLI warns on stderr."""
    out = subprocess.run(CLI[:5] + ["--hits", "3", "--evalue"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    status = int([ln for ln in out.stdout.split("\n") if ln.startswith("# calibration ")][0].split()[-1])
    assert status & cs.CLIPPED and "warning" in out.stderr and "clip" in out.stderr


def test_cli_evalue_needs_hits():
    """Refused before any file is read (the files named here do not exist)."""
    for extra in ([], ["--topk", "5"], ["--queries", "/nonexistent/qs.fasta", "--topk", "5"]):
        args = [os.path.join(LIB, "main"), "--db", "/nonexistent/db.fasta", "--evalue"] + extra
        if "--queries" not in extra:
            args += ["--query", "/nonexistent/q.fasta"]
        out = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "--evalue" in out.stderr and "--hits" in out.stderr, (out.stdout, out.stderr)


def stable_lines(text):
    """The CLI's output without the two lines that carry wall time."""
    return [ln for ln in text.split("\n") if not ln.startswith(("Time elapsed:", "Performance:"))]


@pytest.mark.parametrize("name,flags", [("cli_hits5", ["--query", GOLDEN + "/queries/P01008.fasta", "--hits", "5"]),
                                        ("cli_queries_hits3", ["--queries", GOLDEN + "/calib_queries.fasta", "--hits", "3"])])
def test_cli_without_evalue_is_unchanged(name, flags):
    """Against a run recorded before --evalue existed (tests/golden/*.txt)."""
    out = subprocess.run([CLI[0]] + CLI[3:] + flags, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert stable_lines(out.stdout) == stable_lines(open(os.path.join(GOLDEN, name + ".txt")).read())
