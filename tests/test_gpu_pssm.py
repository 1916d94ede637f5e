"""GPU: profile (PSSM) queries through every scan form, bit for bit.

Two references, no tolerance anywhere:
  * a table derived from a sequence and a matrix (rows[i] = M[q[i]]) must scan
    exactly as the sequence does, in every kernel family (the sequence scans
    are themselves pinned to the oracle by the rest of the suite);
  * a genuinely position-specific table (no 25 x 25 matrix expresses it) must
    equal tests/native/pssm_oracle.cpp, which tests/test_pssm_oracle.py pins
    to the oracle on the CPU.

The scale is tests/test_gpu_scoring_envelope.py's: one database of about 214
subjects of 1..1,500 residues over all 25 codes with planted copies of the
consensus (one with a deletion, one with an insertion); tables of 40, 150 and
375 rows: one, three and six passes."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from pssm_support import PssmOracle, derived, path_score_pssm

pytestmark = pytest.mark.gpu
LIB = os.path.join(REPO, "ece1782-smith-waterman-cuda_amd", "lib")
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; "
                    r"pairs \d+; intra (-?\d+)/\d+ flagged, (-?\d+) again")
QLENS = (40, 150, 375)


class Env:
    pass


def pack(subs):
    res = np.concatenate(subs).astype(np.uint8)
    offs = np.zeros(len(subs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subs])
    return res, offs


def build_subjects():
    rng = np.random.default_rng(4711)
    q0 = rng.integers(0, 25, size=2100).astype(np.uint8)   # the consensus of every table
    q0[200] = q0[100]                                      # two positions with one consensus residue
    subs = []
    for lo, hi, forced in ((1, 40, (1, 2, 39, 40)), (41, 136, (63, 64, 65, 128, 129, 136)), (137, 300, (137, 256, 257, 300))):
        lens = list(forced) + [int(x) for x in rng.integers(lo, hi + 1, size=64 - len(forced))]
        subs += [rng.integers(0, 25, size=n).astype(np.uint8) for n in lens]
    subs += [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(700, 1501, size=12)]
    c = q0[:375]
    subs += [c.copy(), c[:190].copy(), np.concatenate([c[:180], c[183:]]),
             np.insert(c, 240, rng.integers(0, 25, size=2).astype(np.uint8)),
             np.concatenate([rng.integers(0, 25, size=300).astype(np.uint8), c[20:330],
                             rng.integers(0, 25, size=400).astype(np.uint8)]),
             q0[:1400].copy()]
    return q0, subs


def specific_table(q0, n, seed):
    """Entries in -8..12, the consensus entry raised above every other."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-8, 13, size=(n, 25))
    t[np.arange(n), q0[:n]] = rng.integers(13, 16, size=n)
    return np.ascontiguousarray(t, dtype=np.int8)


@pytest.fixture(scope="module")
def env(sw, handle, tmp_path_factory):
    e = Env()
    e.pso = PssmOracle(tmp_path_factory.mktemp("pssm_oracle"))
    e.q0, e.subs = build_subjects()
    assert len(set(np.concatenate(e.subs).tolist())) == 25 and 210 <= len(e.subs) <= 220
    e.res, e.offs = pack(e.subs)
    e.long_sel = np.array([k for k, s in enumerate(e.subs) if len(s) > 64])
    lres, loffs = pack([e.subs[k] for k in e.long_sel])
    e.all_sel = np.arange(len(e.subs))
    e.db = {"mixed": sw.Database(handle, e.res, e.offs),
            "merged": sw.Database(handle, e.res, e.offs, long_threshold=600),
            "long": sw.Database(handle, lres, loffs, long_threshold=64)}
    e.sel = {"mixed": e.all_sel, "merged": e.all_sel, "long": e.long_sel}
    rng = np.random.default_rng(99)
    asym = rng.integers(-12, 13, size=(25, 25))
    np.fill_diagonal(asym, rng.integers(3, 14, size=25))
    e.scorings = {"b50-2-2": (sw.capi.builtin_matrix(0), 2, 2), "b62-11-1": (sw.capi.builtin_matrix(1), 11, 1),
                  "asym-13-3": (np.ascontiguousarray(asym, dtype=np.int8), 13, 3)}
    assert (e.scorings["asym-13-3"][0] != e.scorings["asym-13-3"][0].T).any()
    e.tables = {n: specific_table(e.q0, n, 1000 + n) for n in QLENS + (2100,)}
    t = e.tables[375]
    assert e.q0[100] == e.q0[200] and (t[100] != t[200]).any(), "one consensus residue, two different rows"
    cache = {}

    def want(n, go, ge):
        if (n, go, ge) not in cache:
            cache[(n, go, ge)] = e.pso.scan(e.tables[n], e.res, e.offs, go, ge)
            cache[(n, go, ge)].setflags(write=False)
        return cache[(n, go, ge)]
    e.want = want
    yield e
    for d in e.db.values():
        d.close()


# ---- 1. a derived table scans as its sequence ---------------------------------
FORMS = [("mixed", "default", {})]
FORMS += [("mixed", "%s coop %s" % (v, c), dict(inter_variant=v, coop_width=-1 if c is None else c))
          for v, c in (("32x8", 0), ("32x8", 128), ("64x8", 0), ("64x8", 128), ("y32x8", None), ("f32x8", None))]
FORMS += [("merged", "lpt quads", dict(pair_width=64, lpt=1, quad_width=16, tri_width=0)),
          ("merged", "lpt tris", dict(pair_width=64, lpt=1, quad_width=-1, tri_width=16)),
          ("merged", "lpt 0", dict(pair_width=64, lpt=0))]
FORMS += [("long", "rows 4", dict(intra_x2_rows=4)), ("long", "rows 8", dict(intra_x2_rows=8)),
          ("long", "rows 20", dict(intra_x2_rows=20)), ("long", "intra_x2 0", dict(intra_x2=0)),
          ("long", "int16 first", dict(intra_i16_first=1))]


@pytest.mark.parametrize("scname", ["b50-2-2", "b62-11-1", "asym-13-3"])
def test_derived_equals_sequence(env, sw, handle, knobs, scname):
    """scan_pssm(derived) == scan(query) in every form; where the table holds
    the matrix's largest entry the plans are the same: same kernel names, no
    more launches."""
    mat, go, ge = env.scorings[scname]
    saved = handle.get_opts()
    pssms = {n: sw.Pssm(handle, derived(env.q0[:n], mat)) for n in QLENS}
    assert [len(p) for p in pssms.values()] == list(QLENS)
    assert derived(env.q0[:375], mat).max() == mat.max(), "the six-pass table holds the largest entry"
    for dbname, label, opts in FORMS:
        handle.set_opts(saved)
        if label != "default":  # (the two forms keep separate adaptive observations: routes pinned)
            knobs(inter_i16_span=0, intra_i16_first=0)
            knobs(**opts)
        db = env.db[dbname]
        for n in QLENS:
            q = env.q0[:n]
            db.reset_adaptive()
            want = db.scan(q, mat, go, ge)
            names = (handle.last_kernel(), handle.last_intra_kernel())
            launches = handle.timing()["launches"]
            db.reset_adaptive()
            got = db.scan_pssm(pssms[n], go, ge)
            pnames = (handle.last_kernel(), handle.last_intra_kernel())
            planches = handle.timing()["launches"]
            bad = np.nonzero(got != want)[0]
            assert not len(bad), (scname, label, n, pnames, bad[:10], got[bad[:10]], want[bad[:10]])
            if derived(q, mat).max() == mat.max():
                assert pnames == names, (scname, label, n)
                assert planches <= launches, (scname, label, n, planches, launches)
            if label == "default" and n == 375:
                assert want.max() > 1000  # the planted copies score
    handle.set_opts(saved)
    for p in pssms.values():
        p.close()


# ---- 2, 3. position-specific tables against the CPU restatement ---------------
FAMILIES = {
    "default": ("mixed", {}),
    "single wave": ("mixed", dict(lpt=0, pair_width=0, inter_i16_span=0, intra_i16_first=0)),
    "group": ("merged", dict(lpt=0, pair_width=64, inter_i16_span=0, intra_i16_first=0)),
    "merged": ("merged", dict(lpt=1, pair_width=64, quad_width=16, tri_width=0, inter_i16_span=0, intra_i16_first=0)),
    "intra": ("long", dict(intra_i16_first=0)),
    "int32": ("mixed", dict(inter_variant="32x8", intra_x2=0)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("go,ge", [(2, 2), (11, 1)])
def test_position_specific(env, sw, handle, knobs, family, go, ge):
    dbname, opts = FAMILIES[family]
    if opts:
        knobs(**opts)
    db = env.db[dbname]
    for n in QLENS:
        p = sw.Pssm(handle, env.tables[n])
        got = db.scan_pssm(p, go, ge)
        k, ik = handle.last_kernel(), handle.last_intra_kernel()
        p.close()
        want = env.want(n, go, ge)[env.sel[dbname]]
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (family, n, k, ik, bad[:10], got[bad[:10]], want[bad[:10]])
        if family == "single wave":
            assert k.startswith("sw_inter_x2s<"), k
        elif family == "group" and n > 64:
            assert k.startswith("sw_inter_x2p<") and "+lpt" not in k, k
        elif family == "merged" and n > 64:
            assert "+lpt" in k, k
        elif family == "intra":
            assert ik.startswith("sw_intra_x2<"), ik
        elif family == "int32":
            assert k.startswith("sw_inter<32,8,") and ik.startswith("sw_intra<"), (k, ik)
    # no 25 x 25 matrix expresses the table: the copies of the consensus score its raised entries
    if dbname != "long":
        t = env.tables[375]
        assert env.want(375, go, ge)[192 + 12] == int(t[np.arange(375), env.q0[:375]].sum())


def test_2100_rows(env, sw, handle):
    """Across the sequence builder's 2,048-row chunk: one builder launch."""
    p = sw.Pssm(handle, env.tables[2100])
    assert len(p) == 2100
    for go, ge in ((2, 2), (11, 1)):
        got = env.db["mixed"].scan_pssm(p, go, ge)
        want = env.want(2100, go, ge)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (go, ge, handle.last_kernel(), bad[:10], got[bad[:10]], want[bad[:10]])
    assert want[-1] == int(env.tables[2100][np.arange(1400), env.q0[:1400]].sum())
    p.close()


# ---- 4. guard bands ----------------------------------------------------------------
def flagged(capfd):
    m = RESCUE.findall(capfd.readouterr().err)
    assert m, "no rescue: line"
    return dict(zip(("inter", "inter_again", "intra", "intra_again"), map(int, m[-1])))


@pytest.mark.parametrize("n,top,score", [(300, 20, 6000), (400, 100, 40000)])
def test_guard_bands(env, sw, handle, knobs, capfd, n, top, score):
    """The consensus against its own table: 6,000 is above the fp16 cells'
    limit (the block is flagged), 40,000 above int16 (flagged again, re-scored
    in int32); as one subject per lane and as a long subject."""
    rng = np.random.default_rng(n)
    t = rng.integers(-8, 0, size=(n, 25))
    t[np.arange(n), env.q0[:n]] = top
    t = np.ascontiguousarray(t, dtype=np.int8)
    subs = [env.q0[:n].copy()] + env.subs[:100]
    res, offs = pack(subs)
    want = env.pso.scan(t, res, offs, 2, 2)
    assert want[0] == score and want[1:].max() < min(score, 32767 - 1152)  # only the consensus can pass int16
    p = sw.Pssm(handle, t)
    for threshold, kind in ((100000, "inter"), (64, "intra")):
        knobs(rescue_stats=1, inter_i16_span=0, intra_i16_first=0)
        db = sw.Database(handle, res, offs, long_threshold=threshold)
        capfd.readouterr()
        got = db.scan_pssm(p, 2, 2)
        f = flagged(capfd)
        k, ik = handle.last_kernel(), handle.last_intra_kernel()
        db.close()
        assert np.array_equal(got, want), (kind, k, ik, np.nonzero(got != want)[0][:10], got[0], want[0])
        assert (",fp16>" in k if kind == "inter" else ik.startswith("sw_intra_x2<")), (k, ik)
        assert f[kind] >= 1, (kind, f)
        assert (f[kind + "_again"] >= 1) == (score > 32767), (kind, f)
    p.close()


# ---- 5. top-K -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 25, 300])
def test_topk(env, sw, handle, k):
    p = sw.Pssm(handle, env.tables[375])
    db = env.db["mixed"]
    scores = db.scan_pssm(p, 11, 1)
    keys = db.scan_pssm_topk(p, k, 11, 1)
    p.close()
    ids, vals = sw.capi.topk(scores, k)
    gi, gv = sw.capi.decode_keys(keys)
    assert gi.tolist() == ids.tolist() and gv.tolist() == vals.tolist()
    assert np.array_equal(scores, env.want(375, 11, 1))
    if k > len(scores):
        assert gi[len(scores):].tolist() == [-1] * (k - len(scores))


# ---- 6. traceback -------------------------------------------------------------------
@pytest.mark.parametrize("go,ge", [(2, 2), (11, 1)])
def test_align_pssm(env, sw, handle, go, ge):
    t = env.tables[375]
    p = sw.Pssm(handle, t)
    db = env.db["mixed"]
    scores = db.scan_pssm(p, go, ge)
    ids, _ = sw.capi.topk(scores, 25)
    ids = [int(i) for i in ids] + [0, len(env.subs) - 1]
    got = db.align_pssm(p, ids, go, ge)
    p.close()
    for i, al in zip(ids, got):
        want = env.pso.align(t, env.subs[i], go, ge)
        assert al == want, (i, al, want)
        assert al["score"] == scores[i]
        if al["score"] > 0:
            assert path_score_pssm(t, env.subs[i], go, ge, al) == al["score"]
    assert any("D" in al["ops"] for al in got) and any("I" in al["ops"] for al in got), "the planted gaps show"


@pytest.mark.parametrize("scname", ["b50-2-2", "b62-11-1", "asym-13-3"])
def test_align_derived_equals_align(env, sw, handle, scname):
    mat, go, ge = env.scorings[scname]
    q = env.q0[:375]
    p = sw.Pssm(handle, derived(q, mat))
    db = env.db["mixed"]
    ids = list(range(192 + 12, len(env.subs))) + [0, 5, 100, 191]
    assert db.align_pssm(p, ids, go, ge) == db.align(q, ids, mat, go, ge)
    p.close()


def test_align_pssm_edges(sw, oracle, handle):
    """As test_gpu_align.py test_align_edges: the empty and the one-residue subject."""
    subs = [sw.encode("ACDEFGHIKL"), np.zeros(0, np.uint8), sw.encode("W")]
    res = np.concatenate(subs)
    offs = np.array([0, 10, 10, 11], dtype=np.int64)
    db = sw.Database(handle, res, offs, ids=np.array([5, 9, 2], dtype=np.int32))
    q = sw.encode("DEFG")
    p = sw.Pssm(handle, derived(q, sw.capi.builtin_matrix(0)))
    al = db.align_pssm(p, [5, 9, 2])
    assert al[0]["score"] > 0 and al[0]["ops"] == "MMMM" and (al[0]["s_begin"], al[0]["s_end"]) == (3, 6)
    assert al[1] == {"score": 0, "q_begin": 0, "q_end": 0, "s_begin": 0, "s_end": 0, "ops": ""}
    assert al[2] == oracle.align(q, subs[2])
    with pytest.raises(sw.capi.SWError):
        db.align_pssm(p, [7])  # not an id of this database
    aff = db.align_pssm(p, [5, 9, 2], gap=12, gap_extend=1)
    assert aff[0]["ops"] == "MMMM" and aff[1]["score"] == 0
    assert aff[2] == oracle.align(q, subs[2], None, 12, 1)
    empty = sw.Pssm(handle, np.zeros((0, 25), np.int8))
    assert db.align_pssm(empty, [5])[0]["score"] == 0
    for x in (p, empty):
        x.close()
    db.close()


# ---- 7. state and lifetime ------------------------------------------------------------
def test_state_and_lifetime(env, sw, handle):
    """A PSSM scan and a sequence scan of one length and one gap model
    alternate on one database with the adaptive routes on: separate
    observations, both exact, before and after reset_adaptive."""
    db = env.db["mixed"]
    t = env.tables[375]
    b50 = sw.capi.builtin_matrix(0)
    q = np.random.default_rng(3).integers(0, 20, size=375).astype(np.uint8)
    want_seq = db.scan(q, b50, 2, 2)
    a, b = sw.Pssm(handle, t), sw.Pssm(handle, env.tables[150])  # two alive at once
    for rnd in range(2):
        for _ in range(3):
            assert np.array_equal(db.scan_pssm(a, 2, 2), env.want(375, 2, 2))
            assert np.array_equal(db.scan(q, b50, 2, 2), want_seq)
        assert np.array_equal(db.scan_pssm(b, 2, 2), env.want(150, 2, 2))
        db.reset_adaptive()
    a.close()  # free one, scan with the other
    a.close()
    assert np.array_equal(db.scan_pssm(b, 11, 1), env.want(150, 11, 1))
    empty = sw.Pssm(handle, np.zeros((0, 25), np.int8))
    assert len(empty) == 0
    z = db.scan_pssm(empty, 2, 2)
    assert z.shape == want_seq.shape and not z.any()
    empty.close()
    bad = t.copy()
    bad[7, 3] = 101
    with pytest.raises(sw.capi.SWError, match="-1"):
        sw.Pssm(handle, bad)
    bad[7, 3] = -101
    with pytest.raises(sw.capi.SWError, match="-1"):
        sw.Pssm(handle, bad)
    for go, ge in ((0, 1), (1001, 1), (2, 0), (2, 1001)):
        with pytest.raises(sw.capi.SWError, match="-1"):
            db.scan_pssm(b, go, ge)
        with pytest.raises(sw.capi.SWError, match="-1"):
            db.scan_pssm_topk(b, 5, go, ge)
        with pytest.raises(sw.capi.SWError, match="-1"):
            db.align_pssm(b, [0], go, ge)
    assert np.array_equal(db.scan_pssm(b, 2, 2), env.want(150, 2, 2))  # the handle still scans
    b.close()


# ---- 8. the CLI -------------------------------------------------------------------------
def _pairs(stdout):
    return [tuple(map(int, ln.split(":"))) for ln in stdout.split("\n") if ln and ln[0].isdigit() and ":" in ln]


def test_main_pssm(env, sw, oracle, handle, tmp_path):
    recs = oracle.read_fasta_records(GOLDEN + "/subset111.fasta")
    subs = [sw.encode(s) for _, s in recs]  # as written: a set scoring scans without the '/' padding
    assert len(subs) == 111
    t = specific_table(env.q0, 120, 5)
    path = str(tmp_path / "q.pssm")
    sw.pssm.write_pssm(path, t)
    assert np.array_equal(sw.pssm.read_pssm(path)[0], t)
    db = sw.Database(handle, *pack(subs))
    p = sw.Pssm(handle, t)
    want = db.scan_pssm(p, 11, 1)
    p.close()
    db.close()
    main = os.path.join(LIB, "main")
    swdb = str(tmp_path / "subset111.swdb")
    mk = subprocess.run([main, "--make-db", swdb, "--db", GOLDEN + "/subset111.fasta"], capture_output=True, text=True,
                        timeout=300)
    assert mk.returncode == 0, mk.stderr
    ids, vals = sw.capi.topk(want, 10)
    for dbpath in (GOLDEN + "/subset111.fasta", swdb):
        for topk in (0, 10):
            out = subprocess.run([main, "--pssm", path, "--db", dbpath, "--gap-open", "11", "--gap-extend", "1"] +
                                 (["--topk", "10"] if topk else []), capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr
            assert out.stdout.startswith("Input profile: 120 positions\n")
            assert "Query length: 120 chars." in out.stdout and "Num subjects: 111" in out.stdout
            pairs = _pairs(out.stdout)
            if topk:
                assert pairs == list(zip(ids.tolist(), vals.tolist())), (dbpath, pairs)
            else:
                assert len(pairs) == 111 and all(want[i] == s for i, s in pairs), dbpath
