"""GPU: the iterated profile search (include/sw_amd.h "iterated profile
search") at its limits and across its state, against the numpy model
(tests/profile_support.py), the PSSM oracle (tests/native/pssm_oracle.cpp) and
the scan oracle.  tests/test_profile_limits_inputs.py shows on the CPU that
the inputs have the properties relied on here.

  a  4,096 hits in three launch groups of sw_align's walk back: the rows, the
     results, the tables and the refined table of the second and third group;
  b  sw_msa.hip at the shapes its loops have, and under a permutation of rows;
  c  rows, tables and refine under five scorings at the envelope (open below
     extend, gaps of 1000, entries of +-100, the clamp);
  d  sw_search_iter's other branches (dropped members, the include_max cut,
     a round with added == dropped, a run that stops unconverged), result ids
     with gaps in two layouts, a loaded file, a synthetic database, the edges;
  e  one handle with other work between the rounds' scans;
  f  main --iterations on a .swdb file.

Bytes and integers are compared exactly; a refined table after asserting that
the model's unrounded entries keep 1e-6 from every half-integer."""
import ctypes
import os
import re
import subprocess
import time

import numpy as np
import pytest

import history_support as hs
import profile_support as ps
import pssm_support

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib", "main")
LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged")
MANY_SCORINGS = {"b62-11-1": (1, 11, 1), "b50-2-2": (0, 2, 2)}
ENVELOPE = ["specific-1-4", "specific-1000-1000", "scaled-28-28", "scaled-40-3", "m100-11-1"]


@pytest.fixture(autouse=True)
def timed(request, capfd):
    t = time.perf_counter()
    yield
    with capfd.disabled():
        print("\nLIMITS time | %s | %.2f s" % (request.node.name, time.perf_counter() - t))


@pytest.fixture(scope="module")
def po(tmp_path_factory):
    return pssm_support.PssmOracle(tmp_path_factory.mktemp("limits_oracle"))


# ---- a: rows, tables and refine across launch groups ---------------------------------------
@pytest.fixture(scope="module")
def many(sw, handle):
    q, subjects, ids = ps.many_hits_input()
    res, offs = ps.pack(subjects)
    db = sw.Database(handle, res, offs)
    d = {"q": q, "subjects": subjects, "ids": ids, "db": db, "want": {}}
    d["ends"] = ps.align_group_ends(600, np.diff(offs)[ids])
    assert len(d["ends"]) >= 3
    yield d
    db.close()


def many_expected(sw, po, many, name):
    """The model's rows (without row 0) and the oracle's alignments: the 47
    distinct subjects aligned once, the rows indexed by the ids."""
    if name not in many["want"]:
        mid, go, ge = MANY_SCORINGS[name]
        m = sw.capi.builtin_matrix(mid)
        rows = pssm_support.derived(many["q"], m)
        aligns = [po.align(rows, s, go, ge) for s in many["subjects"]]
        distinct = np.array([ps.row_of(600, s, a) for s, a in zip(many["subjects"], aligns)], dtype=np.uint8)
        many["want"][name] = (m, rows, aligns, distinct[many["ids"]])
    return many["want"][name]


def many_msa(many, hit_rows, with_master):
    top = many["q"] if with_master else np.full(600, ps.NONE, dtype=np.uint8)
    return np.vstack([top[None, :], hit_rows])


@pytest.mark.parametrize("name", list(MANY_SCORINGS))
def test_rows_and_results_of_every_launch_group(sw, handle, po, many, name, capfd):
    m, rows, aligns, hit_rows = many_expected(sw, po, many, name)
    _, go, ge = MANY_SCORINGS[name]
    p = sw.Pssm(handle, rows)
    t = time.perf_counter()
    got, al = many["db"].msa_pssm(p, many["ids"], master=many["q"], gap=go, gap_extend=ge)
    with capfd.disabled():
        print("\nLIMITS msa_pssm of 4,096 hits x 600 | %s | groups end at %s | %.3f s" % (name, many["ends"],
                                                                                      time.perf_counter() - t))
    want = many_msa(many, hit_rows, True)
    assert got.shape == (4097, 600)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], many["ends"])
    for k, i in enumerate(many["ids"]):
        a = aligns[i]
        assert (al[k]["score"], al[k]["q_begin"], al[k]["q_end"], al[k]["s_begin"], al[k]["s_end"]) == \
            (a["score"], a["q_begin"], a["q_end"], a["s_begin"], a["s_end"]), (k, many["ends"])
    with pytest.raises(sw.SWError, match="-1"):
        many["db"].msa_pssm(p, np.zeros(4097, dtype=np.int32), master=many["q"], gap=go, gap_extend=ge)
    p.close()


@pytest.mark.parametrize("with_master", [True, False])
@pytest.mark.parametrize("name", list(MANY_SCORINGS))
def test_tables_and_refine_of_4096_hits(sw, handle, po, many, name, with_master, capfd):
    m, rows, aligns, hit_rows = many_expected(sw, po, many, name)
    _, go, ge = MANY_SCORINGS[name]
    master = many["q"] if with_master else None
    wc, ww, ws = ps.tables(many_msa(many, hit_rows, with_master))
    want, raw = ps.pssm_from_counts(wc, ws, rows, m, 10.0)
    assert ps.half_margin(raw) > 1e-6
    p = sw.Pssm(handle, rows)
    cnt, weight, wsum = many["db"].profile_counts(p, many["ids"], master=master, gap=go, gap_extend=ge)
    assert np.array_equal(cnt, wc), np.argwhere(cnt != wc)[:5]
    assert np.array_equal(weight, ww), np.nonzero(weight != ww)[0][:5]
    assert np.array_equal(wsum, ws), np.argwhere(wsum != ws)[:5]
    t = time.perf_counter()
    new = many["db"].refine_pssm(p, many["ids"], master=master, matrix=m, pseudo=10.0, gap=go, gap_extend=ge)
    with capfd.disabled():
        print("\nLIMITS refine_pssm of 4,096 hits x 600 | %s | %.3f s" % (name, time.perf_counter() - t))
    got = new.rows()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    T = ws.astype(object).sum(axis=1)
    assert (T == 0).any() and np.array_equal(got[T == 0], rows[T == 0])  # nothing counted: the prior row
    if with_master:
        assert ((T == 0) & (many["q"] >= 20)).any()
    new.close()
    p.close()


# ---- b: sw_msa.hip at the shapes its loops have ----------------------------------------------
def shaped_rows(nrows, qlen, seed):
    """Rows over every byte value 0..26 (tests/test_gpu_profile.py
    synthetic_rows, for any qlen): column 0 all 20 residues, and from three
    columns on column 1 gaps only, column 2 codes 20..24 only, the last column
    one residue; every seventh row all NONE."""
    rng = np.random.default_rng(seed)
    msa = rng.integers(0, 27, size=(nrows, qlen)).astype(np.uint8)
    msa[:, 0] = np.arange(nrows) % 20
    if qlen >= 4:
        msa[:, 1] = ps.GAP
        msa[:, 2] = 20 + np.arange(nrows) % 5
        msa[:, qlen - 1] = 7
    msa[6::7] = ps.NONE
    return msa


@pytest.mark.parametrize("nrows, qlen", [(n, q) for n in (31, 32, 33, 63, 97) for q in (1, 2, 128, 129, 1000)] +
                         [(4097, 1000)])
def test_msa_tables_at_the_loops_shapes(sw, handle, nrows, qlen):
    msa = shaped_rows(nrows, qlen, 1000 * nrows + qlen)
    wc, ww, ws = ps.tables(msa)
    cnt, weight, wsum = sw.capi.profile_counts_msa(handle, msa)
    assert np.array_equal(cnt, wc), np.argwhere(cnt != wc)[:5]
    assert np.array_equal(weight, ww), np.nonzero(weight != ww)[0][:5]
    assert np.array_equal(wsum, ws), np.argwhere(wsum != ws)[:5]
    assert int(wsum.max()) < 2 ** 43 and (weight[6::7] == 0).all()
    # another order of the rows (other waves and batches take them): the same column tables
    perm = np.random.default_rng(nrows + qlen).permutation(nrows)
    cnt, weight, wsum = sw.capi.profile_counts_msa(handle, np.ascontiguousarray(msa[perm]))
    assert np.array_equal(cnt, wc) and np.array_equal(wsum, ws) and np.array_equal(weight, ww[perm])


# ---- c: rows and refine at the envelope -------------------------------------------------------
@pytest.fixture(scope="module")
def envelope(sw, handle):
    q0, table, subjects, ids = ps.envelope_input()
    res, offs = ps.pack(subjects)
    db = sw.Database(handle, res, offs)
    yield {"q0": q0, "subjects": subjects, "ids": ids, "db": db,
           "scorings": ps.envelope_scorings(q0, table, sw.capi.builtin_matrix(1))}
    db.close()


@pytest.mark.parametrize("name", ENVELOPE)
def test_envelope_rows_tables_and_refine(sw, handle, po, envelope, name):
    rows, go, ge, mat = envelope["scorings"][name]
    ids, db = envelope["ids"], envelope["db"]
    master = ps.envelope_master(name, envelope["q0"])
    sel = [envelope["subjects"][i] for i in ids]
    aligns = [po.align(rows, s, go, ge) for s in sel]
    want = ps.msa_of(375, master, sel, aligns)
    p = sw.Pssm(handle, rows)
    got, al = db.msa_pssm(p, ids, master=master, gap=go, gap_extend=ge)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    for k, a in enumerate(aligns):
        assert (al[k]["score"], al[k]["q_begin"], al[k]["q_end"]) == (a["score"], a["q_begin"], a["q_end"]), k
    wc, ww, ws = ps.tables(want)
    cnt, weight, wsum = db.profile_counts(p, ids, master=master, gap=go, gap_extend=ge)
    assert np.array_equal(cnt, wc) and np.array_equal(weight, ww) and np.array_equal(wsum, ws)
    for pseudo in (10.0, 0.5):
        table, raw = ps.pssm_from_counts(wc, ws, rows, mat, pseudo)
        assert ps.half_margin(raw) > 1e-6
        new = db.refine_pssm(p, ids, master=master, matrix=mat, pseudo=pseudo, gap=go, gap_extend=ge)
        assert np.array_equal(new.rows(), table), (pseudo, np.argwhere(new.rows() != table)[:5])
        if name == "m100-11-1":  # the clamp, through the device path
            assert (raw > 100.5).any() and (raw < -100.5).any()
            assert int(table[:, :20].max()) == 100 and int(table[:, :20].min()) == -100
        new.close()
    p.close()


def test_refine_without_lambda_leaves_no_pssm(sw, handle, envelope):
    rows, go, ge, _ = envelope["scorings"]["specific-1-4"]
    p = sw.Pssm(handle, rows)
    ids = np.ascontiguousarray(envelope["ids"], dtype=np.int32)
    flat = np.full(625, 3, dtype=np.int8)
    out = ctypes.c_void_p(12345)
    rc = sw.capi.lib().sw_pssm_refine(handle.ptr, envelope["db"].ptr, p.ptr, go, ge, None,
                                      flat.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), 10.0,
                                      ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(ids), ctypes.byref(out))
    assert rc == -5 and not out.value
    assert np.array_equal(p.rows(), rows)
    p.close()


# ---- d: the loop's branches and the ids -------------------------------------------------------
class Family:
    def __init__(self, sw, handle, po):
        self.sw, self.po = sw, po
        self.q, self.res, self.offs = ps.family_database()
        self.m = sw.capi.builtin_matrix(1)
        self.ids = ps.custom_ids(len(self.offs) - 1)
        self.db = sw.Database(handle, self.res, self.offs)
        self.custom = sw.Database(handle, self.res, self.offs, ids=self.ids, long_threshold=ps.FAMILY_LONG_THRESHOLD)
        st = self.custom.stats()
        assert st["n_long"] >= 10 and st["n_long"] < st["n_subjects"] - 10 and st["max_id"] == int(self.ids.max())
        self._models = {}

    def model(self, rounds, inclusion, include_max, custom=False, q=None, k=500):
        key = (rounds, inclusion, include_max, custom, None if q is None else q.tobytes(), k)
        if key not in self._models:
            self._models[key] = ps.search_iter_model(self.sw.capi, self.po, self.q if q is None else q, self.m, 11, 1,
                                                     self.res, self.offs, rounds, inclusion, include_max, 10.0, k, None,
                                                     ids=self.ids if custom else None)
            assert self._models[key]["margin"] > 1e-6
        return self._models[key]

    def close(self):
        self.db.close()
        self.custom.close()


@pytest.fixture(scope="module")
def fam(sw, handle, po):
    f = Family(sw, handle, po)
    yield f
    f.close()


def check_iter(sw, out, model):
    """One sw_search_iter result against the model: the trace, how it ended,
    every round's calibration, the report and the last table."""
    assert out["converged"] == model["converged"] and len(out["rounds"]) == model["rounds_run"]
    prev = set()
    for t, (got, want) in enumerate(zip(out["rounds"], model["rounds"])):
        cur = set(want["ids"])
        assert (got["included"], got["added"], got["dropped"]) == (len(cur), len(cur - prev), len(prev - cur)), t
        for f in ("a", "c", "sigma"):
            assert getattr(got["calib"], f) == getattr(want["calib"], f), (t, f)
        prev = cur
    assert [r["id"] for r in out["rows"]] == model["ids"]
    assert [r["score"] for r in out["rows"]] == model["scores"]
    assert out["n_pass"] == model["n_pass"]
    for f in ("a", "c", "sigma"):
        assert getattr(out["calib"], f) == getattr(model["calib"], f)
    for r in out["rows"][:80]:
        e, bits, z = sw.capi.calib_sig(model["calib"], r["score"], int(model["lengths"][model["index_of"][r["id"]]]))
        assert (r["evalue"], r["bits"], r["z"]) == (e, bits, z)
    if "pssm" in out:
        assert np.array_equal(out["pssm"].rows(), model["rows"])
        out["pssm"].close()


def run_iter(db, fam, rounds, inclusion, include_max, q=None, k=500):
    return db.search_iter(fam.q if q is None else q, rounds, inclusion_evalue=inclusion, include_max=include_max,
                          pseudo=10.0, k=k, matrix=fam.m, gap=11, gap_extend=1, final_pssm=True)


@pytest.mark.parametrize("rounds, inclusion, include_max", [(6, 10.0, 64), (4, 10.0, 64), (6, 1e-3, 10), (6, 1e-3, 1)])
def test_loop_branches_equal_the_model(sw, fam, rounds, inclusion, include_max):
    model = fam.model(rounds, inclusion, include_max)
    if include_max == 64:
        assert model["converged"] == (rounds == 6) and model["rounds_run"] == rounds
        assert any(len(set(a["ids"]) - set(b["ids"])) > 0 for a, b in zip(model["rounds"], model["rounds"][1:]))  # dropped
    check_iter(sw, run_iter(fam.db, fam, rounds, inclusion, include_max), model)
    # every round's included ids in key order: a search stopped after t rounds reports I_t under the
    # inclusion's bounds
    for t in range(1, model["rounds_run"] + 1):
        o = fam.db.search_iter(fam.q, t, inclusion_evalue=inclusion, include_max=include_max, k=include_max,
                               max_evalue=inclusion, matrix=fam.m, gap=11, gap_extend=1)
        assert [r["id"] for r in o["rows"]] == model["rounds"][t - 1]["order"], t
        assert o["n_pass"] == model["rounds"][t - 1]["n_pass"]


@pytest.mark.parametrize("source", ["created", "loaded"])
def test_custom_ids_in_two_layouts(sw, handle, fam, source, tmp_path):
    model = fam.model(6, 10.0, 64, custom=True)
    assert min(model["ids"]) >= 7 and max(model["ids"]) > len(fam.ids)
    db = fam.custom
    if source == "loaded":
        path = str(tmp_path / "family.swdb")
        fam.custom.save(path)
        db = sw.Database.load(handle, path, long_threshold=ps.FAMILY_LONG_THRESHOLD)
        L, ids = db.subjects()
        assert db.stats()["max_id"] == int(fam.ids.max()) and sorted(ids.tolist()) == sorted(fam.ids.tolist())
    check_iter(sw, run_iter(db, fam, 6, 10.0, 64), model)
    short = fam.model(4, 10.0, 64, custom=True)
    check_iter(sw, run_iter(db, fam, 4, 10.0, 64), short)
    assert not short["converged"]
    if source == "loaded":
        db.close()


def test_synthetic_database(sw, handle, po, fam):
    """Database.synthetic holds no family: at inclusion 1e30 whatever ranks
    first is included (include_max 50), over the generator's residues
    regenerated on the host."""
    db = sw.Database.synthetic(handle, hs.C_SEED, hs.C_N)
    subs = hs.c_subjects(sw, *db.subjects())
    res, offs = ps.pack(subs)
    model = ps.search_iter_model(sw.capi, po, fam.q, fam.m, 11, 1, res, offs, 3, 1e30, 50, 10.0, 500, None)
    assert model["margin"] > 1e-6 and all(len(r["ids"]) == 50 for r in model["rounds"])
    check_iter(sw, run_iter(db, fam, 3, 1e30, 50), model)
    db.close()


def test_empty_database(sw, handle, po, fam):
    db = sw.Database(handle, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    out = run_iter(db, fam, 5, 1e-3, 4096)
    assert [(r["included"], r["added"], r["dropped"]) for r in out["rounds"]] == [(0, 0, 0)] * 2
    assert out["converged"] and out["rows"] == [] and out["n_pass"] == 0
    assert np.array_equal(out["pssm"].rows(), pssm_support.derived(fam.q, fam.m))
    out["pssm"].close()
    db.close()


def test_nothing_passes_is_a_refine_without_hits(sw, fam):
    """An inclusion bound nothing passes: I_1 and I_2 are empty, and P_2 =
    refine(P_1, no hit, master = the query) is P_1: the derived table where
    the query holds a counted code, the prior row where it holds 20..24."""
    q25 = fam.q.copy()
    q25[5::7] = 20 + np.arange(len(q25[5::7])) % 5
    for q in (fam.q, q25):
        out = run_iter(fam.db, fam, 5, 1e-300, 4096, q=q, k=20)
        assert [(r["included"], r["added"], r["dropped"]) for r in out["rounds"]] == [(0, 0, 0)] * 2 and out["converged"]
        derived = pssm_support.derived(q, fam.m)
        got = out["pssm"].rows()
        assert np.array_equal(got[q >= 20], derived[q >= 20]) and np.array_equal(got, derived)
        out["pssm"].close()
        model = fam.model(5, 1e-300, 4096, q=q, k=20)
        assert [r["id"] for r in out["rows"]] == model["ids"] and [r["score"] for r in out["rows"]] == model["scores"]


def test_query_over_all_25_codes(sw, fam):
    q25 = fam.q.copy()
    q25[5::7] = 20 + np.arange(len(q25[5::7])) % 5
    assert set(q25.tolist()) == set(range(25))
    model = fam.model(3, 10.0, 64, q=q25)
    assert len(model["rounds"][0]["ids"]) > 0
    check_iter(sw, run_iter(fam.db, fam, 3, 10.0, 64, q=q25), model)


def test_a_matrix_without_lambda_runs_one_round(sw, po, fam):
    flat = np.full((25, 25), 3, dtype=np.int8)
    one = fam.db.search_iter(fam.q, 1, k=50, matrix=flat, gap=11, gap_extend=1, final_pssm=True)
    model = ps.search_iter_model(sw.capi, po, fam.q, flat, 11, 1, fam.res, fam.offs, 1, 1e-3, 4096, 10.0, 50, None)
    check_iter(sw, one, model)
    with pytest.raises(sw.SWError, match="-5"):
        fam.db.search_iter(fam.q, 2, k=50, matrix=flat, gap=11, gap_extend=1)


def test_empty_query(sw, po, fam):
    """qlen 0: every score is 0, nothing passes a finite inclusion bound, the
    refine of no position is the empty table, round 2 converges; the report
    under no cutoff is the k lowest ids with score 0."""
    q = np.zeros(0, dtype=np.uint8)
    model = fam.model(4, 1e-3, 4096, q=q, k=30)
    assert model["rounds_run"] == 2 and model["converged"] and model["scores"] == [0] * 30
    out = run_iter(fam.db, fam, 4, 1e-3, 4096, q=q, k=30)
    assert out["pssm"].rows().shape == (0, 25)
    check_iter(sw, out, model)


# ---- e: one handle, other work in between ---------------------------------------------------
@pytest.fixture(scope="module")
def world(oracle):
    return hs.World(oracle)


class Shared:
    """The models of section e, computed once for both handles."""

    def __init__(self, sw, po, world, fam):
        self.qa = world.queries[4]
        self.x6, self.go, self.ge = world.scoring("b62x6-66-6")
        res, offs = world.packed["A"]
        self.a_iter = ps.search_iter_model(sw.capi, po, self.qa, self.x6, self.go, self.ge, res, offs, 3, 10.0, 4096, 10.0,
                                           500, None)
        assert self.a_iter["margin"] > 1e-6 and self.a_iter["rounds_run"] == 3 and not self.a_iter["converged"]
        t = [r["table"] for r in self.a_iter["rounds"]]
        assert t[0].shape == t[1].shape == t[2].shape and not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2])
        self.fam_scores = po.scan(pssm_support.derived(fam.q, fam.m), fam.res, fam.offs, 11, 1)
        keys = hs.local_topk(self.fam_scores, fam.ids, 4096)
        self.fam_keys = np.concatenate([keys, np.full(4096 - len(keys), hs.PAD, dtype=np.int64)])
        self.fam_ranked = fam.model(1, 1e-3, 4096, custom=True, k=100)
        self.fam_iter = fam.model(3, 1e-3, 4096, custom=True)


@pytest.fixture(scope="module")
def shared(sw, po, world, fam):
    return Shared(sw, po, world, fam)


class HeldRows:
    """A search_iter result's last table, kept past its handle."""

    def __init__(self, pssm):
        self._rows = pssm.rows()
        pssm.close()

    def rows(self):
        return self._rows

    def close(self):
        pass


def sequence(sw, world, fam, shared):
    """The six steps on a fresh handle; returns the routes after every step
    and the results."""
    import torch
    h = sw.Handle(0, env_opts=False)
    h.set_opts(**hs.PROFILES["lpt64"])
    res, offs = world.packed["A"]
    a = sw.Database(h, res, offs, long_threshold=hs.A_THRESHOLD)
    f = sw.Database(h, fam.res, fam.offs, ids=fam.ids, long_threshold=ps.FAMILY_LONG_THRESHOLD)
    routes, out = [], {}

    def step(name, value):
        if isinstance(value, dict):
            value["pssm"] = HeldRows(value["pssm"])
        out[name] = value
        routes.append((name, h.last_kernel(), h.last_intra_kernel()))
    try:
        step("topk", f.scan_topk(fam.q, 4096, fam.m, 11, 1))
        kw = dict(include_max=4096, pseudo=10.0, k=500, final_pssm=True)
        akw = dict(kw, inclusion_evalue=10.0, matrix=shared.x6, gap=shared.go, gap_extend=shared.ge)
        step("iter_a", a.search_iter(shared.qa, 3, **akw))
        p = sw.Pssm(h, pssm_support.derived(fam.q, fam.m))
        step("ranked", f.scan_pssm_topk_ranked(p, 100, gap_open=11, gap_extend=1))
        p.close()
        step("iter_fam", f.search_iter(fam.q, 3, inclusion_evalue=1e-3, matrix=fam.m, gap=11, gap_extend=1, **kw))
        buf = torch.full((a.n_out,), hs.FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the fill ran on torch's stream
        a.scan_device(shared.qa, buf.data_ptr(), shared.x6, shared.go, shared.ge)
        torch.cuda.synchronize()
        step("device", buf.cpu().numpy())
        step("iter_a_again", a.search_iter(shared.qa, 3, **akw))
        # a refine between two top-K scans: the keys share the handle's score buffer with the rounds' state
        p = sw.Pssm(h, pssm_support.derived(fam.q, fam.m))
        k1 = f.scan_topk(fam.q, 4096, fam.m, 11, 1)
        new = f.refine_pssm(p, shared.fam_iter["rounds"][0]["order"], master=fam.q, matrix=fam.m, gap=11, gap_extend=1)
        out["refined"] = new.rows()
        new.close()
        p.close()
        step("topk_after_refine", (k1, f.scan_topk(fam.q, 4096, fam.m, 11, 1)))
    finally:
        a.close()
        f.close()
        h.close()
    return routes, out


def plain(o):
    """A search_iter result as comparable values."""
    return ([(r["id"], r["score"], r["evalue"], r["bits"], r["z"]) for r in o["rows"]], o["n_pass"], o["converged"],
            [(r["included"], r["added"], r["dropped"], r["calib"].a, r["calib"].c, r["calib"].sigma) for r in o["rounds"]],
            o["pssm"].rows().tobytes())


def test_fixture_condition_of_the_shared_handle(sw, world, oracle, capfd):
    """The PSSM scans of section e on A take the merged launch with its drain
    and have something to drain."""
    h = sw.Handle(0, env_opts=False)
    h.set_opts(**dict(hs.PROFILES["lpt64"], rescue_stats=1))
    res, offs = world.packed["A"]
    a = sw.Database(h, res, offs, long_threshold=hs.A_THRESHOLD)
    m, go, ge = world.scoring("b62x6-66-6")
    p = sw.Pssm(h, pssm_support.derived(world.queries[4], m))
    capfd.readouterr()
    got = a.scan_pssm(p, go, ge)
    found = RESCUE.findall(capfd.readouterr().err)
    name = h.last_kernel()
    p.close()
    a.close()
    h.close()
    assert "+lpt+drain" in name, name
    assert found and int(found[-1]) > 0, found
    assert np.array_equal(got, world.full("A", 4, "b62x6-66-6"))


def test_one_handle_with_other_work_in_between(sw, world, fam, shared):
    routes, out = sequence(sw, world, fam, shared)
    assert np.array_equal(out["topk"], shared.fam_keys)
    first = plain(out["iter_a"])
    assert first == plain(out["iter_a_again"])
    check_iter(sw, out["iter_a"], shared.a_iter)
    rows, cal, n_pass = out["ranked"]
    want = shared.fam_ranked
    assert [r["id"] for r in rows] == want["ids"] and [r["score"] for r in rows] == want["scores"]
    assert n_pass == want["n_pass"] and (cal.a, cal.c, cal.sigma) == (want["calib"].a, want["calib"].c, want["calib"].sigma)
    check_iter(sw, out["iter_fam"], shared.fam_iter)
    assert np.array_equal(out["device"], world.full("A", 4, "b62x6-66-6", fill=hs.FILL))
    k1, k2 = out["topk_after_refine"]
    assert np.array_equal(k1, shared.fam_keys) and np.array_equal(k2, shared.fam_keys)
    assert np.array_equal(out["refined"], shared.fam_iter["rounds"][1]["table"])
    # the same steps on a second fresh handle take the same routes and give the same results
    routes2, out2 = sequence(sw, world, fam, shared)
    assert routes == routes2, [(a, b) for a, b in zip(routes, routes2) if a != b]
    assert plain(out2["iter_a"]) == first and plain(out2["iter_a_again"]) == first
    assert np.array_equal(out2["topk"], out["topk"]) and np.array_equal(out2["device"], out["device"])


# ---- f: main --iterations on a .swdb ---------------------------------------------------------
def test_main_iterations_on_a_swdb(sw, fam, tmp_path):
    qf, dbf, pf = tmp_path / "q.fasta", tmp_path / "family.swdb", tmp_path / "last.pssm"
    qf.write_text(">query\n" + "".join(LETTERS[c] for c in fam.q) + "\n")
    fam.db.save(str(dbf))
    run = subprocess.run([MAIN, "--query", str(qf), "--db", str(dbf), "--iterations", "2", "--topk", "70", "--write-pssm",
                          str(pf), "--matrix", "blosum62", "--gap-open", "11", "--gap-extend", "1"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    model = fam.model(2, 1e-3, 4096, k=70)
    assert not model["converged"]
    lib = fam.db.search_iter(fam.q, 2, k=70, matrix=fam.m, gap=11, gap_extend=1, final_pssm=True)
    check_iter(sw, dict(lib), model)
    want = ["# iteration %d included %d added %d dropped %d" % (t + 1, r["included"], r["added"], r["dropped"])
            for t, r in enumerate(lib["rounds"])]
    want.append("# stopped after 2")
    want += ["%d\t%d\t%.3g\t%.1f" % (r["id"], r["score"], r["evalue"], r["bits"]) for r in lib["rows"]]
    lines = run.stdout.split("\n")
    at = lines.index(want[0])
    assert lines[at:at + len(want)] == want
    rows, cons = sw.read_pssm(str(pf))
    assert np.array_equal(rows, model["rows"]) and cons == "".join(LETTERS[c] for c in fam.q)
