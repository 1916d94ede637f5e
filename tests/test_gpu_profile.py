"""GPU: the iterated profile search (include/sw_amd.h "iterated profile
search"): the query-anchored rows the traceback's walk writes (sw_align.hip),
the integer profile tables (sw_msa.hip), sw_pssm_refine, sw_search_iter and
main --iterations, against the numpy model in tests/profile_support.py.

Rows and tables are bytes and integers: compared exactly.  A refined table
is compared exactly after asserting that the model's unrounded entries for
the test's inputs keep 1e-6 from every half-integer.  "11/1" is gap_open 11,
gap_extend 1 (the model on the family database then includes 4, 48 and 60
members, as the issue records)."""
import os
import subprocess

import numpy as np
import pytest

import profile_support as ps
import pssm_support

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "ece1782-smith-waterman-cuda_amd", "lib", "main")
GAPS = [(2, 2), (11, 1)]
QLENS = [1, 63, 64, 65, 300]
TILE = 64  # csrc/sw_kernels.h kMsaTile: columns per workgroup of the column kernels
LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"


@pytest.fixture(scope="module")
def po(tmp_path_factory):
    return pssm_support.PssmOracle(tmp_path_factory.mktemp("profile_oracle"))


def small_subjects():
    """40 subjects of 0..300 residues: an empty one, one of '*' alone (scores 0
    against a table of a query without '*'), mutated pieces of the 300-residue
    query with indels (alignments with I and D runs), random ones over all 25
    codes; a query of codes 0..19 whose prefixes are the shorter queries."""
    rng = np.random.default_rng(11)
    q = rng.integers(0, 20, size=300).astype(np.uint8)
    subj = [np.zeros(0, dtype=np.uint8), np.full(20, 24, dtype=np.uint8)]
    for k in range(24):
        a = int(rng.integers(0, 200))
        b = a + int(rng.integers(20, 100))
        s = q[a:b].copy()
        sub = rng.random(len(s)) < 0.25
        s[sub] = rng.integers(0, 25, size=int(sub.sum()))
        d = int(rng.integers(2, len(s) - 6))
        s = np.delete(s, slice(d, d + int(rng.integers(1, 4))))
        i = int(rng.integers(2, len(s) - 2))
        s = np.insert(s, i, rng.integers(0, 20, size=int(rng.integers(1, 4))))
        s = np.concatenate([rng.integers(0, 25, size=int(rng.integers(0, 30))), s,
                            rng.integers(0, 25, size=int(rng.integers(0, 30)))]).astype(np.uint8)
        subj.append(s[:300])
    subj += [q[:k].copy() for k in (1, 64, 65)]  # the query's own prefixes: full-length M runs
    subj.append(q.copy())
    while len(subj) < 40:
        subj.append(rng.integers(0, 25, size=int(rng.integers(1, 301))).astype(np.uint8))
    offs = np.zeros(len(subj) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subj])
    return {"q": q, "subj": subj, "res": np.concatenate(subj).astype(np.uint8), "offs": offs,
            "ids": np.array(list(range(40)) + [3, 3, 39], dtype=np.int32)}  # ids may repeat


@pytest.fixture(scope="module")
def small(sw, handle):
    d = small_subjects()
    d["db"] = sw.Database(handle, d["res"], d["offs"])
    yield d
    d["db"].close()


_expected = {}


def expected_msa(sw, po, small, qlen, gaps, with_master):
    """The model's rows of one case, computed once (PssmOracle.align's ops replayed)."""
    key = (qlen, gaps, with_master)
    if key not in _expected:
        go, ge = gaps
        q = small["q"][:qlen]
        rows = pssm_support.derived(q, sw.capi.builtin_matrix(1))
        subjects = [small["subj"][i] for i in small["ids"]]
        aligns = [po.align(rows, s, go, ge) for s in subjects]
        _expected[key] = (rows, aligns, ps.msa_of(qlen, q if with_master else None, subjects, aligns))
    return _expected[key]


@pytest.mark.parametrize("with_master", [True, False])
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("qlen", QLENS)
def test_msa_rows_equal_the_replayed_alignments(sw, handle, po, small, qlen, gaps, with_master):
    go, ge = gaps
    rows, aligns, want = expected_msa(sw, po, small, qlen, gaps, with_master)
    q = small["q"][:qlen]
    p = sw.Pssm(handle, rows)
    got, al = small["db"].msa_pssm(p, small["ids"], master=q if with_master else None, gap=go, gap_extend=ge)
    assert got.shape == (len(small["ids"]) + 1, qlen) and got.dtype == np.uint8
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the empty subject and the one that scores 0: exactly NONE; so is every unused position
    assert aligns[1]["score"] == 0 and (got[1] == ps.NONE).all() and (got[2] == ps.NONE).all()
    for k, a in enumerate(aligns):
        if a["score"] > 0:
            span = np.zeros(qlen, dtype=bool)
            span[a["q_begin"] - 1:a["q_end"]] = True
            assert (got[1 + k][~span] == ps.NONE).all() and (got[1 + k][span] != ps.NONE).all()
            assert (al[k]["score"], al[k]["q_begin"], al[k]["q_end"]) == (a["score"], a["q_begin"], a["q_end"])
    if qlen == 300:
        assert (got == ps.GAP).any() and any("D" in a["ops"] for a in aligns)  # the cases hold I and D runs
    # sw_align_pssm is unchanged by the rows' pointer: the same call with ops still spells the oracle's path
    if qlen == 65:
        full = small["db"].align_pssm(p, small["ids"][:30], gap=go, gap_extend=ge)
        for k in range(30):
            assert full[k]["ops"] == (aligns[k]["ops"] if aligns[k]["score"] > 0 else "")
    p.close()


@pytest.mark.parametrize("with_master", [True, False])
@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("qlen", QLENS)
def test_profile_counts_equal_the_model(sw, handle, po, small, qlen, gaps, with_master):
    go, ge = gaps
    rows, aligns, msa = expected_msa(sw, po, small, qlen, gaps, with_master)
    p = sw.Pssm(handle, rows)
    cnt, weight, wsum = small["db"].profile_counts(p, small["ids"], master=small["q"][:qlen] if with_master else None,
                                                   gap=go, gap_extend=ge)
    wc, ww, ws = ps.tables(msa)
    assert np.array_equal(cnt, wc) and np.array_equal(weight, ww) and np.array_equal(wsum, ws)
    p.close()


def synthetic_rows(nrows, qlen, seed):
    """Rows over every byte value 0..26 with the seams the kernels have: column
    0 holds all 20 residues (as far as the rows reach), column 1 gaps only,
    column 2 codes 20..24 only, the last column one residue; every seventh row
    is all NONE."""
    rng = np.random.default_rng(seed)
    msa = rng.integers(0, 27, size=(nrows, qlen)).astype(np.uint8)
    msa[:, 0] = np.arange(nrows) % 20
    msa[:, 1] = ps.GAP
    msa[:, 2] = 20 + np.arange(nrows) % 5
    msa[:, qlen - 1] = 7
    msa[6::7] = ps.NONE
    return msa


@pytest.mark.parametrize("nrows", [1, 2, 64, 65, 4097])
@pytest.mark.parametrize("qlen", [TILE - 1, TILE, TILE + 1])
def test_profile_counts_msa_seams(sw, handle, qlen, nrows):
    msa = synthetic_rows(nrows, qlen, 100 * qlen + nrows)
    cnt, weight, wsum = sw.capi.profile_counts_msa(handle, msa)
    wc, ww, ws = ps.tables(msa)
    assert np.array_equal(cnt, wc), np.argwhere(cnt != wc)[:5]
    assert np.array_equal(weight, ww), np.argwhere(weight != ww)[:5]
    assert np.array_equal(wsum, ws), np.argwhere(wsum != ws)[:5]
    k = (cnt > 0).sum(axis=1)
    assert k[1] == 0 and k[2] == 0 and not wsum[1].any()  # gaps only; codes 20..24 only
    assert k[0] == (20 if nrows >= 64 else nrows) and k[qlen - 1] == 1  # (rows 0 and 1 are not all-NONE ones)
    assert (weight[6::7] == 0).all()  # all-NONE rows weigh nothing
    assert int(wsum.max()) < 2 ** 43


def test_profile_counts_limits(sw, handle, small):
    with pytest.raises(sw.SWError, match="-1"):
        sw.capi.profile_counts_msa(handle, np.zeros((4098, 3), dtype=np.uint8))
    with pytest.raises(sw.SWError, match="-1"):
        sw.capi.profile_counts_msa(handle, np.zeros((0, 3), dtype=np.uint8))
    rows = pssm_support.derived(small["q"][:8], sw.capi.builtin_matrix(1))
    p = sw.Pssm(handle, rows)
    with pytest.raises(sw.SWError, match="-1"):
        small["db"].profile_counts(p, np.zeros(4097, dtype=np.int32))
    with pytest.raises(sw.SWError, match="-1.*not in the database"):
        small["db"].profile_counts(p, [0, 40])
    with pytest.raises(sw.SWError, match="-1"):
        small["db"].msa_pssm(p, [0], master=np.full(8, 25, dtype=np.uint8))
    # no position: one weight per row, nothing else
    cnt, weight, wsum = sw.capi.profile_counts_msa(handle, np.zeros((3, 0), dtype=np.uint8))
    assert cnt.shape == (0, 20) and weight.tolist() == [0, 0, 0]
    assert np.array_equal(p.rows(), rows)
    p.close()


@pytest.mark.parametrize("gaps", GAPS)
@pytest.mark.parametrize("qlen", [65, 300])
def test_refine_equals_the_model(sw, handle, po, small, qlen, gaps):
    go, ge = gaps
    m = sw.capi.builtin_matrix(1)
    q = small["q"][:qlen]
    rows, aligns, msa = expected_msa(sw, po, small, qlen, gaps, True)
    cnt, weight, wsum = ps.tables(msa)
    want, raw = ps.pssm_from_counts(cnt, wsum, rows, m, 10.0)
    margin = ps.half_margin(raw)
    print("half-integer margin", qlen, gaps, margin)
    assert margin > 1e-6, "the model's own values are too close to a rounding edge for these inputs"
    p = sw.Pssm(handle, rows)
    new = small["db"].refine_pssm(p, small["ids"], master=q, matrix=m, pseudo=10.0, gap=go, gap_extend=ge)
    got = new.rows()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not np.array_equal(got, rows)  # the hits moved the table
    # a second step from the refined table (a real PSSM as the prior and as the aligner's scores)
    subjects = [small["subj"][i] for i in small["ids"]]
    want2, raw2, _ = ps.refine_model(po, want, q, subjects, go, ge, m, 10.0)
    assert ps.half_margin(raw2) > 1e-6
    again = small["db"].refine_pssm(new, small["ids"], master=q, matrix=m, gap=go, gap_extend=ge)
    assert np.array_equal(again.rows(), want2)
    again.close()
    new.close()
    p.close()


@pytest.mark.parametrize("mid, go, ge", [(1, 11, 1), (0, 2, 2)])
def test_refine_without_hits_is_the_derived_table(sw, handle, small, mid, go, ge):
    """n = 0 and a master: every position has one observed residue, so the
    result is the table the master stands for, and it scans as sw_scan does."""
    m = sw.capi.builtin_matrix(mid)
    q = small["q"][:130]
    derived = pssm_support.derived(q, m)
    blank = sw.Pssm(handle, np.full((130, 25), -3, dtype=np.int8))  # the prior's columns 20..24 are carried
    new = small["db"].refine_pssm(blank, [], master=q, matrix=m, gap=go, gap_extend=ge)
    got = new.rows()
    assert np.array_equal(got[:, :20], derived[:, :20]) and (got[:, 20:] == -3).all()
    p = sw.Pssm(handle, derived)
    same = small["db"].refine_pssm(p, [], master=q, matrix=m, gap=go, gap_extend=ge)
    assert np.array_equal(same.rows(), derived)
    assert np.array_equal(small["db"].scan_pssm(same, go, ge), small["db"].scan(q, m, go, ge))
    # no master either: nothing observed, the prior itself
    prior = small["db"].refine_pssm(p, [], matrix=m, gap=go, gap_extend=ge)
    assert np.array_equal(prior.rows(), derived)
    for x in (blank, new, p, same, prior):
        x.close()


# ---- the iterated search ---------------------------------------------------------------
@pytest.fixture(scope="module")
def family(sw, handle, po):
    q, res, offs = ps.family_database()
    m = sw.capi.builtin_matrix(1)
    model = ps.search_iter_model(sw.capi, po, q, m, 11, 1, res, offs, 5, 1e-3, 4096, 10.0, 500, None)
    db = sw.Database(handle, res, offs)
    yield {"q": q, "res": res, "offs": offs, "m": m, "model": model, "db": db}
    db.close()


def test_the_model_alone_finds_the_family(family):
    """What the search is for, on the CPU model alone: the query finds a few
    members, the profile finds the family, no random subject comes in, and no
    refined entry sat on a rounding edge."""
    rounds = family["model"]["rounds"]
    counts = [len(r["ids"]) for r in rounds]
    print("model rounds", counts, "converged", family["model"]["converged"], "margin", family["model"]["margin"])
    assert 0 < counts[0] < 10
    assert sum(i < 60 for i in rounds[-1]["ids"]) >= 55
    assert all(i < 60 for r in rounds for i in r["ids"])
    assert family["model"]["converged"] and family["model"]["rounds_run"] < 5
    assert family["model"]["margin"] > 1e-6


def test_search_iter_equals_the_model(sw, family):
    model, db, q, m = family["model"], family["db"], family["q"], family["m"]
    out = db.search_iter(q, 5, inclusion_evalue=1e-3, include_max=4096, pseudo=10.0, k=500, matrix=m, gap=11,
                         gap_extend=1, final_pssm=True)
    assert out["converged"] == model["converged"] and len(out["rounds"]) == model["rounds_run"]
    prev = set()
    for t, (got, want) in enumerate(zip(out["rounds"], model["rounds"])):
        cur = set(want["ids"])
        assert (got["included"], got["added"], got["dropped"]) == (len(cur), len(cur - prev), len(prev - cur)), t
        prev = cur
    # every round's included set: a search stopped after t rounds reports I_t when the report's
    # bounds are the inclusion's
    for t in range(1, model["rounds_run"] + 1):
        o = db.search_iter(q, t, inclusion_evalue=1e-3, include_max=4096, k=4096, max_evalue=1e-3, matrix=m, gap=11,
                           gap_extend=1)
        assert [r["id"] for r in o["rows"]] == model["rounds"][t - 1]["order"], t
        assert o["n_pass"] == len(model["rounds"][t - 1]["ids"])
        assert o["converged"] == (model["converged"] and t == model["rounds_run"])
    inc = [set(r["ids"]) for r in model["rounds"]]
    assert len(inc[0]) < 10 and len(inc[-1] & set(range(60))) >= 55 and not (inc[-1] - set(range(60)))
    # the report: the last round's scores under (k, no cutoff)
    assert [r["id"] for r in out["rows"]] == model["ids"]
    assert [r["score"] for r in out["rows"]] == model["scores"]
    assert out["n_pass"] == model["n_pass"]
    for f in ("a", "c", "sigma"):
        assert getattr(out["calib"], f) == getattr(model["calib"], f)
    for r in out["rows"][:80]:
        e, bits, z = sw.capi.calib_sig(out["calib"], r["score"], int(model["lengths"][r["id"]]))
        assert (r["evalue"], r["bits"], r["z"]) == (e, bits, z)
    assert np.array_equal(out["pssm"].rows(), model["rows"])
    out["pssm"].close()


def test_search_iter_arguments(sw, family):
    db, q, m = family["db"], family["q"], family["m"]
    one = db.search_iter(q, 1, k=5, matrix=m, gap=11, gap_extend=1)
    assert len(one["rounds"]) == 1 and not one["converged"] and len(one["rows"]) == 5
    ranked, _, _ = db.scan_pssm_topk_ranked(sw.Pssm(db.handle, pssm_support.derived(q, m)), 5, gap_open=11, gap_extend=1)
    assert [r["id"] for r in one["rows"]] == [r["id"] for r in ranked]  # round 1 is the query's own search
    for bad in (dict(rounds=0), dict(include_max=0), dict(include_max=4097), dict(k=0), dict(k=4097),
                dict(inclusion_evalue=0.0), dict(max_evalue=-1.0), dict(pseudo=0.0), dict(pseudo=float("nan"))):
        kw = dict(rounds=2, k=5, matrix=m, gap=11, gap_extend=1)
        kw.update(bad)
        rounds = kw.pop("rounds")
        with pytest.raises(sw.SWError, match="-1"):
            db.search_iter(q, rounds, **kw)
    with pytest.raises(sw.SWError, match="-5"):
        db.search_iter(q, 2, k=5, matrix=np.full(625, 3, dtype=np.int8), gap=11, gap_extend=1)


# ---- main --iterations ------------------------------------------------------------------
def test_main_iterations_prints_the_trace_and_writes_the_profile(sw, family, tmp_path):
    q, res, offs, m = family["q"], family["res"], family["offs"], family["m"]
    qf, dbf, pf = tmp_path / "q.fasta", tmp_path / "db.fasta", tmp_path / "last.pssm"
    qf.write_text(">query\n" + "".join(LETTERS[c] for c in q) + "\n")
    with open(dbf, "w") as f:
        for i in range(len(offs) - 1):
            f.write(">%d\n%s\n" % (i, "".join(LETTERS[c] for c in res[offs[i]:offs[i + 1]])))
    scoring = ["--matrix", "blosum62", "--gap-open", "11", "--gap-extend", "1"]
    run = subprocess.run([MAIN, "--query", str(qf), "--db", str(dbf), "--iterations", "3", "--topk", "70",
                          "--write-pssm", str(pf)] + scoring, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lib = family["db"].search_iter(q, 3, k=70, matrix=m, gap=11, gap_extend=1, final_pssm=True)
    want = ["# iteration %d included %d added %d dropped %d" % (t + 1, r["included"], r["added"], r["dropped"])
            for t, r in enumerate(lib["rounds"])]
    want.append("# converged" if lib["converged"] else "# stopped after 3")
    want += ["%d\t%d\t%.3g\t%.1f" % (r["id"], r["score"], r["evalue"], r["bits"]) for r in lib["rows"]]
    lines = run.stdout.split("\n")
    at = lines.index(want[0])
    assert lines[at:at + len(want)] == want
    assert lines[at + len(want)].startswith("=====")
    # the written profile is the last round's, and main --pssm reproduces its scores
    rows, cons = sw.read_pssm(str(pf))
    assert np.array_equal(rows, lib["pssm"].rows()) and cons == "".join(LETTERS[c] for c in q)
    again = subprocess.run([MAIN, "--pssm", str(pf), "--db", str(dbf), "--topk", "25", "--gap-open", "11",
                            "--gap-extend", "1"], capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stderr
    keys = family["db"].scan_pssm_topk(lib["pssm"], 25, 11, 1)
    ids, scores = sw.capi.decode_keys(keys)
    got = [ln for ln in again.stdout.split("\n") if ":" in ln and ln.split(":")[0].isdigit()]
    assert got == ["%d:%d" % (i, s) for i, s in zip(ids, scores)]
    lib["pssm"].close()
