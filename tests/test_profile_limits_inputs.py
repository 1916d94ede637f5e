"""CPU: the inputs of tests/test_gpu_profile_limits.py have the properties its
cases rely on, shown with the numpy model (tests/profile_support.py) and the
PSSM oracle (tests/native/pssm_oracle.cpp) alone: the many-hits input spans
three launch groups whose boundaries are no multiple of its period, the loop
input takes the branches the first loop test never took, the custom ids
change nothing but the ids, every envelope scoring puts gaps (and the +-100
table its extreme entries) on the paths, and the clamp input leaves the
clamp's range on both sides.  The conditions are asserted, the figures
printed.  The clamp case also compares the library's host-only
sw_pssm_from_counts with the model."""
import re

import numpy as np
import pytest

import profile_support as ps
import pssm_support


@pytest.fixture(scope="module")
def po(tmp_path_factory):
    return pssm_support.PssmOracle(tmp_path_factory.mktemp("limits_oracle"))


def test_align_group_ends_restates_the_plan():
    """The three facts tests/native/hits_check.cpp pins for
    swplan::align_groups (its CHECKs, and the line it prints: "align_groups:
    budget 1073741824, three-hit ends 1 3"), from the restated rule."""
    assert ps.align_group_ends(16383, [16385, 16385, 100]) == [1, 3]
    exact = sum((9 + L + 1) * 10 for L in (7, 12, 30))
    assert ps.align_group_ends(9, [7, 12, 30], exact) == [3]
    assert ps.align_group_ends(9, [7, 12, 30], exact - 1) == [2, 3]
    assert ps.align_group_ends(9, []) == [] and ps.align_group_ends(9, [5000000000]) == [1]


# ---- many hits ------------------------------------------------------------------------
@pytest.mark.parametrize("mid, go, ge", [(1, 11, 1), (0, 2, 2)])
def test_many_hits_input(sw, po, mid, go, ge):
    q, subjects, ids = ps.many_hits_input()
    lens = np.array([len(s) for s in subjects])
    assert len(q) == 600 and 25 <= int((q >= 20).sum()) <= 35 and len(subjects) == 47 and len(ids) == 4096
    assert lens.min() >= 380 and lens.max() <= 550
    assert len({s.tobytes() for s in subjects}) == 47 and set(ids.tolist()) == set(range(47))
    ends = ps.align_group_ends(600, lens[ids])
    print("group ends", ends)
    assert len(ends) >= 3 and ends[-1] == 4096
    assert all(e % 47 for e in ends[:-1]) and ends[-1] % 47
    # a group's first rows differ from the first rows of the call: rows written at offset 0 of every group show
    for e in ends[:-1]:
        assert not np.array_equal(ids[e:e + 47], ids[:47])
    m = sw.capi.builtin_matrix(mid)
    rows = pssm_support.derived(q, m)
    aligns = [po.align(rows, s, go, ge) for s in subjects]
    assert all("D" in a["ops"] for a in aligns)
    for master in (q, None):
        msa = ps.msa_of(600, master, [subjects[i] for i in ids], [aligns[i] for i in ids])
        assert (msa == ps.GAP).any()
        cnt, weight, wsum = ps.tables(msa)
        T = wsum.astype(object).sum(axis=1)
        assert (T == 0).any() and int(wsum.max()) < 2 ** 43
        if master is not None:  # a position of codes 20..24 that nothing counted covers: the prior row is carried
            assert ((T == 0) & (q >= 20)).any()
        _, raw = ps.pssm_from_counts(cnt, wsum, rows, m, 10.0)
        print("many hits", mid, go, ge, "master" if master is not None else "no master", "T_i = 0 at", int((T == 0).sum()),
              "margin", ps.half_margin(raw))
        assert ps.half_margin(raw) > 1e-6


# ---- the loop's branches -----------------------------------------------------------------
def trace(model):
    out, prev = [], set()
    for r in model["rounds"]:
        cur = set(r["ids"])
        out.append((len(cur), len(cur - prev), len(prev - cur)))
        prev = cur
    return out


@pytest.fixture(scope="module")
def family():
    return ps.family_database()


@pytest.fixture(scope="module")
def capped(sw, po, family):
    q, res, offs = family
    return ps.search_iter_model(sw.capi, po, q, sw.capi.builtin_matrix(1), 11, 1, res, offs, 6, 10.0, 64, 10.0, 500, None)


def test_loop_branches(capped):
    t = trace(capped)
    print("inclusion 10, include_max 64:", t, "passed", [r["n_pass"] for r in capped["rounds"]], "margin", capped["margin"])
    assert any(d > 0 for _, _, d in t)
    assert any(a == d > 0 for _, a, d in t)  # the round a count-only convergence test stops in
    assert capped["rounds"][0]["n_pass"] < 64 < capped["rounds"][1]["n_pass"] and t[1][0] == 64  # the cap truncates
    assert any(i >= 60 for r in capped["rounds"] for i in r["ids"])  # a random subject is included
    # converged in the last round it was allowed: the same run cut at 4 rounds stops unconverged (the
    # model is deterministic: its first 4 rounds are these, and none of them repeated its predecessor)
    assert capped["converged"] and 4 < capped["rounds_run"] <= 6
    assert all(a or d for _, a, d in t[:4])
    assert capped["margin"] > 1e-6


def test_loop_small_caps(sw, po, family):
    q, res, offs = family
    m = sw.capi.builtin_matrix(1)
    for cap in (10, 1):
        o = ps.search_iter_model(sw.capi, po, q, m, 11, 1, res, offs, 6, 1e-3, cap, 10.0, 500, None)
        print("inclusion 1e-3, include_max", cap, trace(o), "margin", o["margin"])
        assert o["converged"] and trace(o)[-1] == (cap, 0, 0) and o["margin"] > 1e-6
        assert o["rounds"][-1]["n_pass"] > cap


# ---- ids ---------------------------------------------------------------------------------
def test_custom_ids_change_only_the_ids(sw, po, family, capped):
    q, res, offs = family
    n = len(offs) - 1
    ids = ps.custom_ids(n)
    assert len(set(ids.tolist())) == n and ids.min() >= 7 and ids.max() >= 10 * n and (np.diff(ids) < 0).any()
    lens = np.diff(offs)
    assert (lens[:60] >= ps.FAMILY_LONG_THRESHOLD).sum() >= 10 and (lens[:60] < ps.FAMILY_LONG_THRESHOLD).sum() >= 10
    o = ps.search_iter_model(sw.capi, po, q, sw.capi.builtin_matrix(1), 11, 1, res, offs, 6, 10.0, 64, 10.0, 500, None, ids=ids)
    assert o["rounds_run"] == capped["rounds_run"] and o["converged"] == capped["converged"]
    for a, b in zip(capped["rounds"], o["rounds"]):
        # the tie order follows the ids, so the sets could differ where scores tie at the cut: they do not
        assert sorted(int(ids[i]) for i in a["ids"]) == b["ids"]
        assert a["n_pass"] == b["n_pass"]
    assert np.array_equal(o["rows"], capped["rows"])
    assert sorted(o["ids"]) != sorted(capped["ids"])  # the report's ids are the custom ones
    assert [o["index_of"][i] for i in o["ids"]] != capped["ids"]  # ... and its tie order follows them
    assert sorted(o["index_of"][i] for i in o["ids"][:100]) == sorted(capped["ids"][:100])


# ---- the envelope's scorings -----------------------------------------------------------
def on_path(rows, s, al):
    """The table's entries under the alignment's M columns."""
    i, j, out = al["q_begin"] - 1, al["s_begin"] - 1, []
    for op in al["ops"]:
        if op == "M":
            out.append(int(rows[i][s[j]]))
        i += op != "D"
        j += op != "I"
    return out


@pytest.mark.parametrize("name", ["specific-1-4", "specific-1000-1000", "scaled-28-28", "scaled-40-3", "m100-11-1"])
def test_envelope_scorings(sw, po, name):
    q0, table, subjects, ids = ps.envelope_input()
    assert len(q0) == 375 and len(subjects) == 150 and set(np.concatenate(subjects).tolist()) == set(range(25))
    assert int(table.max()) <= 15 and int(table.min()) == -8 and (table.argmax(axis=1) == q0).all()
    rows, go, ge, mat = ps.envelope_scorings(q0, table, sw.capi.builtin_matrix(1))[name]
    sel = [subjects[i] for i in ids]
    aligns = [po.align(rows, s, go, ge) for s in sel]
    msa = ps.msa_of(375, ps.envelope_master(name, q0), sel, aligns)
    assert (msa[1:] == ps.GAP).any() and any("D" in a["ops"] for a in aligns)
    best = max(a["score"] for a in aligns)
    if name.startswith("scaled") or name == "m100-11-1":
        assert int(rows.max()) == 100 and int(rows.min()) == -100
        # past int16, and more than 40 rows of 100 could give: entries of 100 lie on paths
        assert best > 32767
        assert any(100 in on_path(rows, s, a) for s, a in zip(sel, aligns))
    if name == "specific-1-4":
        assert max(len(x) for a in aligns for x in re.findall("I+", a["ops"])) > 1
        assert max(len(x) for a in aligns for x in re.findall("D+", a["ops"])) > 1
    cnt, weight, wsum = ps.tables(msa)
    for pseudo in (10.0, 0.5):
        _, raw = ps.pssm_from_counts(cnt, wsum, rows, mat, pseudo)
        print(name, "best", best, "pseudo", pseudo, "margin", ps.half_margin(raw), "raw", np.nanmin(raw), np.nanmax(raw))
        assert ps.half_margin(raw) > 1e-6
        if name == "m100-11-1":  # the clamp is reached through the device path too
            assert np.nanmax(raw) > 100.5 and np.nanmin(raw) < -100.5


# ---- the clamp --------------------------------------------------------------------------
def test_clamp_is_reached_and_equals_the_model(sw):
    msa = ps.clamp_rows()
    m = ps.matrix_100()
    assert msa.shape == (40, 30) and sorted(set(msa[:, 4].tolist())) == [0, 17] and (msa[:, 4] == 17).sum() == 1
    cnt, weight, wsum = ps.tables(msa)
    prior = pssm_support.derived(msa[0], m)
    for pseudo in (10.0, 0.5):
        want, raw = ps.pssm_from_counts(cnt, wsum, prior, m, pseudo)
        print("clamp: raw", np.nanmin(raw), np.nanmax(raw), "outside", int((np.abs(raw) > 100.5).sum()), "margin",
              ps.half_margin(raw))
        assert (raw > 100.5).any() and (raw < -100.5).any() and ps.half_margin(raw) > 1e-6
        assert int(want[:, :20].max()) == 100 and int(want[:, :20].min()) == -100
        got = sw.capi.pssm_from_counts(cnt, wsum, prior, m, pseudo)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
