"""CPU: the inputs of tests/hits_envelope_support.py can tell a wrong hit-table
kernel from a right one.  Everything here is computed with the oracle alone,
so these are conditions on the inputs, not measurements of the library: the
GPU comparison on the same inputs (tests/test_gpu_hits_envelope.py) cannot
pass with a transposed profile index, with a wrong stored-code entry for B,
J, Z, X or *, with 16-bit values, with a best cell reduced in the wrong order
across waves or chunks, or with a tuple dropped where a wave reads its next
64 top cells or the ring wraps."""
import numpy as np
import pytest

import hits_envelope_support as hes
from conftest import path_score
from hits_envelope_support import SCORINGS


@pytest.fixture(scope="module")
def inputs(sw):
    return hes.build_inputs(sw)


@pytest.fixture(scope="module")
def want(oracle, inputs):
    return hes.Want(oracle, inputs)


def test_shape(sw, inputs):
    e = inputs
    C, wrows = sw.capi.HITS_CHUNK_ROWS, hes.wave_rows(sw)
    assert e.qlens == [40, wrows + 2, 375, C + 1, 1100]
    assert 2 * wrows < 375 < 3 * wrows and 2 * C < 1100 < 2 * C + wrows  # third wave; a short third chunk
    lens = [len(s) for s in e.subs]
    assert {1, 2, 39, 40, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257} <= set(lens)
    assert sum(700 <= n <= 1500 for n in lens[:78]) == 6 and len(e.subs) == 78 + 20 + len(e.column_seams)
    assert set(e.res.tolist()) == set(range(25))
    for q in e.queries[2:]:
        assert set(q.tolist()) == set(range(25))
    for name, m in e.mats.items():
        assert name in ("b50", "b62") or (m != m.T).any()
    d = np.diag(e.mats["idneg"]).astype(int)
    assert sorted(d[d <= 0].tolist()) == [-2, 0, 0] and (np.nonzero(d <= 0)[0] >= 20).sum() >= 2
    assert (e.mats["idneg"] != e.mats["asym"]).sum() == 3
    assert set(SCORINGS[s][0] for s in SCORINGS) <= set(e.mats)
    # per query of 375 and 1,100 rows and per seam: I runs of 1 and 5 rows in columns s - 1 and s,
    # D runs of 1 residue on both sides and of 5 that start on, cross and end on the seam
    assert len(e.column_seams) == 2 * 3 * (2 * 2 + 2 + 3)


def differing(a, b):
    return sum(x != y for x, y in zip(a, b))


@pytest.mark.parametrize("scname", ["asym-12-1", "asym-2-2", "d100-28-28", "pm100-1000-1000", "idneg-11-1"])
def test_wrong_index_shows(oracle, inputs, want, scname):
    """A transposed matrix, and two neighbouring columns or rows swapped among
    the codes 19..24 (what a wrong stored-code entry for B, J, Z, X or * does
    to the profile): each changes at least a quarter of the rows."""
    e = inputs
    mk, go, ge = SCORINGS[scname]
    m = e.mats[mk]
    wrong = {"transposed": np.ascontiguousarray(m.T)}
    for a in range(19, 24):
        perm = np.arange(25)
        perm[[a, a + 1]] = a + 1, a
        wrong["columns %d %d" % (a, a + 1)] = np.ascontiguousarray(m[:, perm])
        wrong["rows %d %d" % (a, a + 1)] = np.ascontiguousarray(m[perm, :])
    for qi in (e.qlens.index(40), e.qlens.index(375)):
        rows = want.rows(scname, qi)
        for what, wm in wrong.items():
            assert (wm != m).any()
            n = differing(rows, hes.rows_under(oracle, e.queries[qi], e.subs, wm, go, ge))
            print("%s q%d %s: %d of %d rows differ" % (scname, e.qlens[qi], what, n, len(rows)))
            assert 4 * n >= len(rows), (scname, e.qlens[qi], what, n)


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_gaps_and_paths(inputs, want, scname):
    """Half of a scoring's rows hold a gap (but where no gap can pay); every
    reported score is its path's own (a run's further residues cost min(open,
    extend): with open below extend the recurrence opens anew from H, which
    its gap column just set); nonpos is all-zero."""
    e = inputs
    mk, go, ge = SCORINGS[scname]
    gapped = total = 0
    for qi, q in enumerate(e.queries):
        rows, als = want.rows(scname, qi), want.als(scname, qi)
        n = sum(r["gaps"] > 0 for r in rows)
        print("%s q%d: %d of %d rows with a gap" % (scname, len(q), n, len(rows)))
        gapped, total = gapped + n, total + len(rows)
        if mk == "nonpos":
            assert not any(r["score"] for r in rows)
        for al, s in zip(als[::7], e.subs[::7]):
            if al["score"]:
                assert path_score(q, s, e.mats[mk], go, min(go, ge), al) == al["score"]
    if mk != "nonpos" and scname != "pm100-1000-1000":
        assert 2 * gapped >= total, (scname, gapped, total)


@pytest.mark.parametrize("scname,sign", [("idneg-11-1", 1), ("pm100-1000-1000", 1), ("asym-12-1", -1), ("pm100-3-1", -1)])
def test_identities_against_positives(inputs, want, scname, sign):
    for qi in range(len(inputs.queries)):
        n = sum(sign * (r["identities"] - r["positives"]) > 0 for r in want.rows(scname, qi))
        print("%s q%d: %d rows with identities %s positives" % (scname, inputs.qlens[qi], n, "<>"[sign > 0]))
        if inputs.qlens[qi] >= 375:  # (the issue asks for 10 rows of a scoring: here of each longer query)
            assert n >= 10, (scname, qi, n)


def test_scale(inputs, want):
    best = max(r["score"] for r in want.rows("d100-40-28", len(inputs.queries) - 1))
    assert best > 100000  # no 16-bit value holds it


def linear_dp(q, s, m, g):
    """H of the linear-gap recurrence, [len(q), len(s)] (plain numpy: a row's
    left-to-right gap chain is a running maximum of t[k] + g k)."""
    ramp = g * np.arange(len(s), dtype=np.int64)
    H = np.zeros((len(q) + 1, len(s) + 1), dtype=np.int64)
    sub = m.astype(np.int64)[:, s]
    for i in range(1, len(q) + 1):
        t = np.maximum(np.maximum(H[i - 1, :-1] + sub[q[i - 1]], H[i - 1, 1:] - g), 0)
        H[i, 1:] = np.maximum.accumulate(t + ramp) - ramp
    return H[1:, 1:]


@pytest.mark.parametrize("qlen,per,least", [(375, "wave", 15), (1100, "chunk", 10)])
def test_tied_best_cells_across_seams(sw, inputs, want, qlen, per, least):
    """Under pm100-1000-1000 many subjects reach their best score at cells of
    more than one wave (one chunk) or of more than one chunk: the reduction by
    (value, row, column) across waves and chunks decides their rows."""
    e = inputs
    mk, go, ge = SCORINGS["pm100-1000-1000"]
    assert go == ge
    qi = e.qlens.index(qlen)
    rows_per = hes.wave_rows(sw) if per == "wave" else sw.capi.HITS_CHUNK_ROWS
    spread = 0
    for s, row in zip(e.subs, want.rows("pm100-1000-1000", qi)):
        H = linear_dp(e.queries[qi], s, e.mats[mk], go)
        assert H.max() == row["score"]
        if row["score"] > 0:
            at = np.nonzero((H == H.max()).any(axis=1))[0]
            assert at[0] == row["q_end"] - 1  # the first one in row-major order is the oracle's
            spread += len(set((at // rows_per).tolist())) > 1
    print("q%d: %d subjects with tied best cells in more than one %s" % (qlen, spread, per))
    assert spread >= least


def seam_run_rows(al, kind, s):
    """Query rows of the runs of `kind` that lie on column seam s."""
    return [rr for (op, rr), (_, cols) in zip(hes.run_rows(al), hes.run_columns(al)) if op == kind and hes.on_seam(cols, s)]


def test_column_seam_runs(sw, inputs, want):
    """Under BLOSUM62 11 / 1 each column-seam subject's path holds a gap run of
    the planted kind and length on its seam column, with the run's query rows
    away from every wave seam."""
    e = inputs
    wrows = hes.wave_rows(sw)
    for k, qi, s, kind, L in e.column_seams:
        al = want.als("b62-11-1", qi)[k]
        runs = seam_run_rows(al, kind, s)
        assert len(runs) == 1, (k, qi, s, kind, L, al)
        if kind == "I":
            assert len(runs[0]) == L
        assert all(min(r % wrows, wrows - r % wrows) >= hes.SEAM_ROW_MARGIN for r in runs[0]), (k, s, kind, runs)


@pytest.mark.parametrize("scname", ["asym-12-1", "idneg-11-1", "d100-40-28"])
def test_column_seam_runs_under_other_matrices(inputs, want, scname):
    """Where a mismatch may score above a match a run can move off its seam:
    still, under a gap that costs more than a mismatch, for each query, seam
    and kind of run some subject keeps one on it."""
    e = inputs
    kept = {}
    for k, qi, s, kind, L in e.column_seams:
        kept[(qi, s, kind)] = kept.get((qi, s, kind), 0) + bool(seam_run_rows(want.als(scname, qi)[k], kind, s))
    print(scname, kept)
    assert len(kept) == 12 and all(kept.values()), kept


@pytest.mark.parametrize("scname", [s for s in SCORINGS if SCORINGS[s][0] != "nonpos"])
def test_every_code_lies_on_a_path(inputs, want, scname):
    e = inputs
    qcodes, scodes = set(), set()
    for qi, q in enumerate(e.queries):
        for al, s in zip(want.als(scname, qi), e.subs):
            a, b = hes.path_codes(al, q, s)
            qcodes |= a
            scodes |= b
    assert qcodes == set(range(25)) and scodes == set(range(25)), (scname, qcodes, scodes)
