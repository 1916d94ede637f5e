"""CPU: what the inputs of tests/length_support.py can see, with the oracle
alone.  tests/test_gpu_lengths.py compares every kernel family with the oracle
on subjects and queries past 2^15 and 2^16; that comparison is worth what the
inputs make depend on the far columns and rows.  Shown here, under both plain
scorings:

  * a giant's score is its end piece's own score (columns L - 937 .. L - 373
    under the 568-row query) and nothing else reaches it: the subject cut at 32,767, 32,768,
    65,535 or 65,536 columns scores strictly less wherever the cut takes a
    column of the end piece, the subject of L mod 2^15 or L mod 2^16 columns
    (a count that wrapped) scores strictly less for every giant longer than
    the power, and the subject whose columns are read mod 2^16 or mod 2^15
    (s[:P] + s[:L - P]: an index that wrapped) scores strictly less wherever
    the end piece has a column from P on.  The piece ends 372 columns
    before the subject's end, so a cut behind it (32,767 of 32,768; 65,535 of
    65,536; both of 65,544) changes nothing, which is asserted too; the cuts
    at 2^15 are seen by five giants, those at 2^16 by the longest alone.
  * each cross piece, aligned alone against its window of the giant, holds its
    single gap run on the planted columns;
  * the best alignment begins past 2^15 in the five giants longer than it (past
    64,500 in the three of 65,536 and more, past 2^16 in the longest);
  * a long query cut at 32,767 or 65,535 rows, or read with its rows mod 2^16,
    changes the score of every subject planted past that row, and at least 10
    subjects per region begin (q_begin) past the power;
  * T's two top scores are past fp16 and int16; under the scaled scorings every
    giant passes the fp16 guard and, with the 900-row prefix query, the int16
    one; sw_align's direction array is past 2^30 bytes for 32,776 x 300 and
    past 2^32 for 65,544 x 300."""
import numpy as np
import pytest

import length_support as ls
import seam_support as ss

P15, P16 = ls.P15, ls.P16


@pytest.fixture(scope="module")
def G():
    return ls.giants()


def mat_of(oracle, mid, k=1):
    return ls.scaled(oracle.matrix(mid), k)


def test_giants_shape(G):
    assert sorted(len(s) for s in G.subs)[-7:] == list(ls.GIANTS)
    assert len(G.subs) == 7 + ls.N_FILLERS and max(len(s) for s in G.subs if len(s) not in ls.GIANTS) <= 3000
    assert min(len(s) for s in G.subs) == 2
    # shuffled: the giants are not in a row, nor sorted
    at = [G.giant[L] for L in ls.GIANTS]
    assert at != sorted(at) and max(at) - min(at) > 7
    for L in ls.ALL_CODES:
        assert len(np.unique(G.subs[G.giant[L]])) == 25
    ids = G.ids_custom
    assert len(set(ids.tolist())) == len(ids) and all(i % 3 == 1 for i in ids) and list(ids) != sorted(ids)
    kinds = {(p, k) for L in ls.GIANTS for p, k, _, _ in G.plan[L]["cross"]}
    assert {(P15, "ins"), (P15, "del"), (P16, "ins")} <= kinds
    for L in ls.GIANTS:
        for p, kind, c0, c1 in G.plan[L]["cross"]:
            assert c0 < p - 2 and p + 2 < c1 and G.plan[L]["start"][1] < c0 and c1 + 300 < G.plan[L]["end"][0]
        assert G.plan[L]["end900"][1] == L - ls.END_PAD and G.plan[L]["end"][1] == L - ls.END_PAD - ss.TAIL


@pytest.mark.parametrize("scoring", ls.SCORINGS, ids=["b62-11-1", "b50-2-2"])
def test_giants_depend_on_their_last_columns(oracle, G, scoring):
    mid, go, ge = scoring
    m = mat_of(oracle, mid)
    whole = ls.scan(oracle, "q568-G", G.q, G, m, go, ge)
    seen = {c: 0 for c in ls.CUTS}
    for L in ls.GIANTS:
        s = G.subs[G.giant[L]]
        e0, e1 = G.plan[L]["end"]
        best = int(whole[G.giant[L]])
        assert best == oracle.score(G.q, s[e0:e1], m, go, ge), L
        # the start and cross pieces score less
        assert oracle.score(G.q, s[:e0 - 100], m, go, ge) < best, L
        for cut in ls.CUTS:
            if cut < e1:
                assert oracle.score(G.q, s[:cut], m, go, ge) < best, (L, cut)
                seen[cut] += 1
            elif cut < L:
                assert oracle.score(G.q, s[:cut], m, go, ge) == best, (L, cut)
        for P in (P15, P16):
            if L > P:
                assert oracle.score(G.q, s[:L % P], m, go, ge) < best, (L, P, "count mod")
                if e1 > P + 100:
                    wrapped = np.concatenate([s[:P], s[:L - P]])
                    assert oracle.score(G.q, wrapped, m, go, ge) < best, (L, P, "index mod")
        al = oracle.align(G.q600, s, m, go, ge)
        # (the 600-row query ends with the 568: the same piece is its best)
        if L > P15:
            assert al["s_begin"] > P15, (L, al["s_begin"])
        if L >= P16:
            assert al["s_begin"] > 64500, (L, al["s_begin"])
        if L == 70001:
            assert al["s_begin"] > P16
        assert al["s_end"] == e1 and al["q_end"] == 600, (L, al["s_end"], al["q_end"])
    assert seen == {P15 - 1: 5, P15: 5, P16 - 1: 1, P16: 1}, seen


@pytest.mark.parametrize("scoring", ls.SCORINGS, ids=["b62-11-1", "b50-2-2"])
def test_cross_pieces_hold_their_run_on_the_power(oracle, G, scoring):
    mid, go, ge = scoring
    m = mat_of(oracle, mid)
    n = 0
    for L in ls.GIANTS:
        s = G.subs[G.giant[L]]
        for p, kind, c0, c1 in G.plan[L]["cross"]:
            w0 = c0 - 50
            al = oracle.align(G.q[ls.CROSS_ROWS[0]:ls.CROSS_ROWS[1]], s[w0:c1 + 50], m, go, ge)
            ops, j = al["ops"], w0 + al["s_begin"] - 1  # 0-based column of the first op
            runs, k = [], 0
            while k < len(ops):
                e = k
                while e < len(ops) and ops[e] == ops[k]:
                    e += 1
                if ops[k] != "M":
                    runs.append((ops[k], j, e - k))
                j += (e - k) if ops[k] != "I" else 0
                k = e
            assert len(runs) == 1, (L, p, kind, runs)
            op, col, length = runs[0]
            assert length == ls.CROSS_L
            if kind == "ins":   # columns against gaps: P - 2 .. P + 2
                assert (op, col) == ("D", p - 2), (L, p, runs)
            else:               # rows against gaps, between columns P - 1 and P
                assert (op, col) == ("I", p), (L, p, runs)
            assert al["s_begin"] + w0 <= c0 + 5 and al["s_end"] + w0 >= c1 - 5
            n += 1
    assert n >= 6


@pytest.mark.parametrize("n", ls.QLONG)
@pytest.mark.parametrize("scoring", ls.SCORINGS, ids=["b62-11-1", "b50-2-2"])
def test_long_queries_depend_on_their_far_rows(oracle, scoring, n):
    mid, go, ge = scoring
    m = mat_of(oracle, mid)
    q, d = ls.long_query(n), ls.S(n)
    assert len(d.subs) == ls.N_S and d.offs[-1] <= ls.S_RESIDUES
    whole = ls.scan(oracle, "q%d-S" % n, q, d, m, go, ge)
    planted = [k for k, x in enumerate(d.meta) if x]
    assert len(planted) == ls.N_S // 2
    for name, (power, lo, hi) in ls.regions(n).items():
        mine = [k for k in planted if d.meta[k][0] == name]
        assert len(mine) >= 15, (name, len(mine))
        past = 0
        cut_at = (power - 1) if power else (n - 600)
        cut = oracle.scan(q[:cut_at], d.res, d.offs, mat=m, gap_open=go, gap_extend=ge, nthreads=16)
        for k in mine:
            r0, rows = d.meta[k][1], d.meta[k][2]
            # (aligned inside a window of the query: the score is the whole query's)
            w0 = max(0, r0 - 400)
            al = oracle.align(q[w0:r0 + rows + 400], d.subs[k], m, go, ge)
            al["q_begin"] += w0
            al["q_end"] += w0
            assert al["q_begin"] > r0 - 3 and al["q_end"] <= r0 + rows + 3 and al["score"] == whole[k], (name, k)
            assert al["q_end"] - al["q_begin"] > rows - 30
            assert al["q_end"] > cut_at and cut[k] < whole[k], (name, k, al, int(cut[k]))
            past += power is not None and al["q_begin"] > power
        if power and hi - power >= 400:
            assert past >= 10, (name, past)
    if n > P16:
        wrapped = np.concatenate([q[:P16], q[:n - P16]])  # rows read mod 2^16
        w = oracle.scan(wrapped, d.res, d.offs, mat=m, gap_open=go, gap_extend=ge, nthreads=16)
        for k in planted:
            if d.meta[k][1] + d.meta[k][2] > P16 + 20:
                assert w[k] < whole[k], k


def test_square_scores_leave_16_bits(oracle):
    t = ls.square()
    assert len(t.subs) == 2 + ls.T_FILLERS and len(t.q) == ls.T_QLEN
    m = mat_of(oracle, 1)
    want = ls.scan(oracle, "qT-T", t.q, t, m, 11, 1)
    top = sorted(want.tolist())[-2:]
    assert top[0] > 65504 and top[1] > 170000 and top[1] == want[t.self_at] and top[0] == want[t.copy_at], top
    assert sorted(want.tolist())[-3] < 200
    u = ls.square_short()
    short = ls.scan(oracle, "qTs-Ts", u.q, u, m, 11, 1)
    assert short[u.self_at] > 65504 and short[u.copy_at] > 32767 and sorted(short.tolist())[-3] < 200


@pytest.mark.parametrize("scoring", ls.RESCUE_SCORINGS, ids=["b62x9-108-9", "b50x6-12-12"])
def test_giants_pass_the_guards_when_scaled(oracle, G, scoring):
    mid, k, go, ge = scoring
    m = mat_of(oracle, mid, k)
    at = [G.giant[L] for L in ls.GIANTS]
    want = ls.scan(oracle, "q568-G", G.q, G, m, go, ge)
    assert np.array_equal(want, k * ls.scan(oracle, "q568-G", G.q, G, mat_of(oracle, mid), go // k, ge // k))
    # past every fp16 limit (the highest: 4096 - 28 ge - 2 max S), below the int16 forms' lowest
    assert want[at].min() >= 4096 and want[at].max() < ls.K_SAT16 - 38 * ge
    # with the 900-row query the giants pass the int16 guard too
    want9 = ls.scan(oracle, "q900-G", G.q900, G, m, go, ge)
    assert want9[at].min() >= ls.K_SAT16


def test_direction_arrays_pass_the_budgets():
    assert ls.align_dirs_bytes(32760, 1) < 1 << 30 < ls.align_dirs_bytes(32776, 1)
    assert ls.align_dirs_bytes(32776, 300) == (32776 + 300 + 1) * 32777 > 1 << 30
    assert ls.align_dirs_bytes(65544, 300) == 65845 * 65545 > 1 << 32
