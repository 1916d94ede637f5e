"""What tests/test_gpu_history.py will run, checked without a device: the
generated histories (tests/history_support.py generate) cover every ordered
pair of op kinds, of databases, of scorings on one database, and put the long
queries behind shorter and longer ones; and the world's fixtures are what the
histories rely on, by the oracle's scores."""
import numpy as np
import pytest

import history_support as hs


@pytest.fixture(scope="module")
def histories():
    return hs.generate()


@pytest.fixture(scope="module")
def world(oracle):
    return hs.World(oracle)


def test_shape(histories):
    assert len(histories) == hs.N_HISTORIES and [len(h) for h in histories] == [37] * 4
    assert hs.generate() == histories  # a function of the seed alone
    for a, b in zip(histories, histories[1:]):
        assert a[-1] == b[0]  # the cut's op is shared, so no transition is lost
    for o in (o for h in histories for o in h):
        assert o.kind in hs.KINDS
        assert o.db in hs.DBS or o.kind == "set_opts"
        if o.kind == "set_threshold":
            assert o.db in ("A", "C") and o.arg in hs.THRESHOLDS
        if o.kind == "scan_batch":
            assert 2 <= len(o.q) <= 9
        elif o.kind in hs.SCORED:
            assert o.q != hs.EMPTY  # the empty query in batches only
        if o.kind == "pssm":
            assert o.q in hs.PSSM_Q and o.sc == "b62-11-1"  # the table is BLOSUM62's


def test_every_ordered_pair_of_kinds(histories):
    seen = set().union(*(hs.transitions(h, lambda o: o.kind) for h in histories))
    assert seen == {(a, b) for a in hs.KINDS for b in hs.KINDS}  # 144, self-loops included


def test_every_database_follows_every_other(histories):
    seen = set().union(*(hs.transitions(h, lambda o: o.db) for h in histories))
    assert {(a, b) for a in hs.DBS for b in hs.DBS if a != b} <= seen


def test_every_scoring_follows_every_other_on_one_database(histories):
    """... within one history: both scans see the same sw_db."""
    for db in hs.DBS:
        seen = set()
        for h in histories:
            seen |= hs.transitions(h, lambda o: o.sc if o.kind in hs.SCORED and o.db == db else None)
        missing = {(a, b) for a in hs.SCORINGS for b in hs.SCORINGS if a != b} - seen
        assert not missing, (db, missing)


def test_long_queries_after_shorter_and_longer(histories):
    """The staircases are per database and scoring: the 900 query comes after
    a shorter and after a longer query under the same scoring on the same
    database earlier in its history, the 1,300 query (no query is longer)
    after a shorter one."""
    def lengths(o):
        return [hs.QLENS[q] for q in (o.q if o.kind == "scan_batch" else (o.q,)) if q != hs.EMPTY]
    after = {900: set(), 1300: set()}
    for h in histories:
        earlier = {}
        for o in h:
            if o.kind not in hs.SCORED:
                continue
            for n in lengths(o):
                if n in after:
                    seen = earlier.get((o.db, o.sc), [])
                    after[n] |= {"shorter" for m in seen if m < n} | {"longer" for m in seen if m > n}
                earlier.setdefault((o.db, o.sc), []).append(n)
    assert after[900] == {"shorter", "longer"} and after[1300] == {"shorter"}


def test_batches_hold_the_empty_query_everywhere(histories):
    places = set()
    for o in (o for h in histories for o in h if o.kind == "scan_batch"):
        places |= {"start" for _ in [0] if o.q[0] == hs.EMPTY} | {"end" for _ in [0] if o.q[-1] == hs.EMPTY}
        places |= {"middle" for q in o.q[1:-1] if q == hs.EMPTY}
        if len(set(o.q)) < len(o.q):
            places.add("repeat")
    assert places == {"start", "middle", "end", "repeat"}


def test_every_choice_is_drawn(histories):
    ops = [o for h in histories for o in h]
    assert {o.arg for o in ops if o.kind == "set_opts"} == set(hs.PROFILES)
    assert {o.arg for o in ops if o.kind == "set_threshold"} == set(hs.THRESHOLDS)
    assert {o.arg[0] for o in ops if o.kind == "fail"} == {"gap0", "entry101", "align_id", "topk0"}
    assert {o.arg for o in ops if o.kind == "topk"} >= {("host", 4096), ("rank", 1)}
    assert {o.arg[0] for o in ops if o.kind == "topk"} == {"host", "rank"}
    assert {o.arg[1] for o in ops if o.kind == "topk"} == set(hs.TOPK)
    assert {o.arg for o in ops if o.kind == "hits"} == {"scan_hits", "hit_stats"}
    assert {o.arg[0] for o in ops if o.kind == "pssm"} == {"scan", "topk"}
    for kind in ("reopen", "reset_adaptive"):
        assert {o.db for o in ops if o.kind == kind} == set(hs.DBS), kind


def test_euler_circuit():
    for seed in range(5):
        c = hs.euler_circuit(12, np.random.default_rng(seed))
        assert len(set(zip(c, c[1:]))) == 144


def test_world_fixtures(world, oracle):
    """The databases are what the histories rely on: A has subjects on both
    sides of its long threshold and B none above any default; the planted
    copies score past the fp16 guard under the first three scorings (4096 - 28
    ge - 2 max S), past the int16 one (32767 - 1152) under the matrix times
    6, in both parts of A; everything else stays below the fp16 guard under
    BLOSUM62 11/1 and its sixfold, so the rescue lists hold the copies only."""
    a = [len(s) for s in world.subs["A"]]
    assert len(a) == 512 and min(a) == 1 and sum(n > hs.A_THRESHOLD for n in a) == 14
    assert max(n for n in a if n <= hs.A_THRESHOLD) == 1500
    assert len(world.subs["B"]) == 130 and max(len(s) for s in world.subs["B"]) <= 400
    assert world.n_out["B"] > 130 and len(set(world.ids["B"].tolist())) == 130
    for sc in hs.SCORINGS[:3]:
        m, go, ge = world.scoring(sc)
        guard = 4096 - 28 * ge - 2 * int(m.max())
        for qi in (4, 5):
            want = world.want("A", qi, sc)
            over = np.nonzero(want >= guard)[0]
            assert sum(a[i] <= hs.A_THRESHOLD for i in over) >= 1 and sum(a[i] > hs.A_THRESHOLD for i in over) >= 1
            if sc != "b50-lin-2":
                assert len(over) == 2, (sc, qi, want[over])
            if sc == "b62x6-66-6":
                assert (want[over] > 32767 - 1152 + 66).all(), want[over]
    # the sixfold scoring is the same alignments: six times BLOSUM62 11/1's scores
    assert np.array_equal(world.want("A", 3, "b62x6-66-6"), 6 * world.want("A", 3, "b62-11-1"))
    assert world.pssm_rows[3].shape == (375, 25) and world.pssm_rows[4].shape == (900, 25)
