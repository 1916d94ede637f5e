"""GPU: scan histories (tests/history_support.py): one handle, the resident
databases A, B and C, and mixed calls in an order that matters.  Every
result of every op is compared with the oracle bit for bit (scores), with the
top-K of the oracle's scores, with hits_support.expected (hit rows) and with
oracle.align and path_score (alignments).

The 4 generated histories run synced (each op checked as it completes, the
whole history twice on fresh handles: the same routes both times, since every
readback has completed when the next scan looks) and queued (device entry
points only, buffers of their own, one synchronise at the end).  The named
histories each aim at one piece of state that outlives a scan: the 32 drain
blobs, the 8 work tables, sw_opts under warm caches, the 4 profile slots, the
score buffer sw_scan_topk shares with its keys, the two int16-first
staircases, the first-use tables across a rebuild, a failed call, two
handles.  The adaptive routes are on except where a history says it forces
them.

20 cases, 14 s in all (the slowest 2.4 s, the fixture's oracle work 3.8 s);
the oracle's work for the whole module (memoised, 16 threads) is 2.3 to 5 s
by the host, most of it in the `world` fixture."""
import re

import numpy as np
import pytest

import history_support as hs

pytestmark = pytest.mark.gpu

# the rescue: line of sw_opts rescue_stats (as tests/test_gpu_scoring_envelope.py reads it)
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; "
                    r"pairs \d+; intra (-?\d+)/\d+ flagged, (-?\d+) again")
FIXED = dict(inter_i16_span=0, intra_i16_first=0)  # the adaptive routes off: a named history that pins route names
HISTORIES = hs.generate()


@pytest.fixture(scope="module")
def world(sw, oracle, handle):
    w = hs.World(oracle)
    c = sw.Database.synthetic(handle, hs.C_SEED, hs.C_N)
    w.set_c(hs.c_subjects(sw, *c.subjects()))
    c.close()
    for h in HISTORIES:
        w.prepare(h)
    return w


@pytest.fixture
def runner(sw, world):
    """A fresh handle with A, B and C on it."""
    r = hs.Runner(sw, world)
    yield r
    r.close()


def flagged(capfd):
    m = RESCUE.findall(capfd.readouterr().err)
    assert m, "no rescue: line"
    return dict(zip(("inter", "inter_again", "intra", "intra_again"), map(int, m[-1])))


def test_fixture_conditions(world, runner, capfd):
    """What the histories on A rely on: the 900 and the 1,300 query under the
    first three scorings take the merged launch with its drain (profile lpt 1,
    pair_width 64), and the drain has something to drain: at least one inter
    block and one long subject flagged, under the matrix times 6 at least one
    of each flagged again by the int16 stage.  (A stale drain blob is
    invisible to a scan that drains nothing.)"""
    runner.profile("lpt64", rescue_stats=1)
    db = runner.dbs["A"]
    assert db.stats()["n_long"] == 14 and db.stats()["n_blocks"] == 8
    assert runner.dbs["B"].stats()["n_long"] == 0
    for qi in (4, 5):
        for sc in hs.SCORINGS[:3]:
            db.reset_adaptive()
            capfd.readouterr()
            got = db.scan(world.query(qi), *world.scoring(sc))
            f = flagged(capfd)
            k = runner.h.last_kernel()
            with capfd.disabled():
                print("HISTORY fixture | q %d %s | %s | %s | %s" % (hs.QLENS[qi], sc, k, runner.h.last_intra_kernel(), f))
            runner.check_scores(got, "A", qi, sc, "fixture")
            assert "+lpt" in k and "+drain" in k, k
            assert f["inter"] >= 1 and f["intra"] >= 1, (qi, sc, f)
            if sc == "b62x6-66-6":
                assert f["inter_again"] >= 1 and f["intra_again"] >= 1, (qi, sc, f)


# ---- the generated histories ---------------------------------------------------
@pytest.mark.parametrize("n", range(hs.N_HISTORIES))
def test_generated_synced(sw, world, n):
    """Each op checked against the oracle as it completes; the history again
    on a fresh handle with fresh databases takes the same routes (a route that
    depends on anything but the history's observations is a finding)."""
    routes = []
    for _ in range(2):
        r = hs.Runner(sw, world)
        try:
            routes.append(r.run_synced(HISTORIES[n], "history %d" % n))
        finally:
            r.close()
    diff = [(k, HISTORIES[n][k], a, b) for k, (a, b) in enumerate(zip(*routes)) if a != b]
    assert not diff, diff[:3]


@pytest.mark.parametrize("n", range(hs.N_HISTORIES))
def test_generated_queued(runner, n):
    """The device entry points alone, no host wait between the ops: the
    adaptive routes see whichever readbacks happen to have landed, so no route
    names here, and every buffer equals the oracle."""
    runner.run_queued(HISTORIES[n], "history %d" % n)


# ---- named histories -------------------------------------------------------------
def drain_uploads(keys, slots=32):
    """drain_blob's cache by its construction: a miss takes the next slot in
    turn.  Returns the scans that upload."""
    held, nxt, misses = [None] * slots, 0, []
    for t, k in enumerate(keys):
        if k not in held:
            held[nxt] = k
            nxt = (nxt + 1) % slots
            misses.append(t)
    return misses


def test_drain_slots(world, runner):
    """More drain blobs than the 32 slots.  The key holds the profile slot
    (a ring of 4) and the list parity (which alternates with it), the score
    buffer, the query length and the scoring: 9 shapes in a ring visit 36
    keys in 36 scans (9 and 4 are coprime), 36 uploads; the 9 scans after
    them find their blobs evicted (uploads 33 to 36 took slots 0 to 3, then
    every further miss the next) and upload again, 45 in all.  The same ring
    by sw_scan_device into two alternating buffers is 36 more keys (the
    buffer's address), 90 uploads; then the host scans' blobs are gone again,
    99.  A slot that
    grew under a later query adds uploads, never removes one.  Every scan
    drains (the copies of the 900 and 1,300 query) and equals the oracle."""
    import torch
    shapes = [(qi, sc) for sc in hs.SCORINGS[:3] for qi in (4, 5)] + [(4, "asym-3-5"), (5, "asym-3-5"), (3, "b62-11-1")]
    assert len(shapes) == 9
    runner.profile("lpt64", **FIXED)
    db = runner.dbs["A"]
    ring = [shapes[t % 9] for t in range(45)]
    keys = [(s, t % 4, "host") for t, s in enumerate(ring)]
    assert drain_uploads(keys) == list(range(45))
    for t, (qi, sc) in enumerate(ring):
        runner.check_scores(db.scan(world.query(qi), *world.scoring(sc)), "A", qi, sc, ("drain host", t))
        assert runner.h.last_kernel().endswith("+lpt+drain"), (t, runner.h.last_kernel())
    bufs = [torch.full((db.n_out,), hs.FILL, dtype=torch.int32, device="cuda") for _ in range(2)]
    dkeys = keys + [(s, (45 + t) % 4, t % 2) for t, s in enumerate(ring)]
    assert len(drain_uploads(dkeys)) == 90
    for t, (qi, sc) in enumerate(ring):
        b = bufs[t % 2]
        b.fill_(hs.FILL)
        torch.cuda.synchronize()
        db.scan_device(world.query(qi), b.data_ptr(), *world.scoring(sc))
        torch.cuda.synchronize()
        runner.check_buffer(b.cpu().numpy(), "A", qi, sc, ("drain device", t))
        assert runner.h.last_kernel().endswith("+lpt+drain"), (t, runner.h.last_kernel())
    assert len(drain_uploads(dkeys + [(s, (90 + t) % 4, "host") for t, s in enumerate(ring[:9])])) == 99
    for t, (qi, sc) in enumerate(ring[:9]):
        runner.check_scores(db.scan(world.query(qi), *world.scoring(sc)), "A", qi, sc, ("drain host again", t))
        assert runner.h.last_kernel().endswith("+lpt+drain"), (t, runner.h.last_kernel())


def block_widths(lengths, thr):
    """Widths of the inter blocks: the subjects up to the threshold, longest
    first, 64 to a block, in groups of 16 columns."""
    short = sorted((n for n in lengths if n <= thr), reverse=True)
    return [-(-max(short[i:i + 64]) // 16) * 16 for i in range(0, len(short), 64)]


def merged_suffix(widths, thr, qlen, affine, opts):
    """The merged launch's suffixes by scan_plan's rules (csrc/sw_plan.cpp,
    pinned on the CPU by tests/native/plan_check.cpp): from two 64-row passes
    on, wave pairs for the blocks at least pair_width wide; 96-row passes under linear gaps from 97
    query rows on; tris under affine gaps for the pair blocks at least
    tri_width (default 0.48 x the long threshold) wide where 3-wave rounds are
    as few as 4-wave ones; tail pairs for the narrowest tail_pairs single-wave
    blocks but one (default: none on so few blocks)."""
    def up(n, m):
        return -(-n // m) * m

    def leading(w):
        n = 0
        while n < npair and widths[n] >= w:
            n += 1
        return n
    if up(qlen, 64) <= 64:
        return ""  # one pass of the two strips: no wave pairs, so no merged launch
    npair = sum(w >= opts.get("pair_width", 64) for w in widths)
    rows = 96 if not affine and up(qlen, 96) > 96 else 64
    passes = up(qlen, rows) // rows
    tri_w = opts.get("tri_width", int(0.48 * thr))
    ntri = leading(tri_w) if affine and tri_w > 0 and passes > 0 and (passes + 2) // 3 <= (passes + 3) // 4 else 0
    singles = len(widths) - npair
    ntail = min(opts.get("tail_pairs", 0), singles - 1) if passes >= 2 and singles >= 2 else 0
    return ("+tail%d" % ntail if ntail else "") + ("+tri%d" % ntri if ntri else "") + "+lpt+drain"


def test_work_tables(world, runner):
    """More merged shapes than the 8 cached work tables: five query lengths,
    both gap models, quads against tris against neither, tail pairs, and
    lpt_pipe / lpt_pipe_tail changed under the same plan; then the first
    shapes again (dropped since, built again).  Each scan's name carries the
    suffixes scan_plan's rules give that shape, and its scores equal the
    oracle's under a table that was built for exactly it."""
    variants = [("lpt64", {}), ("quad16", dict(tri_width=0)), ("tri16", {}), ("lpt64", dict(lpt_pipe=2)),
                ("lpt64", dict(lpt_pipe_tail=3)), ("lpt64", dict(pair_width=256, tail_pairs=2)), ("lpt64", {})]
    widths = block_widths([len(s) for s in world.subs["A"]], hs.A_THRESHOLD)
    assert len(widths) == 8 and sum(w < 256 for w in widths) >= 3
    db = runner.dbs["A"]
    wrong, seen = [], set()
    for name, more in variants:
        opts = dict(hs.PROFILES[name], **more)
        runner.profile(name, **dict(more, **FIXED))
        for qi in (1, 2, 3, 4, 5):
            for sc in ("b62-11-1", "b50-lin-2"):
                runner.check_scores(db.scan(world.query(qi), *world.scoring(sc)), "A", qi, sc, ("tables", name, more))
                k = runner.h.last_kernel()
                want = merged_suffix(widths, hs.A_THRESHOLD, hs.QLENS[qi], sc == "b62-11-1", opts)
                seen.add((qi, sc, want, more.get("lpt_pipe"), more.get("lpt_pipe_tail")))
                if k[k.index(">") + 1:] != want:
                    wrong.append((name, more, hs.QLENS[qi], sc, k, want))
    for x in wrong:
        print("HISTORY tables wrong:", x)
    assert not wrong, wrong
    assert len(seen) > 16  # (two rounds of the 8 tables, by name and option alone)
    assert any("+tri" in s[2] for s in seen) and any("+tail" in s[2] for s in seen)


def test_opts_under_a_warm_cache(world, runner):
    """The same query and scoring on A under each sw_opts profile in turn and
    back again, twice round: the table and the blob cached under one profile
    must not serve another.  The routes are pinned (the adaptive ones off):
    each profile takes the same route at every visit, and the merged profiles'
    names differ as their options do."""
    db, qi, sc = runner.dbs["A"], 4, "b62x6-66-6"
    order = list(hs.PROFILES) + list(hs.PROFILES)[::-1]
    routes = {}
    for visit, name in enumerate(order * 2):
        runner.profile(name, **FIXED)
        runner.check_scores(db.scan(world.query(qi), *world.scoring(sc)), "A", qi, sc, ("warm", visit, name))
        assert routes.setdefault(name, runner.route()) == runner.route(), (visit, name)
    assert "+lpt" in routes["lpt64"][0] and "+lpt" not in routes["nolpt"][0]
    assert routes["int32"][0].startswith("sw_inter<") and routes["int32"][1].startswith("sw_intra<")
    # (a 900-residue query is 14 affine passes: no tris; 375 is 6)
    runner.profile("tri16", **FIXED)
    runner.check_scores(db.scan(world.query(3), *world.scoring(sc)), "A", 3, sc, "warm tri")
    tri = runner.h.last_kernel()
    runner.profile("quad16", tri_width=0, **FIXED)
    runner.check_scores(db.scan(world.query(3), *world.scoring(sc)), "A", 3, sc, "warm quad")
    assert "+tri" in tri and "+tri" not in runner.h.last_kernel()


def test_profile_slots(world, runner):
    """Batches through the ring of 4 profile slots under the matrix times 6
    (every stage of both rescue chains runs, so the deferred tails read their
    slots late): 9 queries in ascending length, so that every reuse of a slot
    grows it while the tail of four scans earlier may still read it; the same
    descending; a batch on A, at once one on B, then A again.  Each batch
    equals the oracle row by row and the per-query scans."""
    sc = "b62x6-66-6"
    asc = (0, 1, 2, 3, 3, 4, 4, 5, 5)
    for db, qs in (("A", asc), ("A", asc[::-1]), ("A", (5, 2, 4)), ("B", (4, 5, 1, 3)), ("A", (5, 2, 4))):
        runner.run(hs.op("scan_batch", db, qs, sc), "slots")
    for db in ("A", "B"):
        got = runner.dbs[db].scan_batch([world.query(q) for q in asc], *world.scoring(sc))
        for row, qi in zip(got, asc):
            assert np.array_equal(row, runner.dbs[db].scan(world.query(qi), *world.scoring(sc))), (db, qi)


def test_score_buffer(world, runner):
    """The handle's score buffer: sw_scan_topk keeps its k keys behind the
    n_out scores in it.  k = 4096 on B (the keys far past B's 130 subjects),
    a scan of C (which grows the buffer), the same ranking on B, a batch on
    A (which grows it again), a scan of B."""
    sc = "b62-11-1"
    for o in (hs.op("topk", "B", 3, sc, ("host", 4096)), hs.op("scan", "C", 4, sc),
              hs.op("topk", "B", 3, sc, ("host", 4096)), hs.op("scan_batch", "A", (2, 5, hs.EMPTY, 4, 3, 3), sc),
              hs.op("scan", "B", 4, sc), hs.op("topk", "C", 2, sc, ("host", 4096)), hs.op("topk", "B", 5, sc, ("host", 1))):
        runner.run(o, "score buffer")


def stair_world(sw, oracle, world):
    """128 subjects of 600..700 residues (two inter blocks) and 64 of 60..120;
    under the asymmetric matrix (mean entry +2) random pairs score with their
    lengths: by the oracle a 500-residue query stays below the fp16 guard on
    every subject, 700 and 800 residues pass it in both wide blocks (the
    smallest database found on which the observation triggers: at least one
    lane of every wide block, most of the blocks up to the last flagged)."""
    rng = np.random.default_rng(5)
    wide = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(600, 701, size=128)]
    narrow = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(60, 121, size=64)]
    q = rng.integers(0, 25, size=800).astype(np.uint8)
    m = world.mats["asym-3-5"]
    scorings = {"X": (m, 3, 5), "Y": (m, 4, 4)}
    return wide, narrow, q, scorings


def stair_want(oracle, subs, q, scoring):
    m, go, ge = scoring
    res, offs = hs.pack(subs)
    return oracle.scan(q, res, offs, mat=m, gap_open=go, gap_extend=ge, nthreads=16)


def test_staircase_inter(sw, oracle, world, runner):
    """adapt_inter_i16_span's staircase, per scoring: +int16[0,n) appears only
    for a query at least as long as an observation under the same scoring; a
    shorter, later observation lowers the length from which it applies; a PSSM
    of the same length shares none of it; sw_db_reset_adaptive forgets it, and
    so does sw_db_set_long_threshold there and back."""
    wide, narrow, q, scorings = stair_world(sw, oracle, world)
    subs = wide + narrow
    res, offs = hs.pack(subs)
    h = runner.h
    h.reset_opts()
    db = sw.Database(h, res, offs, long_threshold=4096)
    assert db.stats()["n_long"] == 0 and db.stats()["n_blocks"] == 3
    order = np.argsort([-len(s) for s in subs], kind="stable")
    want = {}
    for name, s in scorings.items():
        limit = 4096 - 28 * s[2] - 2 * int(s[0].max())
        for n in (500, 700, 800):
            w = want[name, n] = stair_want(oracle, subs, q[:n], s)
            per_block = [int(w[order[b * 64:(b + 1) * 64]].max()) for b in range(3)]
            if n == 500:
                assert max(per_block) < limit - 100, (name, n, per_block)
            else:
                assert min(per_block[:2]) >= limit + 50 and per_block[2] < limit - 100, (name, n, per_block)
    pssm = sw.Pssm(h, scorings["X"][0][q.astype(np.int64)])

    def scan(name, n):
        got = db.scan(q[:n], *scorings[name])
        assert np.array_equal(got, want[name, n]), (name, n, h.last_kernel())
        return "+int16[0,2)" in h.last_kernel()

    steps = []
    steps.append(("first X 800: nothing observed", scan("X", 800), False))
    # (the same query straight after: readback_record's "same as the last
    # observation" skip must tell the scorings apart, or Y is never observed)
    steps.append(("Y 800: another scoring", scan("Y", 800), False))
    steps.append(("X 800 after its observation", scan("X", 800), True))
    steps.append(("Y 800 after its own observation", scan("Y", 800), True))
    steps.append(("X 700: shorter than the observation", scan("X", 700), False))
    steps.append(("X 700: its own observation lowers the step", scan("X", 700), True))
    steps.append(("X 500: shorter than any observation", scan("X", 500), False))
    steps.append(("X 800 still", scan("X", 800), True))
    steps.append(("Y 700: Y's step is at 800", scan("Y", 700), False))
    assert np.array_equal(db.scan_pssm(pssm, 3, 5), want["X", 800])
    steps.append(("PSSM of the 800 query under X's gaps", "+int16" in h.last_kernel(), False))
    steps.append(("X 700 after the PSSM", scan("X", 700), True))
    db.reset_adaptive()
    steps.append(("X 800 after reset_adaptive", scan("X", 800), False))
    steps.append(("X 800 observed again", scan("X", 800), True))
    db.set_long_threshold(5000)
    db.set_long_threshold(4096)
    steps.append(("X 800 after a rebuild there and back", scan("X", 800), False))
    steps.append(("Y 800 after a rebuild there and back", scan("Y", 800), False))
    pssm.close()
    db.close()
    assert [s for s in steps if s[1] != s[2]] == [], steps


def test_staircase_intra(sw, oracle, world, runner):
    """adapt_intra_i16_first the same way (the data of
    test_intra_rescue_chain_fp16_int16_int32 reduced to 12 long subjects of
    600..700 residues): the int16 form runs first only once a scan under the
    same scoring flagged over a third of the long subjects at a query no
    longer than this one."""
    wide, _, q, scorings = stair_world(sw, oracle, world)
    subs = wide[:12]
    res, offs = hs.pack(subs)
    h = runner.h
    h.reset_opts()
    db = sw.Database(h, res, offs, long_threshold=64)
    assert db.stats()["n_long"] == 12 and db.stats()["n_blocks"] == 0
    want = {}
    for name, s in scorings.items():
        # the wavefront cell's guard, at 20 rows per lane and at fewer
        lo, hi = (4096 - (b + 2) * s[2] - 2 * int(s[0].max()) for b in (38, 26))
        for n in (500, 700, 800):
            w = want[name, n] = stair_want(oracle, subs, q[:n], s)
            assert (w.max() < lo - 100) if n == 500 else (3 * int((w >= hi + 50).sum()) > 12), (name, n, w)
    pssm = sw.Pssm(h, scorings["X"][0][q.astype(np.int64)])

    def scan(name, n):
        got = db.scan(q[:n], *scorings[name])
        assert np.array_equal(got, want[name, n]), (name, n, h.last_intra_kernel())
        return h.last_intra_kernel().endswith(",int16>")

    steps = []
    steps.append(("first X 800: nothing observed", scan("X", 800), False))
    # (the same query straight after: readback_record's "same as the last
    # observation" skip must tell the scorings apart, or Y is never observed)
    steps.append(("Y 800: another scoring", scan("Y", 800), False))
    steps.append(("X 800 after its observation", scan("X", 800), True))
    steps.append(("Y 800 after its own observation", scan("Y", 800), True))
    steps.append(("X 700: shorter than the observation", scan("X", 700), False))
    steps.append(("X 700: its own observation lowers the step", scan("X", 700), True))
    steps.append(("X 500: shorter than any observation", scan("X", 500), False))
    steps.append(("X 800 still", scan("X", 800), True))
    steps.append(("Y 700: Y's step is at 800", scan("Y", 700), False))
    assert np.array_equal(db.scan_pssm(pssm, 3, 5), want["X", 800])
    steps.append(("PSSM of the 800 query under X's gaps", h.last_intra_kernel().endswith(",int16>"), False))
    steps.append(("X 700 after the PSSM", scan("X", 700), True))
    db.reset_adaptive()
    steps.append(("X 800 after reset_adaptive", scan("X", 800), False))
    steps.append(("X 800 observed again", scan("X", 800), True))
    db.set_long_threshold(100)
    db.set_long_threshold(64)
    steps.append(("X 800 after a rebuild there and back", scan("X", 800), False))
    pssm.close()
    db.close()
    assert [s for s in steps if s[1] != s[2]] == [], steps


def test_first_use_tables_across_a_rebuild(world, runner):
    """id_index (sw_align) and pos_of (sw_hit_stats) are built on first use
    and survive sw_db_set_long_threshold, d_ids (sw_scan_topk) belongs to the
    layout and does not: the same rows, alignments and keys before the
    rebuild, with most subjects moved to the other layout (A: 1500 to 64; C,
    whose default threshold makes nearly all of its 2,000 subjects long: to
    1500), and back; on A and on C."""
    for db, home, there in (("A", hs.A_THRESHOLD, 64), ("C", 0, 1500)):
        calls = [hs.op("hits", db, 3, "b62-11-1", "hit_stats"), hs.op("align", db, 3, "b62-11-1"),
                 hs.op("topk", db, 3, "b62-11-1", ("host", 100)), hs.op("hits", db, 5, "b50-lin-2", "scan_hits")]
        for o in calls[:2]:
            runner.run(o, "first use")
        n_long = runner.dbs[db].stats()["n_long"]
        runner.dbs[db].set_long_threshold(there)
        assert abs(runner.dbs[db].stats()["n_long"] - n_long) > 400  # most subjects change layout
        for o in calls:
            runner.run(o, "there")
        runner.dbs[db].set_long_threshold(home)
        assert runner.dbs[db].stats()["n_long"] == n_long
        for o in calls:
            runner.run(o, "back")


FAILURES = [("gap0", e) for e in hs.FAIL_ENTRIES] + [("entry101", e) for e in hs.FAIL_ENTRIES] + \
    [("align_id", None), ("topk0", None)]


def test_after_a_failure(world, runner):
    """A call that fails leaves everything as it was: after each failing call
    (a gap of 0 and an entry of 101 at each scan entry point, sw_align with an
    id not in the database, sw_scan_topk with k = 0) the successful op before
    it, repeated, gives the same result by the same route (the adaptive routes
    off: a repeat would otherwise differ by its own observation)."""
    runner.profile("lpt64", **FIXED)
    for db, qi, sc in (("A", 5, "b62x6-66-6"), ("B", 4, "b50-lin-2")):
        good = {"align_id": hs.op("align", db, qi, sc), "topk0": hs.op("topk", db, qi, sc, ("host", 100))}
        for what, entry in FAILURES:
            before = good.get(what, hs.op("scan", db, qi, sc))
            runner.run(before, "before")
            route = runner.route()
            assert "+drain" in route[0] or db == "B", route
            runner.run(hs.op("fail", db, qi, sc, (what, entry)), "failing")
            assert runner.route() == route, (what, entry)
            runner.run(before, "after")
            assert runner.route() == route, (what, entry)


def test_two_handles(sw, world):
    """Two handles on one device, each with its own copy of A, their
    sw_scan_device calls queued alternately, each on its own stream; one
    synchronise, then every buffer equals the oracle."""
    import torch
    rs = [hs.Runner(sw, world) for _ in range(2)]
    try:
        for r in rs:
            r.profile("lpt64")
        shapes = [(5, "b62x6-66-6"), (4, "b50-lin-2"), (3, "b62-11-1"), (5, "asym-3-5"), (4, "b62x6-66-6"), (2, "b62-11-1")]
        n = world.n_out["A"]
        bufs = [[torch.full((n,), hs.FILL, dtype=torch.int32, device="cuda") for _ in shapes] for _ in rs]
        torch.cuda.synchronize()
        for k, (qi, sc) in enumerate(shapes):
            for j, r in enumerate(rs):
                qj, scj = shapes[(k + 3 * j) % len(shapes)]  # the two handles run different shapes side by side
                r.dbs["A"].scan_device(world.query(qj), bufs[j][k].data_ptr(), *world.scoring(scj))
        torch.cuda.synchronize()
        for k in range(len(shapes)):
            for j, r in enumerate(rs):
                qj, scj = shapes[(k + 3 * j) % len(shapes)]
                r.check_buffer(bufs[j][k].cpu().numpy(), "A", qj, scj, ("two handles", j, k))
    finally:
        for r in rs:
            r.close()


def test_oracle_time(world):
    """The module's oracle work, printed (DESIGN.md §3 quotes it)."""
    print("HISTORY oracle seconds %.1f over %d scans" % (world.oracle_seconds, len(world._want)))
    assert world.oracle_seconds < 60
