"""Scan histories: one handle and resident databases across mixed calls.
Shared by tests/test_history_plan.py (CPU: the coverage of what will run) and
tests/test_gpu_history.py (the histories on the device).

The host driver keeps state that outlives a scan: per database the drain
blobs (32 slots), the merged launch's work tables (8), the rescue lists in
two parities, the two readbacks and the int16-first staircases, the first-use
tables of sw_align / sw_hit_stats / sw_scan_topk; per handle the ring of 4
profile slots, the list parity, the score buffer sw_scan_topk shares with its
keys, the top-K workspace, the sw_opts every plan and cache key reads.  A
fault in that state changes a score or a route only for one *order* of calls,
so the unit here is a history: a list of Op, each naming its database, run
on one handle, every result compared with the oracle.

The world (World): database A "mixed" (496 subjects of 1..1,500 residues, 12
of 1,600..3,000, long threshold 1500, near-copies of the 900 and the 1,300
query, one insertion and one deletion each, one among the short and one
behind random residues among the long subjects), B "short only" (130
subjects, none long, result ids with gaps: never merged, another score buffer
size), C = Database.synthetic(handle, 77, 2000); queries of 1, 63, 120, 375,
900 and 1,300 residues (drawn rich in W, C, H, Y, P so that a copy of 900
residues passes the int16 guard under the matrix times 6) and the empty query
in batches; one PSSM derived from BLOSUM62 for the 375 and the 900 query;
four scorings; six sw_opts profiles.  The adaptive routes stay on.

The vocabulary (KINDS): 12 kinds of Op.  generate() walks an Eulerian circuit
of the complete digraph over the kinds, self-loops included (144 transitions,
so every ordered pair of kinds occurs by construction), cuts it into 4
histories of 37 ops (36 transitions each, the cut op shared) and draws each
op's database and query from a seeded generator; a scan's scoring is one that
follows its database's last in a pair of scorings not seen yet, and the
choices of a kind (profiles, thresholds, k, the failing calls) are taken in
turn.  tests/test_history_plan.py asserts what the draws are to cover.

Oracle work: memoised per (database, query, scoring), nthreads=16; the whole
GPU module's is 2.3 to 5 s on 16 threads, by the host (World.oracle_seconds,
printed by the module's last test)."""
import collections
import time

import numpy as np

from hits_support import expected as expected_row
from hits_support import pack

PAD = np.iinfo(np.int64).min
FILL = -7  # what a fresh device score buffer holds: slots no subject maps to keep it

QLENS = (1, 63, 120, 375, 900, 1300)
EMPTY = -1  # the empty query's index (batches only)
PSSM_Q = (3, 4)  # the queries (375, 900) that have a PSSM
SCORINGS = ("b62-11-1", "b50-lin-2", "b62x6-66-6", "asym-3-5")
GAPS = {"b62-11-1": (11, 1), "b50-lin-2": (2, 2), "b62x6-66-6": (66, 6), "asym-3-5": (3, 5)}
DBS = ("A", "B", "C")
C_SEED, C_N = 77, 2000
A_THRESHOLD = 1500
THRESHOLDS = (64, 500, 1500)
TOPK = (1, 100, 4096)

# sw_opts profiles, each applied to the library's defaults (Handle.reset_opts).
# The merged profiles fix 8 rows per lane for the long subjects: under linear
# gaps the cost model gives a 900-residue query 16 rows and a 1,300-residue
# one 12, which the merged launch is not built for (lpt_supported: 4, 6, 8;
# affine scans are moved to 8 by scan_plan itself), and the histories want
# the drain under every scoring.
MERGED = dict(lpt=1, pair_width=64, intra_x2_rows=8)
PROFILES = collections.OrderedDict([
    ("default", {}),
    ("lpt64", MERGED),
    ("quad16", dict(MERGED, quad_width=16)),
    ("tri16", dict(MERGED, tri_width=16)),
    ("nolpt", dict(lpt=0, pair_width=64)),
    ("int32", dict(inter_variant="32x8", intra_x2=0, int16_guard=0)),
])

KINDS = ("scan", "scan_device", "scan_batch", "topk", "pssm", "hits", "align", "set_opts", "set_threshold",
         "reset_adaptive", "reopen", "fail")
SCORED = ("scan", "scan_device", "scan_batch", "topk", "pssm", "hits", "align")  # kinds that scan under a scoring

# kind      q                   sc        arg
# scan, scan_device, align       index     name      -
# scan_batch                    tuple     name      -
# topk                          index     name      ("host" | "rank", k)
# pssm                          3 | 4     b62-11-1  ("scan",) | ("topk", k)
# hits                          index     name      "scan_hits" | "hit_stats"
# set_opts                      -         -         profile name
# set_threshold (A, C)          -         -         threshold
# reset_adaptive, reopen        -         -         -
# fail                          index     name      (what, entry point): what in gap0, entry101 (entry point in
#                                                    FAIL_ENTRIES), align_id, topk0
Op = collections.namedtuple("Op", "kind db q sc arg")
FAIL_ENTRIES = ("scan", "scan_device", "scan_batch", "topk")


def op(kind, db=None, q=None, sc=None, arg=None):
    return Op(kind, db, q, sc, arg)


# ---- the world ---------------------------------------------------------------
def near_copy(q, rng):
    """q with one residue inserted and one deleted."""
    i, d = sorted(int(x) for x in rng.choice(np.arange(10, len(q) - 10), size=2, replace=False))
    return np.concatenate([q[:i], [(int(q[i]) + 1) % 20], q[i:d], q[d + 1:]]).astype(np.uint8)


class World:
    """Queries, matrices, the databases' residues and the oracle's memoised
    answers.  Needs no device; database C's residues are attached by the GPU
    module (set_c) from what Database.subjects() reports."""

    def __init__(self, oracle, seed=2024):
        self.oracle = oracle
        self.oracle_seconds = 0.0
        rng = np.random.default_rng(seed)
        rich = np.array(list(range(20)) + [17, 4, 8, 18, 14] * 2, dtype=np.uint8)  # W C H Y P thrice as often
        self.queries = [rich[rng.integers(0, len(rich), size=n)] for n in QLENS]
        b62 = np.asarray(oracle.matrix(oracle.MATRIX_BLOSUM62), dtype=np.int8).reshape(25, 25)
        b50 = np.asarray(oracle.matrix(oracle.MATRIX_BLOSUM50_REF), dtype=np.int8).reshape(25, 25)
        asym = rng.integers(-9, 14, size=(25, 25))
        np.fill_diagonal(asym, rng.integers(1, 14, size=25))
        assert (asym != asym.T).any()
        self.mats = {"b62-11-1": b62, "b50-lin-2": b50, "b62x6-66-6": (b62.astype(np.int32) * 6).astype(np.int8),
                     "asym-3-5": asym.astype(np.int8)}
        self.pssm_rows = {qi: np.ascontiguousarray(b62[self.queries[qi].astype(np.int64)]) for qi in PSSM_Q}

        def rand(n):
            return rng.integers(0, 25, size=int(n)).astype(np.uint8)
        q900, q1300 = self.queries[4], self.queries[5]
        lens = np.clip(rng.lognormal(np.log(300), 0.8, size=496), 1, 1500).astype(np.int64)
        lens[:8] = (1, 1500, 63, 64, 65, 15, 16, 17)
        a = [rand(n) for n in lens] + [rand(n) for n in rng.integers(1600, 3001, size=12)]
        a += [near_copy(q900, rng), near_copy(q1300, rng),
              np.concatenate([rand(700), near_copy(q900, rng)]), np.concatenate([rand(400), near_copy(q1300, rng)])]
        a = [a[k] for k in rng.permutation(len(a))]
        b = [rand(n) for n in rng.integers(1, 401, size=130)]
        self.subs = {"A": a, "B": b}
        self.ids = {"A": np.arange(len(a), dtype=np.int32),
                    "B": np.sort(rng.permutation(400)[:130]).astype(np.int32)[rng.permutation(130)],
                    "C": np.arange(C_N, dtype=np.int32)}
        self.packed = {k: pack(v) for k, v in self.subs.items()}
        self.n_out = {k: int(v.max()) + 1 for k, v in self.ids.items()}
        assert self.n_out["B"] > 130
        self._want, self._rows, self._als = {}, {}, {}

    def set_c(self, subs):
        """Database C's subjects (code arrays in database order)."""
        assert len(subs) == C_N
        if "C" not in self.subs:
            self.subs["C"] = subs
            self.packed["C"] = pack(subs)

    def scoring(self, sc):
        go, ge = GAPS[sc]
        return self.mats[sc], go, ge

    def query(self, qi):
        return np.zeros(0, dtype=np.uint8) if qi == EMPTY else self.queries[qi]

    def want(self, db, qi, sc):
        """The oracle's scores of the database's subjects, in database order."""
        key = (db, qi, sc)
        if key not in self._want:
            if qi == EMPTY:
                self._want[key] = np.zeros(len(self.subs[db]), dtype=np.int32)
            else:
                m, go, ge = self.scoring(sc)
                res, offs = self.packed[db]
                t = time.perf_counter()
                self._want[key] = self.oracle.scan(self.queries[qi], res, offs, mat=m, gap_open=go, gap_extend=ge,
                                                   nthreads=16)
                self.oracle_seconds += time.perf_counter() - t
            self._want[key].setflags(write=False)
        return self._want[key]

    def full(self, db, qi, sc, fill=0):
        """... indexed by result id, as a scan returns them."""
        out = np.full(self.n_out[db], fill, dtype=np.int32)
        out[self.ids[db]] = self.want(db, qi, sc)
        return out

    def keys(self, db, qi, sc, k):
        """The k best as int64 keys, padded to k."""
        from_oracle = local_topk(self.want(db, qi, sc), self.ids[db], k)
        return np.concatenate([from_oracle, np.full(k - len(from_oracle), PAD, dtype=np.int64)])

    def top_ids(self, db, qi, sc, k):
        """(result id, subject index) of the k best, best first."""
        keys = local_topk(self.want(db, qi, sc), self.ids[db], k)
        rids = ((1 << 31) - 1) - (keys & 0xFFFFFFFF)
        where = {int(r): i for i, r in enumerate(self.ids[db])}
        return [(int(r), where[int(r)]) for r in rids]

    def rows(self, db, qi, sc, k=5):
        """The hit table's rows of the k best (hits_support.expected)."""
        key = (db, qi, sc, k)
        if key not in self._rows:
            m, go, ge = self.scoring(sc)
            t = time.perf_counter()
            self._rows[key] = [expected_row(self.oracle, self.queries[qi], self.subs[db][i], m, go, ge, rid)
                               for rid, i in self.top_ids(db, qi, sc, k)]
            self.oracle_seconds += time.perf_counter() - t
        return self._rows[key]

    def alignments(self, db, qi, sc, k=3):
        key = (db, qi, sc, k)
        if key not in self._als:
            m, go, ge = self.scoring(sc)
            t = time.perf_counter()
            self._als[key] = [self.oracle.align(self.queries[qi], self.subs[db][i], m, go, ge)
                              for _, i in self.top_ids(db, qi, sc, k)]
            self.oracle_seconds += time.perf_counter() - t
        return self._als[key]

    def prepare(self, ops):
        """Every oracle answer the ops will ask for, ahead of their run."""
        for o in ops:
            if o.kind not in SCORED:
                continue
            for qi in (o.q if o.kind == "scan_batch" else (o.q,)):
                self.want(o.db, qi, o.sc)
            if o.kind == "hits":
                self.rows(o.db, o.q, o.sc)
            if o.kind == "align":
                self.alignments(o.db, o.q, o.sc)


def c_subjects(sw, lengths, ids):
    """Database C's subjects regenerated on the CPU (synth.counter_residues)
    from the lengths and ids Database.subjects() reports."""
    table, lut = sw.capi.synth_tables()
    assert np.array_equal(ids, np.arange(C_N))
    assert np.array_equal(lengths, sw.synth.counter_lengths(C_SEED, np.arange(C_N), table))
    return [sw.synth.counter_residues(C_SEED, g, int(n), lut).astype(np.uint8) for g, n in enumerate(lengths)]


def local_topk(scores, ids, k):
    """sw.dist.local_topk (restated: this module imports without the package)."""
    keys = (np.asarray(scores, dtype=np.int64) << 32) | (((1 << 31) - 1) - np.asarray(ids, dtype=np.int64))
    return np.sort(keys)[::-1][:k]


# ---- the generator -----------------------------------------------------------
def euler_circuit(n, rng):
    """An Eulerian circuit of the complete digraph on n nodes with self-loops
    (Hierholzer): n * n + 1 nodes, the first again at the end."""
    out = {v: [int(w) for w in rng.permutation(n)] for v in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == n * n + 1 and circuit[0] == circuit[-1]
    return circuit


N_HISTORIES = 4


def generate(seed=11):
    """The 4 generated histories (lists of Op)."""
    rng = np.random.default_rng(seed)
    kinds = euler_circuit(len(KINDS), rng)
    per = (len(kinds) - 1) // N_HISTORIES
    # per database: the ordered pairs of scorings still to come, and the last
    # scoring scanned under in this history
    need = {d: {(a, b) for a in SCORINGS for b in SCORINGS if a != b} for d in DBS}
    last = {}

    def next_scoring(db):
        """A scoring that follows the database's last one in a pair still
        missing, else the one with the most missing pairs ahead of it."""
        def ahead(s):
            return sum((s, t) in need[db] for t in SCORINGS)
        cand = [s for s in SCORINGS if (last.get(db), s) in need[db]] or [s for s in SCORINGS if s != last.get(db)]
        return max(cand, key=lambda s: (ahead(s), -SCORINGS.index(s)))

    def scanned(db, sc):
        need[db].discard((last.get(db), sc))
        last[db] = sc

    def pick(seq, p=None):
        return seq[int(rng.choice(len(seq), p=p))]

    turn = collections.Counter()

    def rotate(kind, seq):
        """The kind's choices in turn (12 ops of each kind: every choice is taken)."""
        turn[kind] += 1
        return seq[(turn[kind] - 1) % len(seq)]

    def draw(kind):
        db = pick(DBS)
        qi = pick(range(len(QLENS)), p=[.1, .1, .1, .2, .25, .25])
        sc = "b62-11-1" if kind == "pssm" else next_scoring(db) if kind in SCORED else pick(SCORINGS)
        if kind in SCORED:
            scanned(db, sc)
        if kind in ("scan", "scan_device", "align"):
            return op(kind, db, qi, sc)
        if kind == "scan_batch":
            qs = [pick(range(len(QLENS)), p=[.1, .1, .15, .25, .2, .2]) for _ in range(int(rng.integers(2, 8)))]
            where = pick(("start", "middle", "end", "none", "both"))
            if where in ("start", "both"):
                qs.insert(0, EMPTY)
            if where == "middle":
                qs.insert(len(qs) // 2, EMPTY)
            if where in ("end", "both"):
                qs.append(EMPTY)
            return op(kind, db, tuple(qs), sc)
        if kind == "topk":
            return op(kind, db, qi, sc, rotate(kind, [(how, k) for k in TOPK[::-1] for how in ("host", "rank")]))
        if kind == "pssm":
            return op(kind, db, pick(PSSM_Q), "b62-11-1", rotate(kind, (("scan",), ("topk", 100))))
        if kind == "hits":
            return op(kind, db, qi, sc, rotate(kind, ("scan_hits", "hit_stats")))
        if kind == "set_opts":
            return op(kind, arg=rotate(kind, list(PROFILES)[1:] + ["default"]))
        if kind == "set_threshold":
            return op(kind, pick(("A", "C")), arg=rotate(kind, THRESHOLDS))
        if kind in ("reset_adaptive", "reopen"):
            return op(kind, rotate(kind, DBS))
        what = rotate(kind, ("gap0", "entry101", "align_id", "topk0"))
        return op("fail", db, qi, sc, (what, pick(FAIL_ENTRIES) if what in ("gap0", "entry101") else None))

    histories = []
    for h in range(N_HISTORIES):
        last.clear()
        if histories and histories[-1][-1].kind in SCORED:
            last[histories[-1][-1].db] = histories[-1][-1].sc
        ks = kinds[h * per: (h + 1) * per + 1]
        # the op a cut shares is drawn once: the next history starts with the same op
        first = [histories[-1][-1]] if histories else [draw(KINDS[ks[0]])]
        histories.append(first + [draw(KINDS[k]) for k in ks[1:]])
    return histories


def transitions(history, key):
    """Consecutive pairs of key(op) over the ops for which it is not None."""
    seq = [key(o) for o in history if key(o) is not None]
    return set(zip(seq, seq[1:]))


# ---- the executor ------------------------------------------------------------
class Runner:
    """One handle, the three databases and the two PSSMs; runs ops and checks
    each against the World.  routes collects (last_kernel, last_intra_kernel)
    after every op of a synced run."""

    def __init__(self, sw, world, handle=None):
        self.sw, self.w = sw, world
        self.h = handle or sw.Handle(0, env_opts=False)
        self.own = handle is None
        self.h.reset_opts()
        self.dbs, self.routes = {}, []
        for name in DBS:
            self.open(name)
        self.pssm = {qi: sw.Pssm(self.h, rows) for qi, rows in world.pssm_rows.items()}

    def open(self, name):
        sw, w = self.sw, self.w
        if name == "C":
            self.dbs[name] = sw.Database.synthetic(self.h, C_SEED, C_N)
        else:
            res, offs = w.packed[name]
            self.dbs[name] = sw.Database(self.h, res, offs, ids=w.ids[name] if name == "B" else None,
                                         long_threshold=A_THRESHOLD if name == "A" else None)
        assert self.dbs[name].n_out == w.n_out[name]

    def close(self):
        for p in self.pssm.values():
            p.close()
        for db in self.dbs.values():
            db.close()
        if self.own:
            self.h.close()
        else:
            self.h.reset_opts()

    def profile(self, name, **more):
        self.h.reset_opts()
        self.h.set_opts(**dict(PROFILES[name], **more))

    def route(self):
        return self.h.last_kernel(), self.h.last_intra_kernel()

    # -- checks ----------------------------------------------------------------
    def check_buffer(self, got, db, qi, sc, what):
        """A device score buffer that held FILL before the scan."""
        want = self.w.full(db, qi, sc, fill=0 if qi == EMPTY else FILL)
        assert np.array_equal(got, want), (what, self.route(), np.nonzero(got != want)[0][:10])

    def check_scores(self, got, db, qi, sc, what):
        want = self.w.full(db, qi, sc)
        assert np.array_equal(got, want), (what, self.route(), np.nonzero(got != want)[0][:10])

    def bad_scoring(self, what, sc):
        m, go, ge = self.w.scoring(sc)
        if what == "gap0":
            return m, 0, ge
        m = m.copy()
        m[3, 5] = 101
        return m, go, ge

    # -- one op, host-synchronous ------------------------------------------------
    def run(self, o, label=""):
        import torch
        sw, w, h = self.sw, self.w, self.h
        db = self.dbs.get(o.db)
        what = (label, o)
        if o.kind == "scan":
            self.check_scores(db.scan(w.query(o.q), *w.scoring(o.sc)), o.db, o.q, o.sc, what)
        elif o.kind == "scan_device":
            buf = torch.full((db.n_out,), FILL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # the fill ran on torch's stream
            db.scan_device(w.query(o.q), buf.data_ptr(), *w.scoring(o.sc))
            torch.cuda.synchronize()
            self.check_buffer(buf.cpu().numpy(), o.db, o.q, o.sc, what)
        elif o.kind == "scan_batch":
            got = db.scan_batch([w.query(qi) for qi in o.q], *w.scoring(o.sc))
            for row, qi in zip(got, o.q):
                self.check_scores(row, o.db, qi, o.sc, what)
        elif o.kind == "topk":
            how, k = o.arg
            if how == "host":
                keys = db.scan_topk(w.query(o.q), k, *w.scoring(o.sc))
            else:
                buf = torch.full((db.n_out,), FILL, dtype=torch.int32, device="cuda")
                kbuf = torch.zeros(k, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                db.scan_rank_device(w.query(o.q), buf.data_ptr(), k, kbuf.data_ptr(), *w.scoring(o.sc))
                torch.cuda.synchronize()
                self.check_buffer(buf.cpu().numpy(), o.db, o.q, o.sc, what)
                keys = kbuf.cpu().numpy()
            assert np.array_equal(keys, w.keys(o.db, o.q, o.sc, k)), (what, self.route())
        elif o.kind == "pssm":
            go, ge = GAPS[o.sc]
            if o.arg[0] == "scan":
                self.check_scores(db.scan_pssm(self.pssm[o.q], go, ge), o.db, o.q, o.sc, what)
            else:
                keys = db.scan_pssm_topk(self.pssm[o.q], o.arg[1], go, ge)
                assert np.array_equal(keys, w.keys(o.db, o.q, o.sc, o.arg[1])), (what, self.route())
        elif o.kind == "hits":
            q = w.query(o.q)
            if o.arg == "scan_hits":
                got = db.scan_hits(q, 5, *w.scoring(o.sc))
            else:
                got = db.hit_stats(q, [rid for rid, _ in w.top_ids(o.db, o.q, o.sc, 5)], *w.scoring(o.sc))
            assert got == w.rows(o.db, o.q, o.sc), (what, self.route())
        elif o.kind == "align":
            from conftest import path_score
            q = w.query(o.q)
            m, go, ge = w.scoring(o.sc)
            top = w.top_ids(o.db, o.q, o.sc, 3)
            got = db.align(q, [rid for rid, _ in top], m, go, ge)
            for al, want, (_, i) in zip(got, w.alignments(o.db, o.q, o.sc), top):
                assert al["score"] == want["score"] == w.want(o.db, o.q, o.sc)[i], (what, al, want)
                if want["score"] > 0:
                    assert al == want, (what, al, want)
                    assert path_score(q, w.subs[o.db][i], m, go, ge, al) == al["score"], (what, al)
        elif o.kind == "set_opts":
            self.profile(o.arg)
        elif o.kind == "set_threshold":
            db.set_long_threshold(o.arg)
        elif o.kind == "reset_adaptive":
            db.reset_adaptive()
        elif o.kind == "reopen":
            db.close()
            self.open(o.db)
        elif o.kind == "fail":
            self.fail(o, device=False)
        else:
            raise AssertionError(o)

    def fail(self, o, device):
        """A call that must raise SWError and leave everything as it was."""
        import pytest
        import torch
        w, db = self.w, self.dbs[o.db]
        what, entry = o.arg
        q = w.query(o.q)
        with pytest.raises(self.sw.capi.SWError):
            if what == "align_id":
                db.align(q, [w.n_out[o.db] + 5], *w.scoring(o.sc))
            elif what == "topk0":
                db.scan_topk(q, 0, *w.scoring(o.sc))
            else:
                bad = self.bad_scoring(what, o.sc)
                if device or entry == "scan_device":
                    buf = torch.full((3 * db.n_out,), FILL, dtype=torch.int32, device="cuda")
                    kbuf = torch.zeros(8, dtype=torch.int64, device="cuda")
                    if entry == "scan_batch":
                        db.scan_batch_device([q, q[:1], q], buf.data_ptr(), *bad)
                    elif entry == "topk":
                        db.scan_rank_device(q, buf.data_ptr(), 8, kbuf.data_ptr(), *bad)
                    else:
                        db.scan_device(q, buf.data_ptr(), *bad)
                elif entry == "scan":
                    db.scan(q, *bad)
                elif entry == "scan_batch":
                    db.scan_batch([q, q[:1], q], *bad)
                else:
                    db.scan_topk(q, 5, *bad)

    def run_synced(self, ops, label=""):
        """Every op ends in a host-synchronous call or a device synchronise;
        returns the routes, one per op."""
        routes = []
        for k, o in enumerate(ops):
            self.run(o, "%s#%d" % (label, k))
            routes.append(self.route())
        return routes

    # -- queued: device entry points only, one synchronise at the end -------------
    def run_queued(self, ops, label=""):
        """scan, hits and align ops become sw_scan_device (hits: with the
        ranking of its top 5), batches sw_scan_batch_device, topk
        sw_scan_rank_device, pssm sw_scan_pssm_device, each into a buffer of
        its own; no host wait between the ops beyond what set_long_threshold,
        a close and the library itself impose."""
        import torch
        w = self.w
        bufs, kbufs = {}, {}
        for k, o in enumerate(ops):
            if o.kind in SCORED:
                nq = len(o.q) if o.kind == "scan_batch" else 1
                bufs[k] = torch.full((nq, w.n_out[o.db]), FILL, dtype=torch.int32, device="cuda")
                if o.kind in ("topk", "hits"):
                    kbufs[k] = torch.zeros(o.arg[1] if o.kind == "topk" else 5, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # the fills ran on torch's stream
        for k, o in enumerate(ops):
            db = self.dbs.get(o.db)
            if o.kind in ("scan", "scan_device", "align"):
                db.scan_device(w.query(o.q), bufs[k].data_ptr(), *w.scoring(o.sc))
            elif o.kind == "scan_batch":
                db.scan_batch_device([w.query(qi) for qi in o.q], bufs[k].data_ptr(), *w.scoring(o.sc))
            elif o.kind in ("topk", "hits"):
                db.scan_rank_device(w.query(o.q), bufs[k].data_ptr(), len(kbufs[k]), kbufs[k].data_ptr(),
                                    *w.scoring(o.sc))
            elif o.kind == "pssm":
                db.scan_pssm_device(self.pssm[o.q], bufs[k].data_ptr(), *GAPS[o.sc])
            elif o.kind == "fail":
                self.fail(o, device=True)
            else:
                self.run(o)
        torch.cuda.synchronize()
        for k, o in enumerate(ops):
            if k not in bufs:
                continue
            got = bufs[k].cpu().numpy()
            for row, qi in zip(got, o.q if o.kind == "scan_batch" else (o.q,)):
                self.check_buffer(row, o.db, qi, o.sc, ("%s#%d queued" % (label, k), o))
            if k in kbufs:
                n = len(kbufs[k])
                assert np.array_equal(kbufs[k].cpu().numpy(), w.keys(o.db, o.q, o.sc, n)), (label, k, o)
