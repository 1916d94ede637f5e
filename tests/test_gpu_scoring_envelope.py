"""GPU: every kernel family at the edges of the scoring envelope, bit for bit
against the CPU oracle.

check_scoring accepts matrix entries -100..100 and gaps 1..1000, and
swplan::scan_plan switches kernel families on three predicates of the
scoring (tests/native/plan_check.cpp pins them on the CPU; the names
asserted here are the same ones):

  S + go > 127                          a linear gap runs the affine kernels
  2 max S + 27 ge + go < 1024           fp16 / int16, else int32
  2 max S + 39 ge + go < 1024           20 rows per lane (long subjects only)

The scorings below sit on both sides of each, under matrices that are NOT
symmetric (row = query code, column = subject code: a transposed index in
any profile image or in the traceback shows), with entries and gaps at the
ends of the accepted range.  One small database per module run: residues
uniform over all 25 codes, subjects of 1..1,500 residues, planted copies of
the 375-aa query with a deletion and an insertion; queries of one pass, three
passes (the last one short) and six.  The oracle's scores are computed once
per (scoring, query).

The second half plants prefixes of the query whose self-scores sit within
three residues of each guard limit (the fp16 cells' sat_limit and the int16
forms' kSat16, computed here from DESIGN.md §4's formulas, not read from the
library): below the limit nothing is flagged and the 16-bit form itself is
exact, at the limit the block / subject is flagged and re-scored.

No tolerance anywhere: every comparison is np.array_equal or ==."""
import re

import numpy as np
import pytest

from conftest import path_score
from hits_envelope_support import build_matrices

pytestmark = pytest.mark.gpu

A, R = 0, 1  # residue codes of 'A' and 'R'


# ---- the scorings -----------------------------------------------------------
# build_matrices(sw): tests/hits_envelope_support.py (the hit table's envelope tests share the matrices)


# name: (matrix, open, extend, gap model of the kernels that run, fits 16 bits
# (2 max S + 27 ge + go < 1024), fits 20 rows per lane (2 max S + 39 ge + go <
# 1024)) -- the routes are literals: tests/native/plan_check.cpp pins the same
# ones through swplan::plan_scoring and scan_plan
SCORINGS = {
    "asym-12-1": ("asym", 12, 1, "affine", True, True),
    "asym-2-2": ("asym", 2, 2, "linear", True, True),
    "asym-7-3": ("asym", 7, 3, "affine", True, True),
    "one-entry-12-1": ("one", 12, 1, "affine", True, True),
    "one-entry-2-2": ("one", 2, 2, "linear", True, True),
    "int8-fits-27": ("d100", 27, 27, "linear", True, False),      # S + g = 127
    "int8-over-28": ("d100", 28, 28, "affine", True, False),      # S + g = 128: affine kernels, linear gap
    "big-ge-191-30": ("b62", 191, 30, "affine", True, False),     # sum 1023
    "big-ge-192-30": ("b62", 192, 30, "affine", False, False),    # sum 1024
    "big-ge-d100-40-28": ("d100", 40, 28, "affine", True, False),  # sum 996, scores to 37,500
    "big-go-974-1": ("b62", 974, 1, "affine", True, False),       # sum 1023
    "big-go-975-1": ("b62", 975, 1, "affine", False, False),      # sum 1024
    "big-linear-35": ("b50", 35, 35, "linear", True, False),      # sum 1010
    "big-linear-36": ("b50", 36, 36, "linear", False, False),     # sum 1038
    "non-positive-12-1": ("nonpos", 12, 1, "affine", True, True),
    "non-positive-2-2": ("nonpos", 2, 2, "linear", True, True),
    "limits-1000-1000": ("pm100", 1000, 1000, "affine", False, False),
}


def inter_name(gap, fits, variant=""):
    """The inter kernel's name (wave groups, strip height and suffixes aside)."""
    if variant in ("32x8", "64x8"):
        return "sw_inter<%s,8,%s>" % (variant[:2], gap)
    if not fits:
        return "sw_inter<%s,8,%s>" % ("32" if gap == "affine" else "64", gap)
    return "sw_inter_x2s<32,8,%s%s>" % (gap, "" if variant == "y32x8" else ",fp16")


def base(name):
    return name.split(">")[0].replace("sw_inter_x2p", "sw_inter_x2s").replace("<48,", "<32,") + ">"


# ---- the database -----------------------------------------------------------
class Env:
    pass


def build_subjects():
    rng = np.random.default_rng(77)
    q0 = rng.integers(0, 25, size=375).astype(np.uint8)
    subs = []
    for lo, hi, forced in ((1, 40, (1, 2, 39, 40)), (41, 136, (63, 64, 65, 128, 129, 136)), (137, 300, (137, 256, 257, 300))):
        lens = list(forced) + [int(x) for x in rng.integers(lo, hi + 1, size=64 - len(forced))]
        subs += [rng.integers(0, 25, size=n).astype(np.uint8) for n in lens]
    subs += [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(700, 1501, size=12)]
    ins = np.sort(rng.integers(20, 355, size=5))
    planted = [q0.copy(), q0[:190].copy(), np.concatenate([q0[:180], q0[183:]]),
               np.insert(q0, ins, rng.integers(0, 25, size=5).astype(np.uint8))]
    first_planted = len(subs)
    subs += planted
    reps = {}
    for code, lens in ((R, (1, 63, 64, 200)), (A, (50, 300))):
        for n in lens:
            reps[(code, n)] = len(subs)
            subs.append(np.full(n, code, dtype=np.uint8))
    return q0, subs, list(range(first_planted, first_planted + 4)), reps


def pack(subs):
    res = np.concatenate(subs).astype(np.uint8)
    offs = np.zeros(len(subs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subs])
    return res, offs


@pytest.fixture(scope="module")
def env(sw, oracle, handle):
    e = Env()
    e.mats = build_matrices(sw)
    e.q0, e.subs, e.planted, e.reps = build_subjects()
    assert len(set(np.concatenate(e.subs).tolist())) == 25   # B, J, Z, X and * occur
    e.res, e.offs = pack(e.subs)
    e.long_sel = np.array([k for k, s in enumerate(e.subs) if len(s) > 64])
    lres, loffs = pack([e.subs[k] for k in e.long_sel])
    e.all_sel = np.arange(len(e.subs))
    e.db = {"mixed": sw.Database(handle, e.res, e.offs),
            "merged": sw.Database(handle, e.res, e.offs, long_threshold=600),
            "long": sw.Database(handle, lres, loffs, long_threshold=64)}
    st = {k: d.stats() for k, d in e.db.items()}
    assert st["long"]["n_blocks"] == 0 and st["long"]["n_long"] == len(e.long_sel)
    assert st["merged"]["n_long"] == 12 and st["merged"]["n_blocks"] >= 3
    assert st["mixed"]["n_blocks"] >= 3
    e.sel = {"mixed": e.all_sel, "merged": e.all_sel, "long": e.long_sel}
    cache = {}

    def queries(scname):
        if SCORINGS[scname][0] == "one":
            return [np.full(n, A, dtype=np.uint8) for n in (40, 130, 375)]
        return [e.q0[:40], e.q0[:130], e.q0]

    def want(scname, qi):
        if (scname, qi) not in cache:
            mk, go, ge = SCORINGS[scname][:3]
            cache[(scname, qi)] = oracle.scan(queries(scname)[qi], e.res, e.offs, mat=e.mats[mk], gap_open=go,
                                              gap_extend=ge)
            cache[(scname, qi)].setflags(write=False)
        return cache[(scname, qi)]

    e.queries, e.want = queries, want
    yield e
    for d in e.db.values():
        d.close()


def scan_check(e, handle, dbname, scname, qi, label):
    """One scan against the oracle; returns (inter name, intra name)."""
    mk, go, ge = SCORINGS[scname][:3]
    db = e.db[dbname]
    got = db.scan(e.queries(scname)[qi], e.mats[mk], go, ge)
    w = e.want(scname, qi)[e.sel[dbname]]
    names = (handle.last_kernel(), handle.last_intra_kernel())
    print("ENVELOPE %s | %s | q%d | %s | %s" % (scname, label, len(e.queries(scname)[qi]), *names))
    bad = np.nonzero(got != w)[0]
    assert not len(bad), (scname, label, qi, names, bad[:10], got[bad[:10]], w[bad[:10]])
    return names


def intra_ok(name, gap, fits):
    return name.startswith("sw_intra_x2<") if fits else (name.startswith("sw_intra<") and name.endswith(",%s>" % gap))


# ---- every form under every scoring ----------------------------------------
@pytest.mark.parametrize("scname", list(SCORINGS))
def test_default_plan(env, handle, scname):
    """The library's own plan (no sw_opts override)."""
    _, _, _, gap, fits, _ = SCORINGS[scname]
    for qi in range(3):
        k, ik = scan_check(env, handle, "mixed", scname, qi, "default")
        assert base(k) == inter_name(gap, fits), k
        assert intra_ok(ik, gap, fits), ik
        if scname.startswith("non-positive"):
            assert not env.want(scname, qi).any()


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_inter_variants(env, handle, knobs, scname):
    """Each inter shape forced (the int32 ones with the cooperative kernel
    off and on; the int16 and fp16 two-strips kernels): where the scoring
    does not fit 16 bits the forced 16-bit shapes fall back to int32."""
    _, _, _, gap, fits, _ = SCORINGS[scname]
    for variant, coop in (("32x8", 0), ("32x8", 128), ("64x8", 0), ("64x8", 128), ("y32x8", None), ("f32x8", None)):
        knobs(inter_variant=variant, coop_width=-1 if coop is None else coop)
        for qi in range(3):
            k, ik = scan_check(env, handle, "mixed", scname, qi, "%s coop %s" % (variant, coop))
            assert base(k) == inter_name(gap, fits, variant), (variant, k)
            assert intra_ok(ik, gap, fits), ik
            if coop is not None:
                assert (env.db["mixed"].stats()["coop_blocks"] > 0) == (coop > 0), (variant, coop)


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_merged_launch(env, handle, knobs, scname):
    """sw_scan_lpt with quads, with 3-wave groups, and switched off: scans
    of at least two passes whose scoring fits 16 bits take it (3-wave groups
    under the affine kernels only); one-pass and int32 scans cannot."""
    _, _, _, gap, fits, _ = SCORINGS[scname]
    for label, opts in (("lpt quads", dict(lpt=1, quad_width=16, tri_width=0)),
                        ("lpt tris", dict(lpt=1, quad_width=-1, tri_width=16)),
                        ("lpt 0", dict(lpt=0, quad_width=-1, tri_width=-1))):
        knobs(pair_width=64, inter_i16_span=0, intra_i16_first=0, **opts)
        for qi in range(3):
            k, ik = scan_check(env, handle, "merged", scname, qi, label)
            assert base(k) == inter_name(gap, fits), k
            assert intra_ok(ik, gap, fits), ik
            merged = fits and qi > 0 and opts["lpt"] == 1
            assert ("+lpt" in k) == merged, (label, qi, k)
            assert ("+tri" in k) == (merged and label == "lpt tris" and gap == "affine"), (label, qi, k)
            assert ("sw_inter_x2p" in k) == (fits and qi > 0), k


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_long_subjects_only(env, handle, knobs, scname):
    """Every subject on the wavefront kernels: the fp16 two-subjects form at
    4, 8 and 20 rows per lane (20 only inside its own bound), the int32 form
    alone, and the int16 form first."""
    _, _, _, gap, fits, wide = SCORINGS[scname]
    for label, opts in (("rows 4", dict(intra_x2_rows=4)), ("rows 8", dict(intra_x2_rows=8)),
                        ("rows 20", dict(intra_x2_rows=20)), ("intra_x2 0", dict(intra_x2=0)),
                        ("int16 first", dict(intra_i16_first=1))):
        knobs(intra_x2=-1, intra_x2_rows=-1, intra_i16_first=0)
        knobs(**opts)
        for qi in range(3):
            _, ik = scan_check(env, handle, "long", scname, qi, label)
            if not fits or label == "intra_x2 0":
                assert intra_ok(ik, gap, False), ik
            elif label == "int16 first":
                assert ik.startswith("sw_intra_x2<") and ik.endswith(",int16>"), ik
            elif label == "rows 20" and not wide:
                assert ik.startswith("sw_intra_x2<") and ik != "sw_intra_x2<20>", ik
            else:
                assert ik == "sw_intra_x2<%s>" % label.split()[1], ik


@pytest.mark.parametrize("go,ik_want", [(221, "sw_intra_x2<20>"), (222, None)])
def test_rows20_bound(env, oracle, handle, knobs, go, ik_want):
    """2 max S + 39 ge + go at 1023 and 1024 (BLOSUM62, extend 20): 20 rows
    per lane on one side, a narrower fp16 form on the other."""
    knobs(intra_x2_rows=20)
    m = env.mats["b62"]
    assert 2 * 11 + 39 * 20 + 221 == 1023
    lres, loffs = pack([env.subs[k] for k in env.long_sel])
    for q in (env.q0[:130], env.q0):
        got = env.db["long"].scan(q, m, go, 20)
        ik = handle.last_intra_kernel()
        print("ENVELOPE b62-%d-20 | rows 20 | q%d | | %s" % (go, len(q), ik))
        assert np.array_equal(got, oracle.scan(q, lres, loffs, mat=m, gap_open=go, gap_extend=20))
        assert ik == ik_want if ik_want else (ik.startswith("sw_intra_x2<") and ik != "sw_intra_x2<20>"), ik


@pytest.mark.parametrize("scname", ["one-entry-12-1", "one-entry-2-2"])
def test_one_entry_closed_form(env, handle, knobs, scname):
    """Only S[A][R] = 5: an all-A query scores 5 min(qlen, slen) against an
    all-R subject and 0 against an all-A one; with the roles swapped (an
    all-R query) every score is 0.  No oracle involved."""
    mk, go, ge = SCORINGS[scname][:3]
    m = env.mats[mk]
    for dbname, opts in (("mixed", {}), ("mixed", dict(inter_variant="y32x8")), ("mixed", dict(inter_variant="32x8")),
                         ("merged", dict(lpt=1, pair_width=64)), ("long", {}), ("long", dict(intra_x2=0))):
        knobs(inter_variant="", lpt=-1, pair_width=-1, intra_x2=-1)
        knobs(**opts)
        pos = {int(k): j for j, k in enumerate(env.sel[dbname])}
        for qlen in (40, 130, 375):
            got = env.db[dbname].scan(np.full(qlen, A, dtype=np.uint8), m, go, ge)
            swapped = env.db[dbname].scan(np.full(qlen, R, dtype=np.uint8), m, go, ge)
            for (code, n), k in env.reps.items():
                if k in pos:
                    assert got[pos[k]] == (5 * min(qlen, n) if code == R else 0), (dbname, opts, qlen, code, n)
            assert not swapped.any(), (dbname, opts, qlen, np.nonzero(swapped)[0][:10])
    for qlen in (40, 375):
        for n in (1, 63, 64, 200):
            a, r = np.full(qlen, A, dtype=np.uint8), np.full(n, R, dtype=np.uint8)
            assert handle.score_pair(a, r, m, go, ge) == 5 * min(qlen, n)
            assert handle.score_pair(r, a, m, go, ge) == 0


@pytest.mark.parametrize("scname", list(SCORINGS))
def test_score_pair_planted(env, handle, scname):
    """sw_score_pair on the planted pairs."""
    mk, go, ge = SCORINGS[scname][:3]
    for qi in range(3):
        w = env.want(scname, qi)
        for k in env.planted:
            assert handle.score_pair(env.queries(scname)[qi], env.subs[k], env.mats[mk], go, ge) == w[k], (qi, k)


@pytest.mark.parametrize("dbname", ["mixed", "merged", "long"])
@pytest.mark.parametrize("scname", ["asym-7-3", "int8-fits-27", "int8-over-28", "big-ge-d100-40-28", "limits-1000-1000"])
def test_batch(env, handle, knobs, scname, dbname):
    """sw_scan_batch: the three queries twice over in one batch (each
    query's rescue tail beside the next query's first pass: under the
    diagonal-100 matrix the planted copies go down both rescue chains)."""
    mk, go, ge = SCORINGS[scname][:3]
    knobs(pair_width=64)
    order = [2, 1, 0, 2, 0, 1]
    out = env.db[dbname].scan_batch([env.queries(scname)[k] for k in order], env.mats[mk], go, ge)
    for j, k in enumerate(order):
        w = env.want(scname, k)[env.sel[dbname]]
        assert np.array_equal(out[j], w), (j, k, np.nonzero(out[j] != w)[0][:10])


@pytest.mark.parametrize("scname", ["asym-2-2", "asym-12-1", "int8-over-28", "big-ge-191-30"])
def test_align(env, sw, oracle, handle, scname):
    """sw_align on the top 10 hits and the four planted subjects: equal to
    the oracle's traceback (int8-over-28 is a linear gap, so the linear
    traceback kernel runs while the scan takes the affine kernels), the
    path's own score equal to the reported one and to the scan's."""
    mk, go, ge = SCORINGS[scname][:3]
    m, q = env.mats[mk], env.q0
    scores = env.db["mixed"].scan(q, m, go, ge)
    assert np.array_equal(scores, env.want(scname, 2))
    top, _ = sw.capi.topk(scores, 10)
    ids = sorted(set(int(i) for i in top) | set(env.planted))
    got = env.db["mixed"].align(q, ids, m, go, ge)
    for i, al in zip(ids, got):
        want = oracle.align(q, env.subs[i], m, go, ge)
        assert al == want, (i, al, want)
        assert al["score"] == scores[i]
        assert al["score"] > 0 and path_score(q, env.subs[i], m, go, ge, al) == al["score"]
    assert any("D" in al["ops"] or "I" in al["ops"] for al in got), "no path with a gap"


def test_invalid_scorings(env, sw, oracle, handle):
    """Entry 101 or -101, gap 0, gap 1001: every scan entry point returns
    SW_E_INVALID (-1), and the next valid scan still equals the oracle."""
    import torch
    db, q = env.db["mixed"], env.q0[:130]
    good = env.mats["asym"]
    hi, lo = good.copy(), good.copy()
    hi[7, 3], lo[3, 7] = 101, -101
    dev = torch.zeros((2, db.n_out), dtype=torch.int32, device="cuda")
    keys = torch.zeros(16, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    calls = {
        "scan": lambda m, go, ge: db.scan(q, m, go, ge),
        "scan_batch": lambda m, go, ge: db.scan_batch([q, q[:40]], m, go, ge),
        "scan_device": lambda m, go, ge: db.scan_device(q, dev.data_ptr(), m, go, ge),
        "scan_batch_device": lambda m, go, ge: db.scan_batch_device([q, q[:40]], dev.data_ptr(), m, go, ge),
        "scan_topk": lambda m, go, ge: db.scan_topk(q, 5, m, go, ge),
        "scan_rank_device": lambda m, go, ge: db.scan_rank_device(q, dev.data_ptr(), 16, keys.data_ptr(), m, go, ge),
        "score_pair": lambda m, go, ge: handle.score_pair(q, env.subs[env.planted[0]], m, go, ge),
        "align": lambda m, go, ge: db.align(q, [0, 1], m, go, ge),
    }
    for what, (m, go, ge) in {"entry 101": (hi, 12, 1), "entry -101": (lo, 12, 1), "open 0": (good, 0, 1),
                              "extend 0": (good, 12, 0), "open 1001": (good, 1001, 1),
                              "extend 1001": (good, 12, 1001), "linear 1001": (good, 1001, 1001)}.items():
        for name, call in calls.items():
            with pytest.raises(sw.capi.SWError, match=r"error -1:"):
                call(m, go, ge)
                pytest.fail("%s accepted %s" % (name, what))
        torch.cuda.synchronize()
        assert np.array_equal(db.scan(q, good, 12, 1), env.want("asym-12-1", 1)), what


# ---- the guard limits to the unit ------------------------------------------
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; "
                    r"pairs \d+; intra (-?\d+)/\d+ flagged, (-?\d+) again")


def bias_rows(ri):
    """The intra cell's bias in gap extensions: max(26, rows per
    lane + bias period + 2), the period 16 steps at 20 rows and 8 otherwise."""
    return max(26, ri + (16 if ri == 20 else 8) + 2)


K_SAT16 = 32767 - 1152


def limit_query(mat, n, rich, seed):
    """A query over the codes whose diagonal entry is positive (`rich`: the
    five largest diagonals among the 20 amino acids, for the int16 limits)."""
    d = np.diag(mat).astype(int)
    codes = np.argsort(-d[:20], kind="stable")[:5] if rich else np.nonzero(d > 0)[0]
    assert (d[codes] > 0).all()
    return np.random.default_rng(seed).choice(codes, size=n).astype(np.uint8)


def edge_sets(oracle, mat, go, ge, limit, rich, seed, lo, hi, n_ordinary=70, junk=0):
    """The query and the two subject sets: ordinary subjects of lo..hi
    residues plus the prefixes just below / at the limit (each behind `junk`
    random residues, which make it a long subject without reaching the
    query's start).  Everything the test relies on is asserted on the
    oracle's scores: the prefixes' self-scores are the running sums of the
    diagonal, and they lie on the intended side of the limit."""
    d = np.diag(mat).astype(int)
    rng = np.random.default_rng(seed + 1)
    need = limit // int(d[d > 0].min()) + 16
    q = limit_query(mat, min(need, 6000), rich, seed)
    cum = np.cumsum(d[q])
    assert cum[-3] >= limit, "query too short for this limit"
    c = int(np.searchsorted(cum, limit) + 1)          # the first prefix whose self-score reaches the limit
    assert cum[c - 1] >= limit > cum[c - 2]
    q = q[:c + 8]
    ordinary = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(lo, hi + 1, size=n_ordinary)]

    def planted(n):
        return np.concatenate([rng.integers(0, 25, size=junk).astype(np.uint8), q[:n]])
    sets = {"below": ordinary + [planted(c - 1), planted(c - 2), planted(c - 3)],
            "at": ordinary + [planted(c), planted(c + 1)]}
    out = {}
    for name, subs in sets.items():
        res, offs = pack(subs)
        want = oracle.scan(q, res, offs, mat=mat, gap_open=go, gap_extend=ge)
        k = n_ordinary
        if name == "below":
            assert want[k:].tolist() == [cum[c - 2], cum[c - 3], cum[c - 4]]   # the running sums
            assert want.max() < limit
        else:
            assert want[k:].tolist() == [cum[c - 1], cum[c]] and want[k:].min() >= limit
            assert not k or want[:k].max() < limit
        out[name] = (res, offs, want)
    return q, c, out


def flagged(capfd):
    m = RESCUE.findall(capfd.readouterr().err)
    assert m, "no rescue: line"
    return dict(zip(("inter", "inter_again", "intra", "intra_again"), map(int, m[-1])))


# the scorings whose 16-bit forms run: (matrix, open, extend, fits 20 rows per lane)
LIMIT_SCORINGS = {"asym-12-1": ("asym", 12, 1, True), "b50-2-2": ("b50", 2, 2, True),
                  "big-ge-191-30": ("b62", 191, 30, False), "big-linear-35": ("b50", 35, 35, False),
                  "int8-fits-27": ("d100", 27, 27, False), "int8-over-28": ("d100", 28, 28, False),
                  "big-go-974-1": ("b62", 974, 1, False)}


@pytest.mark.parametrize("scname", list(LIMIT_SCORINGS))
def test_fp16_inter_limit(env, sw, oracle, handle, knobs, capfd, scname):
    """sat_limit = 4096 - 28 ge - 2 max(max S, 1) of the inter fp16 cell."""
    mk, go, ge, _ = LIMIT_SCORINGS[scname]
    m = env.mats[mk]
    limit = 4096 - 28 * ge - 2 * max(int(m.max()), 1)
    q, c, sets = edge_sets(oracle, m, go, ge, limit, False, 300, 20, 200)
    knobs(rescue_stats=1, inter_i16_span=0)
    for name, (res, offs, want) in sets.items():
        db = sw.Database(handle, res, offs, long_threshold=100000)
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        f = flagged(capfd)
        k = handle.last_kernel()
        with capfd.disabled():
            print("LIMIT %s | fp16 inter %s | limit %d prefix %d | %s | %s" % (scname, name, limit, c, k, f))
        db.close()
        assert k.endswith(",fp16>"), k
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0], got[-3:], want[-3:])
        assert (f["inter"] == 0) if name == "below" else (f["inter"] >= 1), (name, f)


@pytest.mark.parametrize("ri", [4, 20])
@pytest.mark.parametrize("scname", list(LIMIT_SCORINGS))
def test_fp16_intra_limit(env, sw, oracle, handle, knobs, capfd, scname, ri):
    """sat_limit = 4096 - (intra_bias_rows(ri) + 2) ge - 2 max(max S, 1) of
    the two-subjects fp16 cell at 4 and at 20 rows per lane (where the
    scoring does not admit 20 rows the plan runs a narrower form: its own
    limit is the one checked)."""
    mk, go, ge, wide = LIMIT_SCORINGS[scname]
    m = env.mats[mk]
    knobs(rescue_stats=1, intra_x2_rows=ri, intra_i16_first=0)
    # the rows the plan runs: the forced ones, or (20 not admitted) the cost
    # model's 4..16, which all have the bias of 16
    limit = 4096 - (bias_rows(ri if (ri != 20 or wide) else 16) + 2) * ge - 2 * max(int(m.max()), 1)
    assert bias_rows(4) == bias_rows(16) == 26 and bias_rows(20) == 38
    q, c, sets = edge_sets(oracle, m, go, ge, limit, False, 400 + ri, 70, 200)
    for name, (res, offs, want) in sets.items():
        # (under the diagonal-100 matrix the edge is a prefix of 32 residues)
        db = sw.Database(handle, res, offs, long_threshold=min(64, c - 4))
        assert db.stats()["n_blocks"] == 0
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        f = flagged(capfd)
        ik = handle.last_intra_kernel()
        with capfd.disabled():
            print("LIMIT %s | fp16 intra %s rows %d | limit %d prefix %d | %s | %s" % (scname, name, ri, limit, c, ik, f))
        db.close()
        assert ik.startswith("sw_intra_x2<") and (ik == "sw_intra_x2<%d>" % ri) == (ri != 20 or wide), ik
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0], got[-3:], want[-3:])
        assert (f["intra"] == 0) if name == "below" else (f["intra"] >= 1), (name, f)


@pytest.mark.parametrize("scname", list(LIMIT_SCORINGS))
def test_int16_inter_limit(env, sw, oracle, handle, knobs, capfd, scname):
    """kSat16 = 32767 - 1152 of the int16 two-strips kernel, run first
    (inter_variant y32x8: what it flags is the line's "flagged" count, and
    the int32 kernel re-scores it)."""
    mk, go, ge, _ = LIMIT_SCORINGS[scname]
    m = env.mats[mk]
    q, c, sets = edge_sets(oracle, m, go, ge, K_SAT16, True, 500, 20, 200)
    knobs(rescue_stats=1, inter_variant="y32x8", inter_i16_span=0)
    for name, (res, offs, want) in sets.items():
        db = sw.Database(handle, res, offs, long_threshold=100000)
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        f = flagged(capfd)
        k = handle.last_kernel()
        with capfd.disabled():
            print("LIMIT %s | int16 inter %s | limit %d prefix %d | %s | %s" % (scname, name, K_SAT16, c, k, f))
        db.close()
        assert base(k) == inter_name("linear" if go == ge and int(m.max()) + go <= 127 else "affine", True, "y32x8"), k
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0], got[-3:], want[-3:])
        assert (f["inter"] == 0) if name == "below" else (f["inter"] >= 1), (name, f)


@pytest.mark.parametrize("scname", list(LIMIT_SCORINGS))
def test_int16_intra_limit(env, sw, oracle, handle, knobs, capfd, scname):
    """kSat16 - intra_bias_rows(ri) ge of the two-subjects int16 form, run
    first (intra_i16_first 1): what it flags is the line's "again" count."""
    mk, go, ge, _ = LIMIT_SCORINGS[scname]
    m = env.mats[mk]
    limit = K_SAT16 - bias_rows(8) * ge
    q, c, sets = edge_sets(oracle, m, go, ge, limit, True, 600, 70, 200)
    knobs(rescue_stats=1, intra_i16_first=1, intra_x2_rows=8)
    for name, (res, offs, want) in sets.items():
        db = sw.Database(handle, res, offs, long_threshold=64)
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        f = flagged(capfd)
        ik = handle.last_intra_kernel()
        with capfd.disabled():
            print("LIMIT %s | int16 intra %s | limit %d prefix %d | %s | %s" % (scname, name, limit, c, ik, f))
        db.close()
        assert ik == "sw_intra_x2<8,int16>", ik
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0], got[-3:], want[-3:])
        assert f["intra"] == 0, f
        assert (f["intra_again"] == 0) if name == "below" else (f["intra_again"] >= 1), (name, f)


def test_fp16_limits_merged_drain(env, sw, oracle, handle, knobs, capfd):
    """Both fp16 limits (the same number at up to 16 rows per lane) once
    through the merged launch, which drains what it flags itself: prefixes
    among the inter blocks, and behind 300 random residues among the long
    subjects."""
    mk, go, ge = "asym", 12, 1
    m = env.mats[mk]
    limit = 4096 - 28 * ge - 2 * int(m.max())
    q, c, inter = edge_sets(oracle, m, go, ge, limit, False, 700, 20, 200)
    q2, c2, intra = edge_sets(oracle, m, go, ge, limit, False, 700, 20, 200, n_ordinary=0, junk=300)
    assert np.array_equal(q, q2) and c == c2
    thr = c + 50   # the bare prefixes are inter subjects, the ones behind 300 residues long ones
    rng = np.random.default_rng(9)
    longs = [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(thr + 10, thr + 300, size=9)]
    lres, loffs = pack(longs)
    wl = oracle.scan(q, lres, loffs, mat=m, gap_open=go, gap_extend=ge)
    assert wl.max() < limit
    knobs(rescue_stats=1, lpt=1, pair_width=64, inter_i16_span=0, intra_i16_first=0)
    for name in ("below", "at"):
        res = np.concatenate([inter[name][0], lres, intra[name][0]])
        offs = np.concatenate([inter[name][1], inter[name][1][-1] + loffs[1:], inter[name][1][-1] + loffs[-1] + intra[name][1][1:]])
        want = np.concatenate([inter[name][2], wl, intra[name][2]])
        db = sw.Database(handle, res, offs, long_threshold=thr)
        assert db.stats()["n_long"] == len(longs) + (3 if name == "below" else 2)
        capfd.readouterr()
        got = db.scan(q, m, go, ge)
        f = flagged(capfd)
        k = handle.last_kernel()
        with capfd.disabled():
            print("LIMIT asym-12-1 | merged drain %s | limit %d prefix %d | %s | %s | %s" % (name, limit, c, k,
                                                                                      handle.last_intra_kernel(), f))
        db.close()
        assert k.endswith("+lpt+drain"), k
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0])
        if name == "below":
            assert f["inter"] == 0 and f["intra"] == 0 and f["inter_again"] == 0 and f["intra_again"] == 0, f
        else:
            assert f["inter"] >= 1 and f["intra"] >= 1, f
