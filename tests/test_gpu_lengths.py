"""GPU: every kernel family on subjects and queries past 2^15 and 2^16, bit for
bit against the CPU oracle.

The inputs are tests/length_support.py's (its docstring has the pieces and
where they lie): G, seven giants of 32,760 .. 70,001 residues among 57 fillers,
whose scores depend on their last columns being scanned in their places; four
queries of 32,760 .. 65,544 rows, each with a database S(n) of 120 short
subjects planted from the rows across 2^15, across 2^16 and the last 600; T, a
35,213-row query against itself and a mutated copy (scores past fp16 and
int16).  tests/test_length_inputs.py shows on the CPU that a count or an index
that is cut at, or wraps at, either power changes those scores.

G in five layouts: "lanes" (long threshold 100,000: one 64-lane block 70,016
columns wide, every inter form on the giants), "long" (1: every subject on
the wavefront kernels), "own" (the library's threshold,
64), "split" (3,000: the giants on the wavefront kernels, the fillers in a
block), "mixed" (65,540: the giants of 65,544 and 70,001 long, the others in a
block exactly 2^16 columns wide, so that the merged launch's quads and tris,
which need long subjects beside the blocks, run on giants too).  Each form of
tests/seam_support.py's FORMS runs in its own layout and, the inter forms, on
"lanes" (the merged forms on "mixed").  The default plans assert the names
tests/native/length_check.cpp printed on the CPU (length_support.NAMES).

No tolerance anywhere: every comparison is np.array_equal or == on integers,
whole rows or whole alignments."""
import re
import time

import numpy as np
import pytest

import calib_support as cs
import length_support as ls
import rank_support as rs
import seam_support as ss
from conftest import path_score
from pssm_support import derived

pytestmark = pytest.mark.gpu

RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; "
                    r"pairs \d+; intra (-?\d+)/\d+ flagged, (-?\d+) again")
G_LAYOUTS = dict(ls.LAYOUTS, mixed=65540)
SC = dict(zip(ls.SCORING_NAMES, ls.SCORINGS))
FILL = -7


class Env:
    pass


@pytest.fixture(scope="module")
def env(sw, oracle, handle):
    e = Env()
    e.t0 = time.perf_counter()
    e.G = G = ls.giants()
    e.mats = {mid: sw.capi.builtin_matrix(mid) for mid in (0, 1)}
    for mid, m in e.mats.items():
        assert np.array_equal(m, oracle.matrix(mid))
    e.queries = {568: G.q, 500: G.q[:500], 900: G.q900, 1300: G.q1300, 600: G.q600}
    e.db = {k: sw.Database(handle, G.res, G.offs, long_threshold=t) for k, t in G_LAYOUTS.items()}
    e.lens = np.array([len(s) for s in G.subs], dtype=np.int64)
    st = {k: d.stats() for k, d in e.db.items()}
    assert st["lanes"]["n_long"] == 0 and st["lanes"]["n_blocks"] == 1
    assert st["long"]["n_long"] == 64 and st["long"]["n_blocks"] == 0 and st["split"]["n_long"] == 7 and st["mixed"]["n_long"] == 2
    assert 7 < st["own"]["n_long"] < 64 and st["own"]["n_blocks"] == 1
    assert st["lanes"]["max_length"] == 70001

    def want(qlen, mid, go, ge, k=1):
        return ls.scan(oracle, "q%d-G" % qlen, e.queries[qlen], G, ls.scaled(e.mats[mid], k), go, ge)

    e.want = want
    e.long_dbs = {}
    yield e
    # (the module's oracle time, memoised: DESIGN.md §3 has the figure)
    print("LENGTH oracle %.1f s of %.1f s" % (ls.oracle_seconds(), time.perf_counter() - e.t0))
    for d in list(e.db.values()) + [d for dbs in e.long_dbs.values() for d in dbs.values()]:
        d.close()


S_LAYOUTS = {"own": None, "split": 150, "long": 1}


def long_db(env, sw, handle, n, layout):
    """S(n) on the device in one of S_LAYOUTS."""
    if n not in env.long_dbs:
        d = ls.S(n)
        dbs = {k: sw.Database(handle, d.res, d.offs, long_threshold=t) for k, t in S_LAYOUTS.items()}
        env.long_dbs[n] = dbs
        st = {k: x.stats() for k, x in dbs.items()}
        assert st["long"]["n_long"] == ls.N_S and st["long"]["n_blocks"] == 0 and st["own"]["n_long"] == 0
        assert st["split"]["n_long"] >= 20 and st["split"]["n_blocks"] == 2
    return env.long_dbs[n][layout]


def flagged(capfd):
    m = RESCUE.findall(capfd.readouterr().err)
    assert m, "no rescue: line"
    return dict(zip(("inter", "inter_again", "intra", "intra_again"), map(int, m[-1])))


def differing(env, got, want):
    bad = np.nonzero(got != want)[0]
    return len(bad), [(int(k), int(env.lens[k]), int(got[k]), int(want[k])) for k in bad[:12]]


def base_name(form, affine):
    """The inter kernel a form of seam_support.FORMS means to run, without
    what depends on the database's shape."""
    gap = "affine" if affine else "linear"
    return {"single": "sw_inter_x2s<32,8,%s,fp16>" % gap, "y32x8": "sw_inter_x2s<32,8,%s>" % gap,
            "f32x4": "sw_inter_x2s<32,4,affine,fp16>", "64x8": "sw_inter<64,8,%s>" % gap}.get(form, "sw_inter<32,8,%s>" % gap)


def check_names(form, layout, affine, k, ik, st):
    gap = "affine" if affine else "linear"
    if layout == "long":
        want_ik = {"intra-4": "sw_intra_x2<4>", "intra-8": "sw_intra_x2<8>", "intra-16": "sw_intra_x2<16>",
                   "intra-20": "sw_intra_x2<20>", "intra-int16": "sw_intra_x2<8,int16>"}.get(form)
        if want_ik:
            assert ik == want_ik, ik
        else:
            assert ik.startswith("sw_intra<") and ik.endswith(",%s>" % gap), ik
        return
    base, _, suffix = k.partition(">")
    base += ">"
    assert (ik == "none") == (layout == "lanes"), ik
    if form.startswith("lpt"):
        merged = layout != "lanes"       # the merged launch needs long subjects beside the blocks
        rows96 = merged and not affine and form != "lpt-rows64"
        assert base == "sw_inter_x2p<%d,8,%s,fp16>" % (48 if rows96 else 32, gap), k
        assert ("+lpt" in suffix) == merged, k
        assert ("+tri" in suffix) == (merged and form == "lpt-tris" and affine), k
        if merged:
            assert ik == ("sw_intra_x2<8>" if form == "lpt-persist" else "sw_intra_x2<4>"), ik
        return
    assert suffix == "", k
    if form.startswith("pairs"):
        assert base == "sw_inter_x2p<32,8,%s,fp16>" % gap and st["pair_blocks"] == st["n_blocks"] == 1, (k, st)
    else:
        assert base == base_name(form, affine), k
        if base.startswith("sw_inter<32,"):
            assert (st["coop_blocks"] > 0) == form.startswith("coop"), (form, st["coop_blocks"])


def form_cases():
    out = []
    for form, f in ss.FORMS.items():
        for sname, sc in SC.items():
            if ("a" if sc[1] != sc[2] else "l") not in f[2]:
                continue
            out.append((form, f[0], sname))
            if f[0] == "split":
                out.append((form, "mixed" if form.startswith("lpt") else "lanes", sname))
                if form.startswith("lpt") and form in ("lpt-singles", "lpt-quads"):
                    out.append((form, "lanes", sname))
    return out


FORM_CASES = form_cases()


@pytest.mark.parametrize("form,layout,sname", FORM_CASES, ids=["%s-%s-%s" % c for c in FORM_CASES])
def test_scan_forms(env, handle, knobs, capfd, form, layout, sname):
    """Every form of seam_support.FORMS on G: in its own layout ("split": the
    giants on the wavefront kernels beside the fillers' block; "long"), and
    the inter forms with the giants in a block ("lanes" 70,016 columns wide;
    the merged forms on "mixed", a block 2^16 columns wide)."""
    mid, go, ge = SC[sname]
    _, qlen, _, opts, _ = ss.FORMS[form]
    m = env.mats[mid]
    want = env.want(qlen, mid, go, ge)
    assert want.max() < 4096 - (38 + 2) * ge - 2 * int(m.max()), want.max()
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    knobs(**opts)
    db = env.db[layout]
    capfd.readouterr()
    t0 = time.perf_counter()
    got = db.scan(env.queries[qlen], m, go, ge)
    dt = time.perf_counter() - t0
    f = flagged(capfd)
    k, ik = handle.last_kernel(), handle.last_intra_kernel()
    with capfd.disabled():
        print("LENGTH form %s %s %s | %s | %s | %.3f s" % (form, layout, sname, k, ik, dt))
    check_names(form, layout, go != ge, k, ik, db.stats())
    assert np.array_equal(got, want), (form, layout, sname, k, ik) + differing(env, got, want)
    assert not any(f.values()), (form, layout, sname, f)


DEFAULTS = [(lay, s, q) for lay in ("lanes", "long", "own", "split", "split-merged") for s in ls.SCORING_NAMES
            for q in (568, 1300)]


@pytest.mark.parametrize("layout,sname,qlen", DEFAULTS, ids=["%s-%s-q%d" % c for c in DEFAULTS])
def test_default_plan(env, handle, knobs, capfd, layout, sname, qlen):
    """The library's own plan (and the merged profile on the split): the names
    length_check printed from scan_plan on the CPU, and the flagged counts the
    guards predict.  The adaptive int16-first routes are switched off
    (inter_i16_span 0, intra_i16_first 0), which is what a database's first
    scan runs and keeps the counts a function of the scores; the hit table,
    sw_align and save / load cases below run under the handle's own options,
    adaptive routes included."""
    mid, go, ge = SC[sname]
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    if layout == "split-merged":
        knobs(**ls.MERGED)
    db = env.db[layout.split("-")[0]]
    want = env.want(qlen, mid, go, ge)
    capfd.readouterr()
    got = db.scan(env.queries[qlen], env.mats[mid], go, ge)
    f = flagged(capfd)
    names = (handle.last_kernel(), handle.last_intra_kernel())
    expect = ls.NAMES[layout, sname, qlen]
    # (without inter blocks the handle keeps an earlier scan's inter name)
    assert names[1] == expect[1] and (expect[0] is None or names[0] == expect[0]), (names, expect)
    assert np.array_equal(got, want), (layout, sname, qlen, names) + differing(env, got, want)
    # the 568-row query's pieces stay below every guard; the 1,300-row query's (897 columns) pass the fp16 one
    ri = int(re.match(r"sw_intra_x2<(\d+)>", names[1]).group(1)) if names[1] != "none" else 4
    p = predicted(env.lens, want, G_LAYOUTS[layout.split("-")[0]] or 64, env.mats[mid], ge, ri)
    assert f == p and any(p.values()) == (qlen == 1300), (f, p)


def bias_rows(ri):
    """The intra cell's bias in gap extensions."""
    return max(26, ri + (16 if ri == 20 else 8) + 2)


def predicted(lens, want, threshold, m, ge, ri):
    """The rescue: line's counts from the oracle's scores and DESIGN.md §4's
    guards: an inter block (64 subjects, longest first, stable) is flagged by
    the fp16 form when a lane's score reaches 4096 - 28 ge - 2 max S, and
    again by the int16 form from kSat16 on; a long subject from 4096 -
    (intra_bias_rows + 2) ge - 2 max S, and again from kSat16 - intra_bias_rows
    ge."""
    order = np.argsort(-lens, kind="stable")
    is_long = lens[order] > threshold
    longs, shorts = order[is_long], order[~is_long]
    max_s = max(int(m.max()), 1)
    blocks = [shorts[b:b + 64] for b in range(0, len(shorts), 64)]
    return {"inter": sum(bool((want[b] >= 4096 - 28 * ge - 2 * max_s).any()) for b in blocks),
            "inter_again": sum(bool((want[b] >= ls.K_SAT16).any()) for b in blocks),
            "intra": int((want[longs] >= 4096 - (bias_rows(ri) + 2) * ge - 2 * max_s).sum()),
            "intra_again": int((want[longs] >= ls.K_SAT16 - bias_rows(ri) * ge).sum())}


@pytest.mark.parametrize("stage", ["int16", "int32"])
@pytest.mark.parametrize("variant", ["lanes", "long", "split", "split-drain"])
@pytest.mark.parametrize("scoring", ls.RESCUE_SCORINGS, ids=["b62x9-108-9", "b50x6-12-12"])
def test_rescue_chains(env, handle, knobs, capfd, scoring, variant, stage):
    """The rescue chains on G under the matrix and gaps scaled by 9 and by 6:
    with the 568-row query every giant passes the fp16 guard (stage int16
    re-scores it), with the 900-row one the int16 guard too (stage int32); the
    separate rescue launches (lpt 0) and the merged launch's drain."""
    mid, k, go, ge = scoring
    qlen = 568 if stage == "int16" else 900
    m = ls.scaled(env.mats[mid], k)
    want = env.want(qlen, mid, go, ge, k)
    at = [env.G.giant[L] for L in ls.GIANTS]
    assert want[at].min() >= (4096 if stage == "int16" else ls.K_SAT16)
    layout = variant.split("-")[0]
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1, pair_width=64, quad_width=0, tri_width=0,
          tail_pairs=0, intra_x2_rows=4, lpt=1 if variant == "split-drain" else 0)
    db = env.db[layout]
    capfd.readouterr()
    got = db.scan(env.queries[qlen], m, go, ge)
    f = flagged(capfd)
    name, ik = handle.last_kernel(), handle.last_intra_kernel()
    p = predicted(env.lens, want, G_LAYOUTS[layout], m, ge, 4)
    with capfd.disabled():
        print("LENGTH rescue %s %s %s | %s | %s | counted %s | predicted %s" % (scoring, variant, stage, name, ik, f, p))
    assert np.array_equal(got, want), (scoring, variant, stage, name, ik, f) + differing(env, got, want)
    assert name.endswith("+lpt+drain") == (variant == "split-drain"), name
    if layout != "lanes":
        assert ik == "sw_intra_x2<4>", ik
    assert p["inter" if layout == "lanes" else "intra"] >= 1
    assert f == p, (f, p)


@pytest.mark.parametrize("layout", ["lanes", "long"])
def test_square(env, sw, oracle, handle, knobs, capfd, layout):
    """T: the 35,213-row query against itself and its mutated copy, scores
    near 180,000 and 140,000 under BLOSUM62 11/1 (past fp16's 65,504 and past
    int16), through both chains to the int32 kernels.  The long layout scans
    all of T (1.3 s).  In the lane layout the 64 subjects are one block, which
    one wave group scans three times (fp16, int16, int32): all of T took 33 s
    there (measured once, every score equal to the oracle's, one block flagged
    and flagged again), so that layout scans T cut to 12,000 rows and columns
    (self score past fp16, the copy's past int16)."""
    t = ls.square() if layout == "long" else ls.square_short()
    m = env.mats[1]
    want = ls.scan(oracle, "qT-T" if layout == "long" else "qTs-Ts", t.q, t, m, 11, 1)
    assert want[t.self_at] > 65504 and want[t.copy_at] > 32767
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1, pair_width=16, pair_group=4)
    db = sw.Database(handle, t.res, t.offs, long_threshold=100000 if layout == "lanes" else 1)
    try:
        capfd.readouterr()
        t0 = time.perf_counter()
        got = db.scan(t.q, m, 11, 1)
        dt = time.perf_counter() - t0
        f = flagged(capfd)
        with capfd.disabled():
            print("LENGTH square %s | %s | %s | %s | %.3f s" % (layout, handle.last_kernel(), handle.last_intra_kernel(), f, dt))
        assert np.array_equal(got, want), (layout, int(got[t.self_at]), int(want[t.self_at]), int(got[t.copy_at]))
        if layout == "lanes":
            assert f["inter"] == 1 and f["inter_again"] == 1, f
        else:
            assert f["intra"] == 2 and f["intra_again"] == 2, f
    finally:
        db.close()


# name: (layout, sw_opts overrides, the inter name's start, the intra name's start); layouts of S: "own" (the
# library's threshold leaves every subject in the lanes), "split" (150), "long" (1)
LONG_FORMS = {
    "default": ("own", {}, "sw_inter_x2", "none"),
    "default-split": ("split", {}, "sw_inter_x2", "sw_intra_x2<"),
    "lpt1": ("split", dict(lpt=1, pair_width=16, intra_x2_rows=8), "sw_inter_x2p<", "sw_intra_x2<8>"),
    "int32": ("split", dict(int16_guard=0, inter_variant="32x8", intra_x2=0), "sw_inter<", "sw_intra<"),
    "coop": ("own", dict(lpt=0, inter_variant="32x8", coop_width=16), "sw_inter<32,8,", "none"),
    "long-4": ("long", dict(intra_x2_rows=4), "", "sw_intra_x2<4>"),
    "long-8": ("long", dict(intra_x2_rows=8), "", "sw_intra_x2<8>"),
    "long-20": ("long", dict(intra_x2_rows=20), "", "sw_intra_x2<20>"),
    "long-int32": ("long", dict(intra_x2=0), "", "sw_intra<"),
}
LONG_CASES = [(n, form, s) for n in ls.QLONG for form in LONG_FORMS for s in ls.SCORING_NAMES
              if s == "b62-11-1" or form in ("default", "default-split", "long-8", "int32")]


@pytest.mark.parametrize("n,form,sname", LONG_CASES, ids=["q%d-%s-%s" % c for c in LONG_CASES])
def test_long_queries(env, sw, oracle, handle, knobs, capfd, n, form, sname):
    """A long query against its database S(n), whose best alignments lie in
    the rows across 2^15, across 2^16 and in the last 600."""
    mid, go, ge = SC[sname]
    layout, opts, inter, intra = LONG_FORMS[form]
    q, d, m = ls.long_query(n), ls.S(n), env.mats[mid]
    want = ls.scan(oracle, "q%d-S" % n, q, d, m, go, ge)
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    knobs(**opts)
    db = long_db(env, sw, handle, n, layout)
    capfd.readouterr()
    t0 = time.perf_counter()
    got = db.scan(q, m, go, ge)
    dt = time.perf_counter() - t0
    f = flagged(capfd)
    k, ik = handle.last_kernel(), handle.last_intra_kernel()
    with capfd.disabled():
        print("LENGTH long q%d %s %s | %s | %s | %s | %.3f s" % (n, form, sname, k, ik, f, dt))
    if inter:
        assert k.startswith(inter), k
    assert ik.startswith(intra), ik
    if form == "coop":
        assert db.stats()["coop_blocks"] > 0
    if form == "lpt1":
        assert "+lpt" in k, k
    assert not any(f.values()), f
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (n, form, sname, k, ik, [(int(x), d.meta[x], int(got[x]), int(want[x])) for x in bad[:10]])


def test_long_query_batch(env, sw, oracle, handle, knobs):
    """One batch of (65,544 rows, the empty query, 568 rows) on S(65,544)."""
    n, m = 65544, env.mats[1]
    d = ls.S(n)
    knobs(inter_i16_span=0, intra_i16_first=0)
    db = long_db(env, sw, handle, n, "own")
    out = db.scan_batch([ls.long_query(n), np.zeros(0, np.uint8), env.G.q], m, 11, 1)
    assert np.array_equal(out[0], ls.scan(oracle, "q%d-S" % n, ls.long_query(n), d, m, 11, 1))
    assert not out[1].any()
    assert np.array_equal(out[2], ls.scan(oracle, "q568-S%d" % n, env.G.q, d, m, 11, 1))


@pytest.mark.parametrize("sname", ls.SCORING_NAMES)
def test_score_pair_long_query(env, oracle, handle, sname):
    mid, go, ge = SC[sname]
    n, m = 65544, env.mats[mid]
    d = ls.S(n)
    want = ls.scan(oracle, "q%d-S" % n, ls.long_query(n), d, m, go, ge)
    picked = [k for k, x in enumerate(d.meta) if x and x[0] == "p16"][:2] + [k for k, x in enumerate(d.meta) if x and x[0] == "last"][:1]
    assert len(picked) == 3
    for k in picked:
        assert handle.score_pair(ls.long_query(n), d.subs[k], m, go, ge) == want[k] > 100, (sname, k)
    # ... and a giant against the long query's first 600 rows, subject past 2^16
    s = env.G.subs[env.G.giant[70001]]
    assert handle.score_pair(env.G.q600, s, m, go, ge) == oracle.score(env.G.q600, s, m, go, ge)


def test_pssm_of_the_long_query(env, sw, oracle, handle, knobs):
    """A PSSM derived from the 35,213-row query (rows = matrix[q]): the
    profile build's 2,048-row chunks past row 2^15; its scan equals the
    sequence scan."""
    n, m = 35213, env.mats[1]
    q, d = ls.long_query(n), ls.S(n)
    want = ls.scan(oracle, "q%d-S" % n, q, d, m, 11, 1)
    knobs(inter_i16_span=0, intra_i16_first=0)
    pssm = sw.Pssm(handle, derived(q, m))
    try:
        for layout in ("split", "long"):
            db = long_db(env, sw, handle, n, layout)
            seq = db.scan(q, m, 11, 1)
            names = (handle.last_kernel(), handle.last_intra_kernel())
            got = db.scan_pssm(pssm, 11, 1)
            assert (handle.last_kernel(), handle.last_intra_kernel()) == names, names
            assert np.array_equal(seq, want) and np.array_equal(got, want), (layout, names)
    finally:
        pssm.close()


# ---- the hit table ------------------------------------------------------------
def giant_rows(env, oracle, qlen, sname, which=None):
    """The expected rows of every subject of G (or of the giants `which`)."""
    mid, go, ge = SC[sname]
    ids = range(len(env.G.subs)) if which is None else [env.G.giant[L] for L in which]
    return [ls.row(oracle, "q%d-G%d" % (qlen, k), env.queries[qlen], env.G.subs[k], env.mats[mid], go, ge, k) for k in ids]


@pytest.mark.parametrize("layout,sname", [("lanes", "b62-11-1"), ("long", "b62-11-1"), ("own", "b62-11-1"),
                                          ("own", "b50-2-2")])
def test_hit_rows_of_the_giants(env, oracle, handle, layout, sname):
    """sw_hit_stats, whole rows: every subject of G under the 568-row query
    (two chunks of 512 rows with a boundary row 70,001 columns long)."""
    mid, go, ge = SC[sname]
    want = giant_rows(env, oracle, 568, sname)
    got = env.db[layout].hit_stats(env.G.q, list(range(len(want))), env.mats[mid], go, ge)
    for k, (row, w) in enumerate(zip(got, want)):
        assert row == w, (layout, sname, k, row, w)
    for L in ls.GIANTS:
        w = want[env.G.giant[L]]
        assert w["s_end"] == L - ls.END_PAD - ss.TAIL and w["s_len"] == L and w["gap_opens"] >= 1, w
    assert [w["score"] for w in want] == env.want(568, mid, go, ge).tolist()


def test_hit_rows_three_chunks(env, oracle, handle):
    """The giants of 35,213, 65,536 and 70,001 under the 1,300-row query."""
    which = (35213, 65536, 70001)
    want = giant_rows(env, oracle, 1300, "b62-11-1", which)
    ids = [env.G.giant[L] for L in which]
    for layout in ("lanes", "split"):
        got = env.db[layout].hit_stats(env.G.q1300, ids, env.mats[1], 11, 1)
        assert got == want, (layout, got, want)
    for L, w in zip(which, want):
        assert L - ls.END_PAD - 5 <= w["s_end"] <= L - ls.END_PAD + 5 and w["s_begin"] > min(L, ls.P16) - 1000, w


def top_ids(rows, k):
    return sorted(range(len(rows)), key=lambda i: (-rows[i]["score"], rows[i]["id"]))[:k]


def test_scan_hits_of_the_giants(env, oracle, handle):
    """sw_scan_hits and one sw_scan_batch_hits call on G against the oracle's 25 best."""
    want = giant_rows(env, oracle, 568, "b62-11-1")
    top = [want[i] for i in top_ids(want, 25)]
    assert {r["id"] for r in top[:7]} == {env.G.giant[L] for L in ls.GIANTS}
    db = env.db["own"]
    assert db.scan_hits(env.G.q, 25, env.mats[1], 11, 1) == top
    batch = db.scan_batch_hits([env.G.q, np.zeros(0, np.uint8), env.G.q], 25, env.mats[1], 11, 1)
    assert batch[0] == top and batch[2] == top


def long_rows(env, oracle, n, sname, picked):
    mid, go, ge = SC[sname]
    d = ls.S(n)
    return [ls.row(oracle, "q%d-S%d" % (n, k), ls.long_query(n), d.subs[k], env.mats[mid], go, ge, k) for k in picked]


def picked_of(n, per_region=4):
    d = ls.S(n)
    out = []
    for r in ls.regions(n):
        out += [k for k, x in enumerate(d.meta) if x and x[0] == r][:per_region]
    return out + [k for k, x in enumerate(d.meta) if x is None][:4]


def test_hit_rows_of_the_long_query(env, sw, oracle, handle):
    """S(65,544) under the 65,544-row query: 129 chunks and their boundary
    row's scratch; q_begin past 2^15, q_end past 2^15 and 2^16 (the query has
    8 rows past 2^16).  Rows of 16 subjects, four per region and four fillers:
    the oracle's traceback of a 65,544-row query takes 0.3 s per subject on
    one core, all 120 would take 35 s; sw_scan's scores cover all 120."""
    n = 65544
    picked = picked_of(n)
    want = long_rows(env, oracle, n, "b62-11-1", picked)
    assert sum(w["q_end"] > ls.P16 for w in want) >= 4 and sum(ls.P15 < w["q_begin"] < ls.P16 - 1000 for w in want) >= 2
    for layout in ("split", "long"):
        got = long_db(env, sw, handle, n, layout).hit_stats(ls.long_query(n), picked, env.mats[1], 11, 1)
        for row, w in zip(got, want):
            assert row == w, (layout, row, w)


# ---- the traceback --------------------------------------------------------------
@pytest.mark.parametrize("sname", ls.SCORING_NAMES)
def test_align_on_the_giants(env, oracle, handle, sname):
    """sw_align of the 600-row query on the giants of 35,213, 65,536 and
    70,001 (42 M direction bytes each, diagonals up to 70,601)."""
    mid, go, ge = SC[sname]
    m = env.mats[mid]
    which = (35213, 65536, 70001)
    ids = [env.G.giant[L] for L in which]
    got = env.db["own"].align(env.G.q600, ids, m, go, ge)
    for L, k, al in zip(which, ids, got):
        w = ls.align(oracle, "q600-G%d" % k, env.G.q600, env.G.subs[k], m, go, ge)
        assert al == w, (sname, L, {x: al[x] for x in al if x != "ops"}, {x: w[x] for x in w if x != "ops"})
        assert path_score(env.G.q600, env.G.subs[k], m, go, ge, al) == al["score"], (sname, L)
        assert al["s_end"] == L - ls.END_PAD - ss.TAIL and al["s_begin"] > min(L, ls.P16) - 1100


def test_align_over_the_direction_budget(env, sw, oracle, handle):
    """Three hits of the 32,776-row query in one call: each direction array is
    past the 2^30-byte launch budget, so the call runs three groups of one."""
    n, m = 32776, env.mats[1]
    d, q = ls.S(n), ls.long_query(n)
    picked = [k for k, x in enumerate(d.meta) if x and x[0] == "p15"][:2] + [k for k, x in enumerate(d.meta) if x and x[0] == "last"][:1]
    assert all(ls.align_dirs_bytes(n, len(d.subs[k])) > 1 << 30 for k in picked)
    got = long_db(env, sw, handle, n, "split").align(q, picked, m, 11, 1)
    for k, al in zip(picked, got):
        w = ls.align(oracle, "q%d-S%d" % (n, k), q, d.subs[k], m, 11, 1)
        assert al == w, (k, {x: al[x] for x in al if x != "ops"}, {x: w[x] for x in w if x != "ops"})
        assert al["q_end"] > ls.P15 - 300 and path_score(q, d.subs[k], m, 11, 1, al) == al["score"]


def test_align_past_2_32_direction_bytes(env, sw, oracle, handle):
    """One hit of the 65,544-row query: 4.3 GB of direction bytes, d (qlen + 1) past 2^32."""
    n, m = 65544, env.mats[1]
    d, q = ls.S(n), ls.long_query(n)
    k = [k for k, x in enumerate(d.meta) if x and x[0] == "p16"][0]
    assert ls.align_dirs_bytes(n, len(d.subs[k])) > 1 << 32
    al = long_db(env, sw, handle, n, "split").align(q, [k], m, 11, 1)[0]
    w = ls.align(oracle, "q%d-S%d" % (n, k), q, d.subs[k], m, 11, 1)
    assert al == w, ({x: al[x] for x in al if x != "ops"}, {x: w[x] for x in w if x != "ops"})
    assert al["q_begin"] > ls.P16 - 400 and al["q_end"] > ls.P16 and path_score(q, d.subs[k], m, 11, 1, al) == al["score"]


# ---- around the scan -------------------------------------------------------------
def test_histogram_and_ranking(env, sw, handle, knobs):
    """sw_score_hist and sw_sig_topk_device on G: the giants' length bins (60
    .. 64), an adjustment table of 70,002 entries and one cut at 100."""
    import torch
    knobs(inter_i16_span=0, intra_i16_first=0)
    db = env.db["own"]
    want = env.want(568, 1, 11, 1)
    d = torch.full((db.n_out,), FILL, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    db.scan_device(env.G.q, d.data_ptr(), env.mats[1], 11, 1)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), want)
    H = db.score_hist(d.data_ptr())
    assert np.array_equal(H, cs.table(want, env.lens))
    assert {int(b) for b in cs.length_bin(np.array(ls.GIANTS))} == {59, 60, 63, 64}
    cal = sw.capi.calib_fit(H, 568)
    ids = np.arange(len(env.lens))
    for max_len in (70001, 100):
        adj = sw.capi.sig_rank_table(cal, max_len)
        assert len(adj) == max_len + 1
        r = rs.rank_values(want, env.lens, adj)
        for k in (7, 64, 70):
            keys, count = db.sig_topk(d.data_ptr(), adj, rs.R_FLOOR, k)
            assert count == rs.count(r, rs.R_FLOOR) and np.array_equal(keys, rs.select(rs.keys(r, ids), k)), (max_len, k)


def test_save_and_load(env, sw, handle, knobs, tmp_path):
    knobs(inter_i16_span=0, intra_i16_first=0)
    path = str(tmp_path / "giants.swdb")
    env.db["own"].save(path)
    db = sw.Database.load(handle, path)
    try:
        assert db.stats()["max_length"] == 70001 and db.n == len(env.G.subs)
        for sname, (mid, go, ge) in SC.items():
            assert np.array_equal(db.scan(env.G.q, env.mats[mid], go, ge), env.want(568, mid, go, ge)), sname
        db.set_long_threshold(100000)
        assert np.array_equal(db.scan(env.G.q, env.mats[1], 11, 1), env.want(568, 1, 11, 1))
    finally:
        db.close()


def test_custom_ids_merged(env, sw, oracle, handle, knobs):
    """G with result ids 3 perm(i) + 1 through a merged scan, and its rows."""
    ids = env.G.ids_custom
    knobs(inter_i16_span=0, intra_i16_first=0)
    knobs(**ls.MERGED)
    db = sw.Database(handle, env.G.res, env.G.offs, ids=ids, long_threshold=3000)
    try:
        want = env.want(568, 1, 11, 1)
        got = db.scan(env.G.q, env.mats[1], 11, 1)
        assert "+lpt" in handle.last_kernel(), handle.last_kernel()
        assert np.array_equal(got[ids], want) and int(got.sum()) == int(want.sum())
        rows = giant_rows(env, oracle, 568, "b62-11-1")
        which = [env.G.giant[L] for L in ls.GIANTS]
        assert db.hit_stats(env.G.q, ids[which], env.mats[1], 11, 1) == [dict(rows[k], id=int(ids[k])) for k in which]
    finally:
        db.close()
