"""GPU: gap runs across every row and column seam of every scan kernel, bit
for bit against the CPU oracle.

The subjects are the seam probes of tests/seam_support.py (its docstring has
the probes, the windows and the table of seam rows per kernel form): copies of
one 568-residue query with 1 .. 70 rows deleted, or 1 .. 70 columns inserted,
so that the OPTIMAL alignment's gap run starts before, lies across and ends
behind each seam -- the 16-row row groups, the strips' delay line, the pass
boundary in HBM, the short last pass's strip edge, the wave groups' LDS
rings, the int32 and cooperative strips, the wavefront kernels' lanes and
chunks, every column mod 64.  tests/test_seam_probes.py proves on the CPU that
a carry dropped or off by one extension at any of those rows or columns
changes some probe's score; here every kernel form scans the same subjects.

One database (about 2,000 subjects: probes, long twins, 60 random controls) in
three layouts: "split" (long threshold 700: probes on the inter kernels, twins
on the wavefront kernels), "long" (64: everything on the wavefront kernels),
"inter" (everything on the inter kernels; rescue chains only).  The oracle's
scores are computed once per (scoring, query).  Every case asserts the kernel
names it meant to run, and (sw_opts rescue_stats) that no block or subject
was flagged: the form's own kernel scored every probe.  The rescue cases run
the same probes under the matrix and gaps scaled by 9 (BLOSUM62 108/9) and 6
(BLOSUM50 linear 12) -- the same alignments, scores x k -- so that every copy
passes the fp16 guard, and with the 900-residue query the twins pass the
int16 guard too; they assert the flagged counts of each stage.

No tolerance anywhere: every comparison is np.array_equal or ==."""
import re

import numpy as np
import pytest

import seam_support as ss
from pssm_support import derived

pytestmark = pytest.mark.gpu

K_SAT16 = 32767 - 1152
RESCUE = re.compile(r"rescue: qlen \d+ go \d+ ge \d+: inter (-?\d+)/\d+ blocks flagged .*?, (-?\d+) again; "
                    r"pairs \d+; intra (-?\d+)/\d+ flagged, (-?\d+) again")
THRESHOLDS = {"split": ss.SPLIT_THRESHOLD, "long": 64, "inter": 100000}


class Env:
    pass


@pytest.fixture(scope="module")
def env(sw, oracle, handle):
    e = Env()
    e.P = P = ss.build()
    e.mats = {mid: sw.capi.builtin_matrix(mid) for mid in (0, 1)}
    for mid, m in e.mats.items():
        assert np.array_equal(m, oracle.matrix(mid))
    e.queries = {ss.QLEN: P.q, 500: P.q[:500], ss.Q2LEN: P.q2}
    e.db = {k: sw.Database(handle, P.res, P.offs, long_threshold=t) for k, t in THRESHOLDS.items()}
    st = {k: d.stats() for k, d in e.db.items()}
    kinds = np.array([m[3] for m in P.meta])
    assert st["split"]["n_long"] == int((kinds == "twin").sum()) and st["split"]["n_blocks"] >= 20
    assert st["long"]["n_blocks"] == 0 and st["inter"]["n_long"] == 0
    cache = {}

    def matrix(mid, k=1):
        return np.ascontiguousarray(e.mats[mid].astype(np.int64) * k, dtype=np.int8)

    def want(mid, k, go, ge, qlen):
        key = (mid, k, go, ge, qlen)
        if key not in cache:
            cache[key] = oracle.scan(e.queries[qlen], P.res, P.offs, mat=matrix(mid, k), gap_open=go, gap_extend=ge)
            cache[key].setflags(write=False)
        return cache[key]

    e.matrix, e.want = matrix, want
    yield e
    for d in e.db.values():
        d.close()


def differing(P, got, want):
    """The first differing subjects as (axis, p or c, L, kind, got, want)."""
    bad = np.nonzero(got != want)[0]
    return len(bad), [P.meta[k][:4] + (int(got[k]), int(want[k])) for k in bad[:12]]


def flagged(capfd):
    m = RESCUE.findall(capfd.readouterr().err)
    assert m, "no rescue: line"
    return dict(zip(("inter", "inter_again", "intra", "intra_again"), map(int, m[-1])))


def check_names(form, affine, k, ik, st):
    """The kernels a form means to run (sw_last_kernel / sw_last_intra_kernel)."""
    gap = "affine" if affine else "linear"
    layout = ss.FORMS[form][0]
    base, _, suffix = k.partition(">")
    base += ">"
    if layout == "long":
        want_ik = {"intra-4": "sw_intra_x2<4>", "intra-8": "sw_intra_x2<8>", "intra-16": "sw_intra_x2<16>",
                   "intra-20": "sw_intra_x2<20>", "intra-int16": "sw_intra_x2<8,int16>"}.get(form)
        if want_ik:
            assert ik == want_ik, ik
        else:
            assert ik.startswith("sw_intra<") and ik.endswith(",%s>" % gap), ik
        return
    if form.startswith("lpt"):
        rows96 = not affine and form != "lpt-rows64"
        assert base == "sw_inter_x2p<%d,8,%s,fp16>" % (48 if rows96 else 32, gap), k
        assert "+lpt" in suffix, k
        assert ("+tri" in suffix) == (form == "lpt-tris" and affine), k
        assert ("+tail8" in suffix) == (form == "lpt-tail"), k
        assert ik == ("sw_intra_x2<8>" if form == "lpt-persist" else "sw_intra_x2<4>"), ik
        # every block by wave groups, or (pair width 600) the few widest
        if ss.FORMS[form][3]["pair_width"] == 16:
            assert st["pair_blocks"] == st["n_blocks"], st
        else:
            assert 0 < st["pair_blocks"] < st["n_blocks"] // 2, st
        return
    assert suffix == "", k
    assert ik.startswith("sw_intra_x2<"), ik
    if form == "single":
        assert base == "sw_inter_x2s<32,8,%s,fp16>" % gap, k
    elif form.startswith("pairs"):
        assert base == "sw_inter_x2p<32,8,%s,fp16>" % gap and st["pair_blocks"] == st["n_blocks"], (k, st)
    elif form == "y32x8":
        assert base == "sw_inter_x2s<32,8,%s>" % gap, k
    elif form == "f32x4":
        assert base == "sw_inter_x2s<32,4,affine,fp16>", k
    elif form == "64x8":
        assert base == "sw_inter<64,8,%s>" % gap, k
    else:
        assert base == "sw_inter<32,8,%s>" % gap, k
        assert (st["coop_blocks"] > 0) == form.startswith("coop"), (form, st["coop_blocks"])


CASES = [(form, sc) for form, f in ss.FORMS.items() for sc in ss.SCORINGS
         if ("a" if sc[1] != sc[2] else "l") in f[2]]


@pytest.mark.parametrize("form,scoring", CASES, ids=["%s-%d-%d-%d" % ((f,) + s) for f, s in CASES])
def test_seam_probes(env, handle, knobs, capfd, form, scoring):
    mid, go, ge = scoring
    layout, qlen, _, opts, _ = ss.FORMS[form]
    m = env.matrix(mid)
    want = env.want(mid, 1, go, ge, qlen)
    # below every fp16 guard limit (the lowest: 20 rows per lane)
    assert want.max() < 4096 - (38 + 2) * ge - 2 * int(m.max()), want.max()
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1)
    knobs(**opts)
    db = env.db[layout]
    capfd.readouterr()
    got = db.scan(env.queries[qlen], m, go, ge)
    f = flagged(capfd)
    k, ik = handle.last_kernel(), handle.last_intra_kernel()
    check_names(form, go != ge, k, ik, db.stats())
    assert np.array_equal(got, want), (form, scoring, k, ik) + differing(env.P, got, want)
    assert not any(f.values()), (form, scoring, f)


@pytest.mark.parametrize("stage", ["int16", "int32"])
@pytest.mark.parametrize("layout", ["inter", "long", "split"])
@pytest.mark.parametrize("scoring", ss.RESCUE_SCORINGS, ids=["b62x9-108-9", "b50x6-12-12"])
def test_seam_probes_rescued(env, handle, knobs, capfd, scoring, layout, stage):
    """The rescue chains' own strips and lanes under the same probes: the
    separate rescue launches on the inter and the long layout (lpt 0), the
    merged launch's drain on the split one (lpt 1).  With the 568-residue
    query every copy passes the fp16 guard and stays under the int16 one
    (stage int16 re-scores it); with the 900-residue query the twins, copies
    of its whole length, pass the int16 guard too (stage int32)."""
    mid, k, go, ge = scoring
    qlen = ss.QLEN if stage == "int16" else ss.Q2LEN
    m = env.matrix(mid, k)
    want = env.want(mid, k, go, ge, qlen)
    kinds = np.array([x[3] for x in env.P.meta])
    copies, twins = want[kinds != "random"], want[kinds == "twin"]
    # the same alignments as under the unscaled scoring, scores x k
    assert np.array_equal(want, k * env.want(mid, 1, go // k, ge // k, qlen))
    # the fp16 limits' highest is 4096 - 28 ge - 2 max S; the int16 forms' lowest kSat16 - 38 ge
    assert copies.min() >= 4096
    if stage == "int16":
        assert copies.max() < K_SAT16 - 38 * ge
    else:
        assert twins.min() >= K_SAT16 and want[kinds == "probe"].max() < K_SAT16 - 38 * ge
    knobs(inter_i16_span=0, intra_i16_first=0, rescue_stats=1, pair_width=64, quad_width=0, tri_width=0,
          tail_pairs=0, intra_x2_rows=4, lpt=1 if layout == "split" else 0)
    db = env.db[layout]
    capfd.readouterr()
    got = db.scan(env.queries[qlen], m, go, ge)
    f = flagged(capfd)
    name, ik = handle.last_kernel(), handle.last_intra_kernel()
    assert np.array_equal(got, want), (scoring, layout, stage, name, ik, f) + differing(env.P, got, want)
    st = db.stats()
    if layout != "long":
        assert name.startswith("sw_inter_x2p<") and ",fp16>" in name, name
        assert name.endswith("+lpt+drain") == (layout == "split"), name
        # every block that holds a copy (the subjects are packed longest first, 64 to a block,
        # the 400-residue controls last)
        n_inter = int((kinds == "probe").sum() + (layout == "inter") * (kinds == "twin").sum())
        assert (n_inter + 63) // 64 <= f["inter"] <= st["n_blocks"], (f, st["n_blocks"])
    if layout != "inter":
        assert ik == "sw_intra_x2<4>", ik
        assert f["intra"] >= len(twins), f
    if stage == "int16":
        assert f["inter_again"] == 0 and f["intra_again"] == 0, f
    elif layout == "inter":
        assert f["inter_again"] >= 1, f
    else:
        assert f["intra_again"] >= len(twins), f


@pytest.mark.parametrize("scoring", [ss.SCORINGS[0], ss.SCORINGS[2]])
def test_batch_default_plan(env, handle, knobs, scoring):
    """sw_scan_batch of two queries under the library's own plan (the first
    query's deferred tail and boundary rows beside the second's passes)."""
    mid, go, ge = scoring
    knobs(inter_i16_span=0, intra_i16_first=0)
    out = env.db["split"].scan_batch([env.queries[ss.QLEN], env.queries[500]], env.matrix(mid), go, ge)
    name = handle.last_kernel()
    # (the last scan's: 500 rows, where the plan's 8 rows per lane admit the merged launch under
    # both gap models; linear: its 96-row passes)
    assert name.startswith("sw_inter_x2p<32,8,affine,fp16>" if go != ge else "sw_inter_x2p<48,8,linear,fp16>"), name
    assert "+lpt" in name, name
    for j, qlen in enumerate((ss.QLEN, 500)):
        want = env.want(mid, 1, go, ge, qlen)
        assert np.array_equal(out[j], want), (scoring, qlen, name) + differing(env.P, out[j], want)


@pytest.mark.parametrize("scoring", ss.SCORINGS)
def test_score_pair_across_256(env, handle, scoring):
    """sw_score_pair on the probes whose run starts on, or ends on, seam 256."""
    mid, go, ge = scoring
    want = env.want(mid, 1, go, ge, ss.QLEN)
    picked = [j for j, (axis, p, L, kind) in enumerate(env.P.meta)
              if kind == "probe" and axis == "r" and (p == 256 or p + L - 1 == 256)]
    assert len(picked) >= 10
    for j in picked:
        got = handle.score_pair(env.P.q, env.P.subs[j], env.matrix(mid), go, ge)
        assert got == want[j], (scoring, env.P.meta[j], got, int(want[j]))


@pytest.mark.parametrize("scoring", [ss.SCORINGS[1], ss.SCORINGS[3]])
def test_pssm_default_plan(env, sw, handle, knobs, scoring):
    """sw_scan_pssm with the table derived from the query: the same kernels
    behind the other profile builder."""
    mid, go, ge = scoring
    knobs(inter_i16_span=0, intra_i16_first=0)
    db = env.db["split"]
    want = env.want(mid, 1, go, ge, ss.QLEN)
    seq = db.scan(env.P.q, env.matrix(mid), go, ge)
    names = (handle.last_kernel(), handle.last_intra_kernel())
    pssm = sw.Pssm(handle, derived(env.P.q, env.matrix(mid)))
    try:
        got = db.scan_pssm(pssm, go, ge)
        assert (handle.last_kernel(), handle.last_intra_kernel()) == names, names
    finally:
        pssm.close()
    assert names[0].startswith("sw_inter_x2p<32,8,") and names[1].startswith("sw_intra_x2<"), names
    assert np.array_equal(seq, want), (scoring, names) + differing(env.P, seq, want)
    assert np.array_equal(got, want), (scoring, names) + differing(env.P, got, want)
