"""Seam probes: subjects whose OPTIMAL alignment has a gap run lying across a
chosen row or column seam of the scan kernels' DP matrix.  Shared by
tests/test_seam_probes.py (CPU: what the probes would see of a mis-carried
value, through tests/native/seam_check.cpp) and tests/test_gpu_seams.py (GPU:
every kernel form bit for bit against the oracle on the same subjects).

Every scan kernel cuts the matrix into pieces and hands (H, gap state) from
one piece to the next, each hand-over corrected by a multiple of ge since the
biased cell.  A carry that is off by ge, or dropped and re-opened from H,
changes a score only if the optimal path has a gap run across that seam, which
random subjects and a few fixed indels almost never have (the control of
test_seam_probes.py measures how seldom).

Conventions (0-based).  Row seam r = the step from query row r - 1 to row r
("the seam at 256": row 256 is a pass's first row); column seam c likewise in
the subject.
  row probe (p, L)     q[:p] + q[p + L:]: query rows p .. p + L - 1 stand
                       against gaps.  The run OPENS across seam p (from H of
                       row p - 1) and its gap state F is CARRIED across seams
                       p + 1 .. p + L - 1; row p + L takes the run's end as its
                       diagonal.
  column probe (c, L)  q[:c] + L residues of a separate generator (none equal
                       to q[c - 1] or q[c]) + q[c:]: subject columns c .. c +
                       L - 1 stand against gaps (E).
  long twin            a probe + TAIL residues unrelated to q (they are the
                       rows 568.. of the longer query Q2): over the long
                       threshold of the "split" layout, seams unchanged.
For each seam s of a window and each L: the probes (s, L) and (s - 1, L)
(start on / just before the seam) and (s - L + 1, L) (end on it).  L = 1, 2, 5
(short), 17 (longer than a 16-row group), 40 (longer than a 32-row strip), 70
(longer than a 64-row pass).  Near the query's end the flank behind the gap is
short, so the last window takes L <= 5 for runs that start in it and L <= 17
for runs that end in it (test_seam_probes.py checks that this still sees
every fault at every row).

The query (QLEN = 568) is uniform over the 16 amino acids whose diagonal
entries are the lowest (no C, H, P, W), no residue twice in a row: its copies score about 2,900 under
BLOSUM62 and 3,600 under BLOSUM50, below every fp16 guard limit (3,834 at the
least: 20 rows per lane, extend 6), so a form's own kernel scores them, not a
rescue stage; the GPU test asserts that on the oracle's scores.  568 = 8
passes of 64 rows + 56 (short last pass, strips of 28) = 5 passes of 96 + 88
(short, strips of 44).

Seam rows per form (row_seams(); constants from csrc: the two-strips pass of
R = 64 rows (sw_plan.cpp inter_shape) or 96 (scan_plan lpt_rows, linear merged
launch), strips of R / 2, row groups kRowGroup = 16 (sw_inter_x2.hip), the
short pass's strips of R / 2 - 4 (swplan::short_rows), wave groups G = 2, 4, 3
(x2p_wg: pass p on wave p % G, LDS ring inside a round, HBM between rounds),
int32 strips rescue_rows = 32 affine / 64 linear, kCoopRows = 32, intra lanes
of RI rows and chunks of kLanes * RI = 64 RI, the pipelined pairs' 128-row
chunk per wave of 2 rows per lane (lpt_plan nchp)):

  kind         64-row passes          96-row passes        in a window at
  row-group    16, 48 (mod 64)        16, 32, 64, 80 (96)  256/272/304/320
  strip        32 (mod 64)            48 (mod 96)          288 | 240
  pass (HBM)   0 (mod 64); groups:    0 (mod 96)           256, 320 | 288;
               passes p % G == G - 1                       tris 192, quads96 384
  hand-over    the other pass seams of a group (LDS ring)  320 (G 2, 4), 256 (G 3), 288 (96)
  short-strip  512 + 28 = 540         480 + 44 = 524       540 | 524
  short-group  528, 556               496, 512, 540, 556   528 | 540 (short pass's own groups)
  int32 strip  every 32 (affine, coop) / 64 (linear)       256, 288, 320
  lane         every RI rows (2 in the pipelined form)     every window
  chunk        64 RI: 256 (RI 4), 512 (RI 8); 128 (pipe)   256, 512
At RI 16 and 20 one chunk (1,024 and 1,280 rows) holds the query: the chunk
seam is covered at RI 4 and 8 only.  test_seam_probes.py asserts that every
(form, gap model, kind) has a seam inside a row window.

Columns: insertions start in 72 consecutive columns (160 .. 231) and run up to
70 columns on, so the runs start, cross and end at every residue mod 8, 16, 32
and 64: the sub-group rebase (8, or 4 for f32x4), the 16-column groups, the
wavefront kernels' 32-step boundary flush and 8-step rebase, the ring slots
and group ticks (one per 8 columns).
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "seam_check.cpp")

# (matrix id, open, extend): test_gpu_short_pass.py's four, and an open below
# extend (swplan::cell_range admits it: test_cell_range.py "open-below-extend")
SCORINGS = ((1, 12, 1), (1, 14, 3), (0, 2, 2), (1, 5, 5), (1, 5, 6))
# Rescue chains: matrix and gaps scaled by k, the same optimal alignments with
# scores x k.  (matrix id, k, open, extend), entries within +-100 and
# 2 max S + 27 ge + go < 1024: BLOSUM62 x 9 with 108/9 (549), BLOSUM50 x 6
# with linear 12 (516).
RESCUE_SCORINGS = ((1, 9, 108, 9), (0, 6, 12, 12))

QLEN, Q2LEN = 568, 900
TAIL = Q2LEN - QLEN
LS = (1, 2, 5, 17, 40, 70)
# (first seam, last seam, L of runs that start at the seam, L of runs that end on it)
ROW_WINDOWS = ((190, 194, LS, LS), (238, 326, LS, LS), (382, 386, LS, LS), (510, 546, (1, 2, 5), (1, 2, 5, 17)))
COL_WINDOW = (160, 231)
TWIN_LS = (5, 40)         # the probes that get a long twin
SPLIT_THRESHOLD = 700     # probes (<= 638) inter, twins (>= 860) long
ALPHABET = np.array([0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 18, 19], dtype=np.uint8)  # no C, H, P, W
N_RANDOM = 60             # the control's random 400-residue subjects

FAULTS = ("carry dropped", "carry +ge", "carry -ge", "open dropped", "open +ge", "open -ge")


def gap_state_dominated(go, ge):
    """open <= extend: F[i-1] - ge <= H[i-1] - go in every cell (H >= F), so the
    gap state never wins and a carry that is dropped or ge too low cannot
    change any score: the one exemption of test_seam_probes.py (linear gaps,
    and the open-below-extend scoring, which is the linear gap `open`)."""
    return go <= ge


class Probes:
    pass


_cache = {}


def build():
    """The query, the longer query, and the subjects: row probes, column
    probes, twins, random controls (in that order).  meta[k] = (axis, p, L,
    kind), axis 'r' / 'c', kind 'probe' / 'twin' / 'random'."""
    if "p" in _cache:
        return _cache["p"]
    rng = np.random.default_rng(20260)
    # no residue twice in a row: under linear gaps a run splits for free, so
    # beside a doubled residue it can step round any one seam (rows r - 1 and
    # r alike: gap one, match the other) and no probe could see that seam
    q2 = ALPHABET[np.cumsum(rng.integers(1, len(ALPHABET), size=Q2LEN)) % len(ALPHABET)]
    q = q2[:QLEN]
    ins = np.random.default_rng(4711)
    subs, meta, seen = [], [], set()

    def add(axis, p, L):
        if (axis, p, L) in seen or p < 1:
            return
        seen.add((axis, p, L))
        if axis == "r":
            s = np.concatenate([q[:p], q[p + L:]])
        else:
            # (none of the inserted residues equals a neighbour of the insertion:
            # the run could split at such a residue and step round a seam)
            other = ALPHABET[(ALPHABET != q[p - 1]) & (ALPHABET != q[p])]
            s = np.concatenate([q[:p], other[ins.integers(0, len(other), size=L)], q[p:]])
        subs.append(s)
        meta.append((axis, p, L, "probe"))

    for lo, hi, l_start, l_end in ROW_WINDOWS:
        for L in l_start:
            for s in range(lo - 1, hi + 1):
                add("r", s, L)
        for L in l_end:
            for s in range(lo, hi + 1):
                add("r", s - L + 1, L)
    lo, hi = COL_WINDOW
    for L in LS:
        for s in range(lo - 1, hi + 1):
            add("c", s, L)
        for s in range(lo, hi + 1):
            add("c", s - L + 1, L)
    n_probes = len(subs)
    for k in range(n_probes):
        axis, p, L, _ = meta[k]
        if L in TWIN_LS:
            subs.append(np.concatenate([subs[k], q2[QLEN:]]))
            meta.append((axis, p, L, "twin"))
    rnd = np.random.default_rng(99)
    for _ in range(N_RANDOM):
        subs.append(ALPHABET[rnd.integers(0, len(ALPHABET), size=400)])
        meta.append(("-", 0, 0, "random"))
    P = Probes()
    P.q, P.q2, P.subs, P.meta, P.n_probes = q, q2, subs, meta, n_probes
    P.res = np.concatenate(subs).astype(np.uint8)
    P.offs = np.zeros(len(subs) + 1, dtype=np.int64)
    P.offs[1:] = np.cumsum([len(s) for s in subs])
    for a in (P.q, P.q2, P.res, P.offs):
        a.setflags(write=False)
    _cache["p"] = P
    return P


def candidates(meta, axis, seam, fault, linear):
    """Indices of the probes whose gap run lies across `seam` for this fault,
    most direct first: a carry fault needs the run on both sides of the seam
    (p < seam <= p + L - 1); an opening fault the run's first cell behind it
    (p == seam), or under a gap state that H - go dominates any cell of the
    run (every step of the run re-opens from H)."""
    out = []
    for k, (ax, p, L, kind) in enumerate(meta):
        if ax != axis or kind != "probe":
            continue
        if fault < 3 or linear:
            inside = p < seam <= p + L - 1 if fault < 3 else p <= seam <= p + L - 1
            if inside:
                out.append((abs(seam - p - L // 2), L, k))
        elif p == seam:
            out.append((0, L, k))
    return [k for _, _, k in sorted(out)]


# ---- the seam table -----------------------------------------------------------
def short_rows(qlen, rows):
    """swplan::short_rows and the last pass's first row."""
    s0 = (qlen - 1) // rows * rows
    left = qlen - s0
    return (rows // 2 - 4 if (left + 1) // 2 <= rows // 2 - 4 else rows // 2), s0


def intra_rows_for(qlen, longest):
    """swplan::intra_rows_for (the int32 wavefront kernel's rows per lane)."""
    best, best_cost = 16, 1e300
    for ri in range(2, 17, 2):
        nch = (qlen + 64 * ri - 1) // (64 * ri)
        cost = nch * (longest + 63) * (ri * 3.7 + 8.0)
        if cost < best_cost:
            best, best_cost = ri, cost
    return best


def row_seams(shape, qlen):
    """kind -> sorted seam rows (0 < row < qlen) of a kernel shape:
    ("x2s", pass rows, waves per group, short last pass, biased cell),
    ("int32", strip rows), ("coop",), ("intra", rows per lane) or ("pipe",)."""
    out = {}

    def put(kind, r):
        if 0 < r < qlen:
            out.setdefault(kind, set()).add(r)

    if shape[0] == "x2s":
        _, rows, G, short, biased = shape
        strip = rows // 2
        re_last, s_last = short_rows(qlen, rows) if short else (strip, -1)
        for p, s0 in enumerate(range(0, qlen, rows)):
            if p:
                put("hand-over" if G > 1 and p % G else "pass", s0)
            h = re_last if s0 == s_last else strip
            put("short-strip" if h != strip else "strip", s0 + h)
            if biased:
                for half in (0, 1):
                    for g in range(16, h, 16):
                        put("short-group" if h != strip else "row-group", s0 + half * h + g)
    elif shape[0] == "int32":
        for r in range(shape[1], qlen, shape[1]):
            put("int32-strip", r)
    elif shape[0] == "coop":
        for r in range(32, qlen, 32):
            put("coop-strip", r)
    else:
        ri, chunk = (shape[1], 64 * shape[1]) if shape[0] == "intra" else (2, 128)
        for r in range(ri, qlen, ri):
            put("chunk" if r % chunk == 0 else "lane", r)
    return {k: sorted(v) for k, v in out.items()}


def in_windows(rows):
    return [r for r in rows if any(lo <= r <= hi for lo, hi, _, _ in ROW_WINDOWS)]


# ---- the kernel forms (sw_opts overrides) -------------------------------------
# name: (layout, query length, gap models it runs under, overrides, shape(affine) -> row_seams shape)
# layout "split": long threshold 700 (probes inter, twins long); "long": 64 (every subject long)
_LPT = dict(lpt=1, intra_x2_rows=4, tail_pairs=0, lpt_persist=0, lpt_pipe=0, lpt_pipe_tail=0)
_SEP = dict(lpt=0, coop_width=0)


def _x2s(G, lpt=False, rows=None, short=True, biased=True):
    return lambda affine: ("x2s", rows or (96 if lpt and not affine else 64), G, short, biased)


FORMS = {
    "single": ("split", QLEN, "al", dict(_SEP, pair_width=0), _x2s(1)),
    "pairs-2": ("split", QLEN, "al", dict(_SEP, pair_width=16, pair_group=2), _x2s(2)),
    "pairs-4": ("split", QLEN, "al", dict(_SEP, pair_width=16, pair_group=4), _x2s(4)),
    "lpt-singles": ("split", QLEN, "al", dict(_LPT, pair_width=600, quad_width=0, tri_width=0), _x2s(1, True)),
    "lpt-quads": ("split", QLEN, "al", dict(_LPT, pair_width=16, quad_width=16, tri_width=0), _x2s(4, True)),
    # (3-wave groups under affine gaps only; the linear scan keeps its pairs)
    "lpt-tris": ("split", QLEN, "al", dict(_LPT, pair_width=16, quad_width=0, tri_width=16),
                 lambda affine: ("x2s", 64, 3, True, True) if affine else ("x2s", 96, 2, True, True)),
    "lpt-rows64": ("split", QLEN, "l", dict(_LPT, pair_width=16, quad_width=16, tri_width=0, lpt_rows=64),
                   _x2s(4, True, 64)),
    "lpt-rows96": ("split", QLEN, "l", dict(_LPT, pair_width=16, quad_width=16, tri_width=0, lpt_rows=96),
                   _x2s(4, True, 96)),
    "lpt-tail": ("split", QLEN, "al", dict(_LPT, pair_width=600, quad_width=0, tri_width=0, tail_pairs=8),
                 _x2s(2, True)),
    "lpt-persist": ("split", QLEN, "al", dict(_LPT, pair_width=16, quad_width=16, tri_width=0, lpt_persist=3,
                                              intra_x2_rows=8), _x2s(4, True)),
    "y32x8": ("split", QLEN, "al", dict(_SEP, pair_width=0, inter_variant="y32x8"), _x2s(1, biased=False)),
    "f32x4": ("split", QLEN, "a", dict(_SEP, pair_width=0, inter_variant="f32x4"), _x2s(1)),
    "32x8": ("split", QLEN, "al", dict(_SEP, inter_variant="32x8"), lambda affine: ("int32", 32)),
    "64x8": ("split", QLEN, "al", dict(_SEP, inter_variant="64x8"), lambda affine: ("int32", 64)),
    "coop-skew0": ("split", QLEN, "al", dict(lpt=0, inter_variant="32x8", coop_width=128, coop_skew=0),
                   lambda affine: ("coop",)),
    "coop-skew1": ("split", QLEN, "al", dict(lpt=0, inter_variant="32x8", coop_width=128, coop_skew=1),
                   lambda affine: ("coop",)),
    "intra-4": ("long", QLEN, "al", dict(intra_x2_rows=4), lambda affine: ("intra", 4)),
    "intra-8": ("long", QLEN, "al", dict(intra_x2_rows=8), lambda affine: ("intra", 8)),
    "intra-16": ("long", QLEN, "al", dict(intra_x2_rows=16), lambda affine: ("intra", 16)),
    "intra-20": ("long", QLEN, "al", dict(intra_x2_rows=20), lambda affine: ("intra", 20)),
    "intra-int32": ("long", QLEN, "al", dict(intra_x2=0),
                    lambda affine: ("intra", intra_rows_for(QLEN, QLEN + LS[-1] + TAIL))),
    "intra-int16": ("long", QLEN, "al", dict(intra_i16_first=1, intra_x2_rows=8), lambda affine: ("intra", 8)),
    # the pipelined pairs need a query of at most 4 chunks of 128 rows
    "lpt-pipe": ("split", 500, "al", dict(_LPT, pair_width=16, quad_width=16, tri_width=0, lpt_pipe=4,
                                          lpt_pipe_tail=100000), lambda affine: ("pipe",)),
}

# the seam kinds each shape must show inside a row window
KINDS = {"x2s": ("strip", "pass", "short-strip"), "int32": ("int32-strip",), "coop": ("coop-strip",),
         "intra": ("lane",), "pipe": ("lane", "chunk")}


def required_kinds(shape, qlen):
    kinds = list(KINDS[shape[0]])
    if shape[0] == "x2s":
        if shape[4]:
            kinds += ["row-group", "short-group"]
        if shape[2] > 1:
            kinds.append("hand-over")
        if qlen != QLEN:
            kinds = [k for k in kinds if not k.startswith("short")]
    if shape[0] == "intra" and 64 * shape[1] < qlen:
        kinds.append("chunk")
    return kinds


# ---- the native checker ---------------------------------------------------------
def build_checker(tmpdir):
    exe = os.path.join(str(tmpdir), "seam_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-pthread", SRC, "-o", exe], check=True,
                   timeout=300)
    return exe


def run_checker(exe, tmpdir, mats, scorings, q, subs, tasks, name="seam_in.txt"):
    """mats: list of 25 x 25; scorings: (matrix index, open, extend); tasks:
    (scoring, axis 0/1, seam, fault, [subject indices]).  Returns (base
    [scoring][subject], [(first detecting subject or -1, its score, tried)])."""
    path = os.path.join(str(tmpdir), name)
    with open(path, "w") as f:
        f.write("%d\n" % len(mats))
        for m in mats:
            f.write(" ".join(str(int(v)) for v in np.asarray(m).reshape(625)) + "\n")
        f.write("%d\n" % len(scorings))
        for s in scorings:
            f.write("%d %d %d\n" % tuple(s))
        f.write("%d %s\n" % (len(q), " ".join(map(str, q.tolist()))))
        f.write("%d\n" % len(subs))
        for s in subs:
            f.write("%d %s\n" % (len(s), " ".join(map(str, s.tolist()))))
        f.write("%d\n" % len(tasks))
        for k, axis, seam, fault, idx in tasks:
            f.write("%d %d %d %d %d %s\n" % (k, axis, seam, fault, len(idx), " ".join(map(str, idx))))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "seam_check ok", r.stdout[-2000:] + r.stderr[-2000:]
    base = [np.array(ln.split()[2:], dtype=np.int64) for ln in lines if ln.startswith("base ")]
    out = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("task ")]
    assert len(base) == len(scorings) and len(out) == len(tasks)
    return base, out
