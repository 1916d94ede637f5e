"""Inputs past 2^15 and 2^16 in either direction.  Shared by
tests/test_length_inputs.py (CPU: what the inputs can see of a count or an
index that is cut or wraps, oracle only) and tests/test_gpu_lengths.py (GPU:
every kernel family on the same inputs, bit for bit against the oracle).

G, the giants.  Seven subjects of GIANTS residues (the two powers on both
sides at blk_cols' 8-column granularity, the longest Swiss-Prot record, one odd
length past everything) among N_FILLERS fillers of 2 .. 3,000 residues (a long
threshold is at least 1, so that every subject can be long), in a shuffled
order; ids_custom gives the variant's result ids 3 perm(i) + 1.  The query is
tests/seam_support.py's 568-residue one (no residue twice in a row); q900,
q1300 and q600 are longer queries whose first 568, first 900 and last 568 rows
are that query, the 900-row one and that query.  Each giant is random residues
(the 20 amino acids; the giants of 35,213 and 70,001 over all 25 codes) with
pieces of the query planted, 0-based columns:
  start  columns 100 .. 399: query rows 0 .. 299, about 25 % substituted.
  cross  query rows 100 .. 499 (400 rows) with ONE gap run on a power P (2^15;
         2^16 where the giant holds it clear of the end piece): kind "ins", 5
         columns inserted at P - 2 .. P + 2 (the run starts before and ends
         after column P); kind "del", query rows 300 .. 304 deleted with the
         junction on P (column P - 1 aligns row 299, column P row 305).  The
         giants take the kinds in turn; 70,001 has "del" at 2^15 and "ins" at
         2^16.  A giant of at most 2^15 + 1,400 columns that cannot hold the
         piece on 2^15 gets it on 2^14.
  end    the 900-row query of tests/seam_support.py (the 568 rows and 332
         more) with rows 280 .. 282 deleted, 897 columns ending END_PAD = 40
         columns before the subject's end.  Its first 565 columns are the
         568-row query's best piece: the subject's score is that piece's and
         depends on columns L - 937 .. L - 373 being scanned, in their places;
         under the 900-row and the 1,300-row query on all of L - 937 .. L - 41
         (and, the matrix scaled, the giants then pass the int16 guard).

Q_long and S.  QLONG rows: prefixes of one 65,544-row random query (20 amino
acids).  S(n), the database of the n-row query: N_S subjects of 2 .. 400
residues, at most 12,000 in all; every second one a piece of the query (60 ..
300 rows, one indel of 1 .. 3 rows or columns in its middle) from, in turn,
the rows across 2^15, the rows across 2^16 and the last 600 rows, for the
regions the query has.  In a power's region the pieces alternate between
straddling the power and starting 1 .. 150 rows past it; where the query ends
8 rows past the power (32,776 and 65,544) every piece straddles it and ends
on the query's last rows.

T, the square case.  The 35,213-row query, with a database of the query
itself, a copy with 10 % substitutions and three indels, and 62 fillers;
square_short() is T cut to 12,000 rows and columns (the lane layout's).

Scorings: SCORINGS (BLOSUM62 11/1, BLOSUM50 linear 2) and, for the rescue
chains, tests/seam_support.py's RESCUE_SCORINGS (the matrix and gaps times 9
and times 6).

Oracle work is memoised at module scope per (query, database, scoring);
oracle_seconds() is what it has cost so far."""
import time

import numpy as np

import seam_support as ss
from hits_support import expected as expected_row
from hits_support import pack

P15, P16 = 1 << 15, 1 << 16
GIANTS = (32760, 32768, 35213, 65528, 65536, 65544, 70001)
ALL_CODES = (35213, 70001)
N_FILLERS = 57
END_PAD = 40
END_DEL = (280, 3)            # the end piece: rows 280 .. 282 deleted
END_COLS = 900 - 3            # its columns: the 900-row query's
CROSS_ROWS = (100, 500)       # the cross piece's query rows
CROSS_AT = 200                # the gap run's place inside it (query row 300)
CROSS_L = 5
QLONG = (32760, 32776, 35213, 65544)
N_S = 120
S_RESIDUES = 12000
T_QLEN = 35213
T_FILLERS = 62
# (matrix id, open, extend)
SCORINGS = ((1, 11, 1), (0, 2, 2))
RESCUE_SCORINGS = ss.RESCUE_SCORINGS
K_SAT16 = 32767 - 1152
CUTS = (P15 - 1, P15, P16 - 1, P16)

_cache = {}
_spent = [0.0]


class Inputs:
    pass


def oracle_seconds():
    return _spent[0]


def _sub(rng, piece, rate):
    """piece with about `rate` of its residues replaced by another one."""
    out = piece.copy()
    hit = rng.random(len(out)) < rate
    out[hit] = (out[hit] + rng.integers(1, 20, size=int(hit.sum()))) % 20
    return out


def cross_powers(L):
    """The powers a giant of L columns holds a cross piece on: clear of the
    end piece (which starts at L - 605) by more than 300 columns."""
    ps = [p for p in (P15, P16) if p + 205 + 300 < L - END_PAD - END_COLS]
    return ps or [1 << 14]


def giants():
    """G: .q (568), .q1300, .q600, .subs, .res, .offs, .giant (index in subs
    of each giant, by length), .plan[L] = {"start": (c0, c1), "end": (c0, c1),
    "cross": [(power, kind, c0, c1)]} (0-based column ranges, c1 exclusive)."""
    if "g" in _cache:
        return _cache["g"]
    P = ss.build()
    q = P.q
    rng = np.random.default_rng(70001)
    g = Inputs()
    g.q = q
    # longer and shorter queries over the same rows: the 568 first, then others
    # of seam_support's alphabet; the 600-row one ends on the query's last row
    g.q1300 = np.concatenate([P.q2, ss.ALPHABET[np.cumsum(rng.integers(1, 16, size=1300 - len(P.q2))) % 16]])
    g.q600 = np.concatenate([ss.ALPHABET[np.cumsum(rng.integers(1, 16, size=600 - len(q))) % 16], q])
    # the end piece: the 900-row query with rows 280 .. 282 deleted; the 568-row query's part is its first 565 columns
    end_piece = np.concatenate([q[:END_DEL[0]], q[END_DEL[0] + END_DEL[1]:], P.q2[ss.QLEN:]])
    g.q900 = P.q2
    other = np.array([4, 8, 14, 17], dtype=np.uint8)  # C, H, P, W: none in the query
    subs, plan, kind_turn = {}, {}, 0
    for L in GIANTS:
        s = rng.integers(0, 25 if L in ALL_CODES else 20, size=L).astype(np.uint8)
        pl = {"start": (100, 400), "cross": []}
        s[100:400] = _sub(rng, q[:300], 0.25)
        for p in cross_powers(L):
            kind = ("ins", "del")[kind_turn % 2] if L != 70001 else ("del" if p == P15 else "ins")
            kind_turn += 1
            a, b = CROSS_ROWS
            if kind == "ins":
                piece = np.concatenate([q[a:a + CROSS_AT], other[rng.integers(0, 4, size=CROSS_L)], q[a + CROSS_AT:b]])
                c0 = p - 2 - CROSS_AT
            else:
                piece = np.concatenate([q[a:a + CROSS_AT], q[a + CROSS_AT + CROSS_L:b]])
                c0 = p - CROSS_AT
            s[c0:c0 + len(piece)] = piece
            pl["cross"].append((p, kind, c0, c0 + len(piece)))
        e1 = L - END_PAD
        s[e1 - len(end_piece):e1] = end_piece
        pl["end"] = (e1 - len(end_piece), e1 - ss.TAIL)   # the 568-row query's part
        pl["end900"] = (e1 - len(end_piece), e1)
        subs[L], plan[L] = s, pl
    fillers = [rng.integers(0, 20, size=int(n)).astype(np.uint8)
               for n in np.concatenate([[2, 3, 3000], rng.integers(2, 3001, size=N_FILLERS - 3)])]
    everything = [subs[L] for L in GIANTS] + fillers
    order = rng.permutation(len(everything))
    g.subs = [everything[k] for k in order]
    g.giant = {L: int(np.nonzero(order == k)[0][0]) for k, L in enumerate(GIANTS)}
    g.plan = plan
    g.res, g.offs = pack(g.subs)
    g.ids_custom = (3 * np.random.default_rng(3).permutation(len(g.subs)) + 1).astype(np.int32)
    for a in (g.q1300, g.q600, g.res, g.offs, g.ids_custom):
        a.setflags(write=False)
    _cache["g"] = g
    return g


def long_base():
    if "qb" not in _cache:
        qb = np.random.default_rng(65544).integers(0, 20, size=QLONG[-1]).astype(np.uint8)
        qb.setflags(write=False)
        _cache["qb"] = qb
    return _cache["qb"]


def long_query(n):
    return long_base()[:n]


def regions(n):
    """name -> (power or None, first row, last row + 1) of the query regions
    the n-row query has."""
    out = {}
    if n > P15:
        out["p15"] = (P15, P15 - 300, min(n, P15 + 450))
    if n > P16:
        out["p16"] = (P16, P16 - 300, min(n, P16 + 450))
    out["last"] = (None, n - 600, n)
    return out


def S(n):
    """The database of the n-row long query: .subs, .res, .offs, .meta[k] =
    (region, first row, rows) or None for a filler."""
    key = ("S", n)
    if key in _cache:
        return _cache[key]
    q = long_query(n)
    rng = np.random.default_rng(n)
    reg = regions(n)
    names = list(reg)
    d = Inputs()
    d.subs, d.meta = [], []
    turn = {r: 0 for r in names}
    budget = S_RESIDUES
    for k in range(N_S):
        left = N_S - k
        if k % 2 == 0:
            r = names[(k // 2) % len(names)]
            power, lo, hi = reg[r]
            rows = int(rng.integers(60, 301))
            if power is None:
                r0 = int(rng.integers(lo, hi - rows + 1))
            elif turn[r] % 2 == 0 or hi - power < 70:     # straddles the power
                r0 = max(lo, min(power - rows // 2, hi - rows))
                r0 -= int(rng.integers(0, 8)) if r0 - 8 >= lo else 0
            else:                                          # starts just past it
                rows = min(rows, hi - power - 1)
                r0 = int(rng.integers(power + 1, hi - rows + 1)) if hi - rows > power else power + 1
            turn[r] += 1
            piece = q[r0:r0 + rows]
            mid, L = len(piece) // 2, int(rng.integers(1, 4))
            if (k // 2) % 2:
                s = np.concatenate([piece[:mid], piece[mid + L:]])
            else:
                s = np.concatenate([piece[:mid], rng.integers(0, 20, size=L).astype(np.uint8), piece[mid:]])
            d.meta.append((r, r0, len(piece)))
        else:
            cap = max(1, min(400, (budget - 300 * (left // 2)) // max(1, (left + 1) // 2)))
            s = rng.integers(0, 20, size=int(rng.integers(2, max(cap, 2) + 1))).astype(np.uint8)
            d.meta.append(None)
        budget -= len(s)
        d.subs.append(s)
    d.subs[1] = d.subs[1][:2]        # two residues
    d.res, d.offs = pack(d.subs)
    assert d.offs[-1] <= S_RESIDUES and max(len(s) for s in d.subs) <= 400
    _cache[key] = d
    return d


def square():
    """T: .q (35,213 rows), .subs (the query, its mutated copy, 62 fillers)."""
    if "t" in _cache:
        return _cache["t"]
    q = long_query(T_QLEN)
    rng = np.random.default_rng(35213)
    t = Inputs()
    t.q = q
    c = _sub(rng, q, 0.10)
    c = np.concatenate([c[:9000], c[9004:20000], rng.integers(0, 20, size=6).astype(np.uint8), c[20000:33000],
                        c[33002:]])
    fillers = [rng.integers(0, 20, size=int(n)).astype(np.uint8) for n in rng.integers(1, 1500, size=T_FILLERS)]
    everything = [q.copy(), c] + fillers
    order = rng.permutation(len(everything))
    t.subs = [everything[k] for k in order]
    t.self_at, t.copy_at = (int(np.nonzero(order == k)[0][0]) for k in (0, 1))
    t.res, t.offs = pack(t.subs)
    _cache["t"] = t
    return t


T_SHORT = 12000


def square_short():
    """T cut to T_SHORT rows and columns, for the lane layout: there one wave
    group scans the 64 subjects' block, 35,216 columns x 35,213 rows through the
    fp16, int16 and int32 stages in 33 s (measured); 12,000 rows still put
    the self score past fp16 and the copy's past int16, in about 4 s."""
    if "ts" not in _cache:
        t = square()
        u = Inputs()
        u.q = t.q[:T_SHORT]
        u.subs = [s[:T_SHORT] for s in t.subs]
        u.self_at, u.copy_at = t.self_at, t.copy_at
        u.res, u.offs = pack(u.subs)
        _cache["ts"] = u
    return _cache["ts"]


def scaled(mat, k):
    return np.ascontiguousarray(np.asarray(mat).astype(np.int64) * k, dtype=np.int8)


def scan(oracle, name, q, db, mat, go, ge):
    """oracle.scan, memoised per (name of query and database, scoring)."""
    key = ("scan", name, int(np.asarray(mat).astype(np.int64).sum()), int(mat[0][0]), go, ge)
    if key not in _cache:
        t0 = time.perf_counter()
        out = oracle.scan(q, db.res, db.offs, mat=mat, gap_open=go, gap_extend=ge, nthreads=16)
        _spent[0] += time.perf_counter() - t0
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def row(oracle, name, q, s, mat, go, ge, rid):
    """hits_support.expected (the oracle's alignment as a hit-table row),
    memoised per (name of query and subject, scoring); id = rid."""
    key = ("row", name, int(np.asarray(mat).astype(np.int64).sum()), int(mat[0][0]), go, ge)
    if key not in _cache:
        t0 = time.perf_counter()
        _cache[key] = expected_row(oracle, q, s, mat, go, ge, 0)
        _spent[0] += time.perf_counter() - t0
    return dict(_cache[key], id=int(rid))


def align(oracle, name, q, s, mat, go, ge):
    key = ("align", name, int(np.asarray(mat).astype(np.int64).sum()), int(mat[0][0]), go, ge)
    if key not in _cache:
        t0 = time.perf_counter()
        _cache[key] = oracle.align(q, s, mat, go, ge)
        _spent[0] += time.perf_counter() - t0
    return dict(_cache[key])


def align_dirs_bytes(qlen, slen):
    """swplan::align_dirs_bytes restated: one byte per cell, diagonal-major."""
    return (qlen + slen + 1) * (qlen + 1)


# ---- the kernel names of G's scans ---------------------------------------------
# What scan_plan names for G per (layout, scoring, query rows), the library's
# own policies but in "split-merged" (MERGED below).  tests/test_length_plan.py
# asserts that tests/native/length_check.cpp prints exactly these from the
# real scan_plan on the CPU; tests/test_gpu_lengths.py asserts them on the
# device: a change of routing is made in both places.
LAYOUTS = {"lanes": 100000, "long": 1, "own": None, "split": 3000}   # long thresholds (None: the library's, 64)
MERGED = dict(lpt=1, pair_width=16, intra_x2_rows=8)
SCORING_NAMES = ("b62-11-1", "b50-2-2")
_X2P_A, _X2P_L = "sw_inter_x2p<32,8,affine,fp16>", "sw_inter_x2p<32,8,linear,fp16>"
_X2S_A, _X2S_L = "sw_inter_x2s<32,8,affine,fp16>", "sw_inter_x2s<32,8,linear,fp16>"
NAMES = {}
for _q, _ri in ((568, 10), (900, 16), (1300, 12)):
    NAMES["lanes", "b62-11-1", _q] = (_X2P_A, "none")
    NAMES["lanes", "b50-2-2", _q] = (_X2P_L, "none")
    NAMES["own", "b62-11-1", _q] = (_X2S_A, "sw_intra_x2<%d>" % _ri)
    NAMES["own", "b50-2-2", _q] = (_X2S_L, "sw_intra_x2<%d>" % _ri)
    for _s in SCORING_NAMES:   # (no inter blocks: no inter name)
        NAMES["long", _s, _q] = (None, "sw_intra_x2<%d>" % _ri)
    NAMES["split", "b62-11-1", _q] = (_X2P_A + ("+tri1" if _q == 568 else "") + "+lpt+drain", "sw_intra_x2<8>")
    NAMES["split", "b50-2-2", _q] = (_X2P_L, "sw_intra_x2<%d>" % _ri)
    NAMES["split-merged", "b62-11-1", _q] = NAMES["split", "b62-11-1", _q]
    NAMES["split-merged", "b50-2-2", _q] = ("sw_inter_x2p<48,8,linear,fp16>+lpt+drain", "sw_intra_x2<8>")
