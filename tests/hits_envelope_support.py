"""Inputs of the hit table's envelope tests (tests/test_hits_envelope_inputs.py
on the CPU, tests/test_gpu_hits_envelope.py on the GPU), and the matrices of
tests/test_gpu_scoring_envelope.py, which imports build_matrices from here.

Everything is generated from seeds, over all 25 residue codes (B, J, Z, X
and * included): matrices that are NOT symmetric, with entries and gaps at
the ends of the accepted range; prefixes of one 1,100-residue query that end
40 rows in, two rows past the first wave seam, inside the third wave, one row
past the first chunk and in a short third chunk; and subjects of 1..1,500
residues, planted copies of every query, and copies whose one gap run lies on
a chosen SUBJECT column (64, 128, 192: where a wave reads its next 64 top
cells and where the 128-column ring wraps) while its query rows stay at least
20 rows away from every wave seam.

A column seam s is the boundary between the 0-based subject columns s - 1 and
s.  A run of D (subject residues against gaps, along a row) covers the columns
of its residues; a run of I (query residues against gaps, down a column) sits
in the column of the last aligned pair before it.  A run lies on the seam if
one of its columns is s - 1 or s (run_columns, on_seam)."""
import numpy as np

from hits_support import row_of

N_CODES = 25
A, R = 0, 1  # residue codes of 'A' and 'R'
QUERY_RESIDUES = 1100
COLUMN_SEAMS = (64, 128, 192)
SEAM_ROW_MARGIN = 20  # a column-seam run's query rows keep this distance from the wave seams


# ---- the scorings -----------------------------------------------------------
def build_matrices(sw):
    rng = np.random.default_rng(2024)
    asym = rng.integers(-12, 13, size=(25, 25))
    np.fill_diagonal(asym, rng.integers(3, 14, size=25))
    one = np.full((25, 25), -5)
    one[A, R] = 5
    d100 = rng.integers(-100, 0, size=(25, 25))
    d100[3, 17], d100[17, 3] = -100, -1
    np.fill_diagonal(d100, 100)
    nonpos = rng.integers(-12, 1, size=(25, 25))
    nonpos[5, 5] = nonpos[2, 9] = 0
    pm100 = np.where(rng.random((25, 25)) < 0.3, 100, -100)
    np.fill_diagonal(pm100, 100)
    pm100[24, 24] = -100
    out = {"asym": asym, "one": one, "d100": d100, "nonpos": nonpos, "pm100": pm100,
           "b50": sw.capi.builtin_matrix(0), "b62": sw.capi.builtin_matrix(1)}
    out = {k: np.ascontiguousarray(v, dtype=np.int8) for k, v in out.items()}
    for k in ("asym", "one", "d100", "nonpos", "pm100"):
        assert (out[k] != out[k].T).any()
    assert out["nonpos"].max() == 0 and out["d100"].max() == 100 and out["d100"].min() == -100
    assert out["b62"].max() == 11 and out["b50"].max() == 15
    return out


IDNEG_DIAGONAL = {4: 0, 21: -2, 23: 0}  # C, J and X: identities that are not positives


def matrices(sw):
    """The envelope's matrices plus idneg: asym with three diagonal entries <= 0."""
    out = build_matrices(sw)
    idneg = out["asym"].copy()
    for code, v in IDNEG_DIAGONAL.items():
        idneg[code, code] = v
    out["idneg"] = idneg
    for k, m in out.items():
        assert m.dtype == np.int8 and m.shape == (25, 25)
        assert k in ("b50", "b62") or (m != m.T).any(), k
    return out


# name: (matrix, open, extend)
SCORINGS = {
    "asym-12-1": ("asym", 12, 1),
    "asym-2-2": ("asym", 2, 2),
    "asym-7-3": ("asym", 7, 3),
    "asym-1-4": ("asym", 1, 4),              # open below extend
    "idneg-11-1": ("idneg", 11, 1),          # identities that are not positives
    "d100-27-27": ("d100", 27, 27),
    "d100-28-28": ("d100", 28, 28),
    "d100-40-28": ("d100", 40, 28),          # scores to 110,000
    "nonpos-12-1": ("nonpos", 12, 1),        # every row all-zero but id and s_len
    "pm100-1000-1000": ("pm100", 1000, 1000),
    "pm100-3-1": ("pm100", 3, 1),
    "b62-11-1": ("b62", 11, 1),
}


# ---- queries and subjects ---------------------------------------------------
def wave_rows(sw):
    """Query rows of one wave of sw_hits."""
    return sw.capi.HITS_ROWS_PER_LANE * 64


def query_lengths(sw):
    return [40, wave_rows(sw) + 2, 375, sw.capi.HITS_CHUNK_ROWS + 1, QUERY_RESIDUES]


def _clear_of_wave_seams(lo, hi, wrows):
    """Rows lo..hi (0-based) are all at least SEAM_ROW_MARGIN rows from a multiple of wrows."""
    return all(min(r % wrows, wrows - r % wrows) >= SEAM_ROW_MARGIN for r in (lo, hi))


def _column_seam_subjects(q, first_row, wrows, rng):
    """[(subject, seam, kind, L)]: pieces of q with one run on each column seam.

    kind "I": L query rows are missing after the subject's column c (c = s - 1,
    s); kind "D": L foreign residues stand in columns c .. c + L - 1 (the run
    starts on, crosses and ends on s: c = s, s - 1, s - L + 1).  The query row p
    of the edit is the first one >= first_row + c whose rows are clear of the
    wave seams and whose neighbours leave the run no second place."""
    out = []
    n = len(q)
    for s in COLUMN_SEAMS:
        for L in (1, 5):
            for kind, cols in (("I", (s - 1, s)), ("D", sorted({s, s - 1, s - L + 1}))):
                for c in cols:
                    before = c + 1 if kind == "I" else c  # residues of the subject before the edit
                    p = next(p for p in range(first_row + before, n - L - 60)
                             if _clear_of_wave_seams(p - 2, p + L + 1, wrows)
                             # (I: the missing rows must not pass for their neighbours)
                             and not (kind == "I" and (q[p] == q[p + L] or q[p - 1] == q[p + L - 1]))
                             # (B, J, Z, X, *: rows so flat that a run beside one may move for free)
                             and max(q[p - 2:p + L + 2]) < 20)
                    tail = min(80, n - p - (L if kind == "I" else 0))
                    if kind == "I":
                        sub = np.concatenate([q[p - before:p], q[p + L:p + L + tail]])
                    else:
                        other = np.setdiff1d(np.arange(20, dtype=np.uint8), [q[p - 1], q[p]])
                        sub = np.concatenate([q[p - before:p], other[rng.integers(0, len(other), size=L)], q[p:p + tail]])
                    out.append((sub.astype(np.uint8), s, kind, L))
    return out


def _embed_piece(sub, q0, k, rng):
    """Overwrites part of a random subject (of at least 24 residues) with a
    piece of the query's first 40 rows, common to every query, that lacks 1..3
    rows or holds 1..3 foreign residues between flanks of 8 or 12 rows: under a
    gap that costs far more than a mismatch (BLOSUM62 11 / 1) unrelated
    sequences seldom align with a gap, and every other subject stays unrelated
    for the tied best cells."""
    if len(sub) < 24:
        return
    f, d = (8 if len(sub) < 40 else 12), 1 + k // 2 % 3
    a = int(rng.integers(0, 40 - 2 * f - d + 1))
    if k % 4 == 1:
        piece = np.concatenate([q0[a:a + f], q0[a + f + d:a + 2 * f + d]])
    else:
        piece = np.concatenate([q0[a:a + f], (q0[a + f:a + f + d] + 7) % N_CODES, q0[a + f:a + 2 * f]])
    at = int(rng.integers(0, len(sub) - len(piece) + 1))
    sub[at:at + len(piece)] = piece


class Inputs:
    """mats, scorings' names, queries, subs, res / offs, planted[qlen] (4
    subject indices per query length) and column_seams: [(subject index, query
    index, seam, kind, L)]."""


def build_inputs(sw):
    e = Inputs()
    e.mats = matrices(sw)
    rng = np.random.default_rng(20267)
    q0 = rng.integers(0, N_CODES, size=QUERY_RESIDUES).astype(np.uint8)
    e.qlens = query_lengths(sw)
    assert e.qlens == sorted(e.qlens) and e.qlens[-1] == len(q0) > 2 * sw.capi.HITS_CHUNK_ROWS
    e.queries = [q0[:n] for n in e.qlens]
    subs = []
    for lo, hi, forced in ((1, 40, (1, 2, 39, 40)), (41, 136, (63, 64, 65, 127, 128, 129)),
                           (137, 300, (191, 192, 193, 256, 257))):
        lens = list(forced) + [int(x) for x in rng.integers(lo, hi + 1, size=24 - len(forced))]
        subs += [rng.integers(0, N_CODES, size=n).astype(np.uint8) for n in lens]
    subs += [rng.integers(0, N_CODES, size=int(n)).astype(np.uint8) for n in rng.integers(700, 1501, size=6)]
    for k in range(len(subs)):  # every other subject, and all of the longest 18 (which seldom tie anyway)
        if k % 2 or k >= 60:
            _embed_piece(subs[k], q0, k, rng)
    e.planted = {}
    for n in e.qlens:
        q = q0[:n]
        ins = np.sort(rng.choice(np.arange(5, n - 5), size=5, replace=False))
        e.planted[n] = list(range(len(subs), len(subs) + 4))
        subs += [q.copy(), q[:n // 2].copy(), np.concatenate([q[:n // 2], q[n // 2 + 3:]]),
                 np.insert(q, ins, rng.integers(0, N_CODES, size=5).astype(np.uint8))]
    e.column_seams = []
    wrows = wave_rows(sw)
    # the 375-row query from its first rows, the 1,100-row one inside its second chunk
    for qi, first_row in ((e.qlens.index(375), 0), (len(e.qlens) - 1, sw.capi.HITS_CHUNK_ROWS + 60)):
        for sub, s, kind, L in _column_seam_subjects(e.queries[qi], first_row, wrows, rng):
            e.column_seams.append((len(subs), qi, s, kind, L))
            subs.append(sub)
    e.subs = subs
    e.res = np.concatenate(subs).astype(np.uint8)
    e.offs = np.zeros(len(subs) + 1, dtype=np.int64)
    e.offs[1:] = np.cumsum([len(s) for s in subs])
    for a in e.queries + e.subs + [e.res, e.offs] + list(e.mats.values()):
        a.setflags(write=False)
    return e


# ---- the oracle's rows --------------------------------------------------------
class Want:
    """The oracle's alignments and rows, once per (scoring name or (matrix,
    open, extend), query index): als(...)[k] / rows(...)[k] belong to subject k,
    rows carry id k."""

    def __init__(self, oracle, inputs):
        self.oracle, self.inputs, self.cache = oracle, inputs, {}

    def _get(self, scname, qi):
        if (scname, qi) not in self.cache:
            e = self.inputs
            mk, go, ge = SCORINGS[scname]
            m, q = e.mats[mk], e.queries[qi]
            als = [self.oracle.align(q, s, m, go, ge) for s in e.subs]
            rows = [row_of(al, q, s, m, k) for k, (al, s) in enumerate(zip(als, e.subs))]
            self.cache[(scname, qi)] = (als, rows)
        return self.cache[(scname, qi)]

    def als(self, scname, qi):
        return self._get(scname, qi)[0]

    def rows(self, scname, qi):
        return self._get(scname, qi)[1]


def rows_under(oracle, q, subs, mat, go, ge):
    """The oracle's rows of q against subs under any matrix (the wrong-index ones)."""
    return [row_of(oracle.align(q, s, mat, go, ge), q, s, mat, k) for k, s in enumerate(subs)]


def run_columns(al):
    """[(op, [0-based subject columns])] of every gap run of an alignment: a D
    run's own columns; for an I run the column of the pair before it."""
    i, j = al["q_begin"] - 1, al["s_begin"] - 1
    runs, prev = [], ""
    for op in al["ops"]:
        if op == "M":
            i, j = i + 1, j + 1
        elif op == "D":
            if prev != "D":
                runs.append(("D", []))
            runs[-1][1].append(j)
            j += 1
        else:
            if prev != "I":
                runs.append(("I", [j - 1]))
            i += 1
        prev = op
    return runs


def run_rows(al):
    """[(op, [0-based query rows])] of every gap run: an I run's own rows; for a
    D run the row of the pair before it."""
    i, j = al["q_begin"] - 1, al["s_begin"] - 1
    runs, prev = [], ""
    for op in al["ops"]:
        if op == "M":
            i, j = i + 1, j + 1
        elif op == "I":
            if prev != "I":
                runs.append(("I", []))
            runs[-1][1].append(i)
            i += 1
        else:
            if prev != "D":
                runs.append(("D", [i - 1]))
            j += 1
        prev = op
    return runs


def on_seam(cols, s):
    return s - 1 in cols or s in cols


def path_codes(al, q, s):
    """(query codes, subject codes) on the aligned pairs of a path."""
    i, j = al["q_begin"] - 1, al["s_begin"] - 1
    qc, sc = set(), set()
    for op in al["ops"]:
        if op == "M":
            qc.add(int(q[i]))
            sc.add(int(s[j]))
            i, j = i + 1, j + 1
        elif op == "I":
            i += 1
        else:
            j += 1
    return qc, sc
