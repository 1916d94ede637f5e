"""Shared by the traceback tests (tests/test_align_inputs.py on the CPU,
tests/test_gpu_align_rules.py on the GPU).

align_py is a plain Python restatement of the traceback's rules as
csrc/sw_align.hip and oracle/sw_oracle.c state them:

  * E(i, j) opens from H(i, j-1) unless extending E(i, j-1) is STRICTLY
    better; F(i, j) likewise down the column;
  * H(i, j) takes E (left), then F (up), then the diagonal, each only on a
    strict improvement over the running value that starts at 0;
  * the end cell is the first strict maximum in row-major order;
  * the walk back follows a gap run to the cell that opened it and stops at a
    cell without a source.

With gap == gap_extend no run ever extends and the rules are cpu.cpp's linear
ones.  variant= swaps one rule for a wrong one (VARIANTS); a wrong rule still
finds an optimal alignment, so only inputs whose optimal paths tie can tell it
from the right one.  The tie set below is such inputs: few letters, custom
match / mismatch matrices, and scorings with 2 gap < |mismatch| under both gap
models, where an I D pair beats a mismatch and the left-before-up rule lies on
traced paths.  tests/test_align_inputs.py asserts that every variant differs
from the oracle somewhere on the set, i.e. that the set can tell the rules
apart."""
import numpy as np

VARIANTS = ("up_first",    # H takes F before E
            "diag_first",  # H takes the diagonal before E and F
            "last_max",    # the last maximum in row-major order ends the alignment
            "col_major",   # on equal maxima: the smaller column, then the smaller row
            "e_ext_tie",   # E extends on a tie
            "f_ext_tie")   # F extends on a tie
AFFINE_ONLY = ("e_ext_tie", "f_ext_tie")  # under a linear gap an extension is never taken

NEG = -(1 << 29)


def align_py(q, s, mat, gap, gap_extend=None, variant=None):
    """The dict oracle.align returns; variant None: the rules above."""
    assert variant is None or variant in VARIANTS
    go, ge = gap, gap if gap_extend is None else gap_extend
    n, m = len(q), len(s)
    zero = {"score": 0, "q_end": 0, "s_end": 0, "q_begin": 0, "s_begin": 0, "ops": ""}
    if n == 0 or m == 0:
        return zero
    order = {"up_first": (2, 1, 3), "diag_first": (3, 1, 2)}.get(variant, (1, 2, 3))
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    T = [[0] * (m + 1) for _ in range(n + 1)]  # bits 0-1: H's source; bit 2: E extends; bit 3: F extends
    best, bi, bj = 0, 0, 0
    for i in range(1, n + 1):
        row = mat[q[i - 1]]
        for j in range(1, m + 1):
            t = 0
            e, x = H[i][j - 1] - go, E[i][j - 1] - ge
            if x > e or (variant == "e_ext_tie" and x == e):
                e, t = x, t | 4
            f, x = H[i - 1][j] - go, F[i - 1][j] - ge
            if x > f or (variant == "f_ext_tie" and x == f):
                f, t = x, t | 8
            cand = {1: e, 2: f, 3: H[i - 1][j - 1] + int(row[s[j - 1]])}
            h = 0
            for src in order:
                if cand[src] > h:
                    h, t = cand[src], (t & 12) | src
            H[i][j], E[i][j], F[i][j], T[i][j] = h, e, f, t
            if h > best:
                wins = True
            elif h == best and h > 0:
                wins = variant == "last_max" or (variant == "col_major" and (j, i) < (bj, bi))
            else:
                wins = False
            if wins:
                best, bi, bj = h, i, j
    i, j, state, ops = bi, bj, 0, []
    while i > 0 and j > 0:
        t = T[i][j]
        if state == 0:
            src = t & 3
            if src == 0:
                break
            if src != 3:
                state = src
                continue
            ops.append("M")
            i, j = i - 1, j - 1
        elif state == 1:
            ops.append("D")
            state = 1 if t & 4 else 0
            j -= 1
        else:
            ops.append("I")
            state = 2 if t & 8 else 0
            i -= 1
    return {"score": best, "q_end": bi, "s_end": bj, "q_begin": i + 1, "s_begin": j + 1, "ops": "".join(reversed(ops))}


def identity_matrix(match, mismatch):
    """25 x 25 int8: match on the diagonal, mismatch elsewhere."""
    m = np.full((25, 25), mismatch, dtype=np.int8)
    np.fill_diagonal(m, match)
    return m


# name: (letters, match, mismatch, gap, gap_extend).  2 gap < |mismatch| in
# lin-3-2m4-1, aff-3-2m5-2-1: an I D pair (2 gap) beats a mismatch there.
SCORINGS = {
    "lin-2-3m3-2": (2, 3, -3, 2, 2),
    "lin-3-2m4-1": (3, 2, -4, 1, 1),
    "lin-3-2m4-3": (3, 2, -4, 3, 3),
    "aff-2-3m3-3-1": (2, 3, -3, 3, 1),
    "aff-3-2m4-2-1": (3, 2, -4, 2, 1),
    "aff-3-2m5-2-1": (3, 2, -5, 2, 1),
    "aff-3-3m2-3-1": (3, 3, -2, 3, 1),
}


def is_affine(name):
    return SCORINGS[name][3] != SCORINGS[name][4]


def scoring(name):
    """(matrix, gap, gap_extend) of a SCORINGS entry."""
    _, match, mismatch, go, ge = SCORINGS[name]
    return identity_matrix(match, mismatch), go, ge


def _groups(letters, seed, nq, ns):
    """nq queries of 1..40 letters with ns subjects each: random ones, a
    repeat of a short motif, and a copy of the query with letters changed."""
    rng = np.random.default_rng(seed)

    def rand(lo=1, hi=40):
        return rng.integers(0, letters, size=int(rng.integers(lo, hi + 1))).astype(np.uint8)

    groups = []
    for k in range(nq):
        q = rand(1, 6) if k == 0 else rand(8, 40)
        subs = [rand() for _ in range(ns - 2)]
        motif = rand(1, 4)
        subs.append(np.tile(motif, 40 // len(motif))[: int(rng.integers(1, 41))])
        c = q.copy()
        c[rng.integers(0, len(c), size=max(1, len(c) // 6))] = rng.integers(0, letters)
        subs.append(c)
        groups.append((q, subs))
    return groups


# letters -> [(query, [subject, ...]), ...]: a query and its subjects make one
# GPU call; every (query, subject) of a scoring's alphabet is a pair of the set
TIE_GROUPS = {2: _groups(2, 20261, 10, 14), 3: _groups(3, 20262, 14, 16)}


def tie_cases(name):
    """(group index, subject index, query, subject) of every pair under a scoring."""
    for g, (q, subs) in enumerate(TIE_GROUPS[SCORINGS[name][0]]):
        for k, s in enumerate(subs):
            yield g, k, q, s


def periodic(motif, k):
    return np.tile(np.asarray(motif, dtype=np.uint8), k)
