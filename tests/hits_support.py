"""Expected hit-table rows (sw_hit, include/sw_amd.h), derived from the
oracle's traceback: shared by tests/test_gpu_hits.py's cases; and the seam
inputs (gap runs placed on chosen query rows), shared with
tests/test_gpu_align_rules.py.

A row is a function of the alignment oracle.align reports: its begin and end
cells and its ops string.  identities and positives come from replaying the
ops over the two sequences, gap_opens counts maximal runs of I or of D, and a
hit of score 0 reports 0 in every field but id and s_len (the oracle's 1 / 0
begin / end pair is not carried over)."""
import numpy as np

FIELDS = ("id", "score", "q_begin", "q_end", "s_begin", "s_end", "s_len", "length", "identities", "positives",
          "gap_opens", "gaps")


def row_of(al, q, s, mat, rid):
    """The row of alignment `al` (a dict of oracle.align / Database.align)."""
    row = dict.fromkeys(FIELDS, 0)
    row["id"], row["s_len"] = int(rid), len(s)
    if al["score"] == 0:
        return row
    row.update(score=al["score"], q_begin=al["q_begin"], q_end=al["q_end"], s_begin=al["s_begin"], s_end=al["s_end"],
               length=len(al["ops"]))
    i, j, prev = al["q_begin"] - 1, al["s_begin"] - 1, ""
    for op in al["ops"]:
        if op == "M":
            row["identities"] += int(q[i] == s[j])
            row["positives"] += int(mat[q[i]][s[j]] > 0)
            i += 1
            j += 1
        else:
            row["gaps"] += 1
            row["gap_opens"] += int(op != prev)
            if op == "I":
                i += 1
            else:
                j += 1
        prev = op
    assert (i, j) == (al["q_end"], al["s_end"])
    return row


def expected(oracle, q, s, mat, go, ge, rid):
    return row_of(oracle.align(q, s, mat, go, ge), q, s, mat, rid)


def pack(subs):
    """(residues, offsets) of a list of code arrays."""
    res = np.concatenate([np.asarray(s, dtype=np.uint8) for s in subs] + [np.zeros(0, np.uint8)])
    offs = np.zeros(len(subs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subs])
    return res, offs


# no C, H, P, W (tests/seam_support.py): the 16 lowest diagonal entries
ALPHABET = np.array([0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 18, 19], dtype=np.uint8)


def seam_query(n, seed):
    """No residue twice in a row: beside a doubled residue a gap run splits for
    free and can step round any one seam (tests/seam_support.py)."""
    rng = np.random.default_rng(seed)
    return ALPHABET[np.cumsum(rng.integers(1, len(ALPHABET), size=n)) % len(ALPHABET)]


def seam_subjects(q, seams):
    """Copies of q with L = 1, 2, 5 rows deleted (query rows against gaps: a
    run down the column) or L columns inserted (a run along the row) so that
    the run starts on, crosses and ends on each seam row."""
    ins = np.random.default_rng(4711)
    subs, seen = [], set()
    for s in seams:
        for L in (1, 2, 5):
            for p in (s, s - 1, s - L + 1):
                if p < 1 or p + L >= len(q) or (p, L) in seen:
                    continue
                seen.add((p, L))
                subs.append(np.concatenate([q[:p], q[p + L:]]))
                other = ALPHABET[(ALPHABET != q[p - 1]) & (ALPHABET != q[p])]
                subs.append(np.concatenate([q[:p], other[ins.integers(0, len(other), size=L)], q[p:]]))
    return subs
