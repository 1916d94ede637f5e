"""PSSM text files, mirroring sw_solver_read_pssm (csrc/swsolver.cpp; the
format is stated in include/sw_solver_ext.h) as fasta.py mirrors the FASTA
parsers: the same table, the same consensus and the same error words.

    rows, consensus = read_pssm(path)     # int8 [positions][25], str

* Blank lines, lines starting with '#', and every line before the header are
  ignored.
* The header is the first line whose tokens are all single residue letters;
  its columns are the leading run of distinct letters, stopping at the first
  repeat (an NCBI ASCII PSSM repeats its 20 letters).
* Each following line is one position: an optional integer position, an
  optional residue letter (the consensus), then at least one integer per
  column; further tokens are ignored.  Without a letter, a leading position
  is recognised by the line holding more tokens than the header has columns.
  The first line that is not such a row ends the table.
* Unnamed columns: B, Z, J take floor((a + b) / 2) of N/D, Q/E, I/L when both
  are named; every other one takes X when X is named, else the row's minimum.

`derived(query_codes, matrix)` is the table a residue sequence stands for
under a 25 x 25 matrix (rows[i] = matrix[q[i]]): its scan equals the
sequence's, bit for bit.
"""
import re

import numpy as np

LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"  # code order (SWSolver.cu:17-41)
_INT = re.compile(r"[+-]?[0-9]+\Z")
_PAIRS = ((20, 2, 3), (22, 5, 6), (21, 9, 10))  # B: N D, Z: Q E, J: I L
_X = 23


class PSSMError(ValueError):
    pass


def _is_letter(t):
    return len(t) == 1 and (t.isascii() and t.isalpha() or t == "*")


def read_pssm(path):
    """(rows int8 [positions][25], consensus str); PSSMError on a bad file."""
    def bad(why):
        return PSSMError("%s: %s" % (path, why))

    try:
        with open(path, "rb") as f:
            lines = f.read().decode("latin-1").split("\n")
    except OSError:
        raise bad("cannot open PSSM file")
    col, named, header = [], [False] * 25, False
    rows, cons_out = [], []
    for line in lines:
        tok = line.split()
        if not tok or tok[0][0] == "#":
            continue
        if not header:
            if not all(_is_letter(t) for t in tok):
                continue
            for t in tok:
                c = LETTERS.find(t.upper())
                if c < 0:
                    raise bad("unknown residue letter '%s' in the header" % t)
                if named[c]:
                    break
                named[c] = True
                col.append(c)
            header = True
            continue
        at, pos, cons = 0, False, -1
        if len(tok) >= 2 and _INT.match(tok[0]) and _is_letter(tok[1]):
            pos, at = True, 1
        if at < len(tok) and _is_letter(tok[at]):
            cons = LETTERS.find(tok[at].upper())
            if cons < 0:
                raise bad("unknown residue letter '%s'" % tok[at])
            at += 1
        elif _INT.match(tok[0]) and len(tok) > len(col):
            pos, at = True, 1
        if at >= len(tok):
            if pos:
                raise bad("short row '%s'" % line)
            break
        if not _INT.match(tok[at]):
            break
        if len(tok) - at < len(col):
            raise bad("short row %d: %d of %d entries" % (len(rows) + 1, len(tok) - at, len(col)))
        v = [0] * 25
        for j, c in enumerate(col):
            t = tok[at + j]
            if not _INT.match(t):
                raise bad("bad entry '%s' in row %d" % (t, len(rows) + 1))
            x = int(t)
            if x < -100 or x > 100:
                raise bad("entry '%s' outside -100..100 in row %d" % (t, len(rows) + 1))
            v[c] = x
        lo = min(v[c] for c in col)
        have = list(named)
        for b, x, y in _PAIRS:
            if not named[b] and named[x] and named[y]:
                v[b] = (v[x] + v[y]) // 2
                have[b] = True
        for c in range(25):
            if not have[c]:
                v[c] = v[_X] if named[_X] else lo
        if cons < 0:
            for c in range(25):
                if named[c] and (cons < 0 or v[c] > v[cons]):
                    cons = c
        rows.append(v)
        cons_out.append(LETTERS[cons])
    if not header:
        raise bad("no header line of residue letters")
    if not rows:
        raise bad("no rows after the header")
    return np.array(rows, dtype=np.int8).reshape(-1, 25), "".join(cons_out)


def derived(query_codes, matrix):
    """rows[i] = matrix[q[i]]: the PSSM of a residue sequence under a matrix."""
    m = np.asarray(matrix, dtype=np.int8).reshape(25, 25)
    q = np.asarray(query_codes, dtype=np.int64)
    return np.ascontiguousarray(m[q], dtype=np.int8).reshape(-1, 25)


def write_pssm(path, rows, consensus=None):
    """A 25-column file read_pssm reads back as `rows` (tests, examples)."""
    r = np.asarray(rows).reshape(-1, 25)
    with open(path, "w") as f:
        f.write("# position-specific scoring matrix, %d positions\n" % len(r))
        f.write("      " + " ".join("%4s" % c for c in LETTERS) + "\n")
        for i, row in enumerate(r):
            c = consensus[i] if consensus else LETTERS[int(np.argmax(row))]
            f.write("%4d %s " % (i + 1, c) + " ".join("%4d" % int(x) for x in row) + "\n")
