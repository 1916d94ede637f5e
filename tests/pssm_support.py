"""Shared by the PSSM tests: tests/native/pssm_oracle.cpp compiled into a
temporary shared object (as test_plan.py builds plan_check) and its ctypes
face, the derived table of a sequence, and the score of a path under a table."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pssm_oracle.cpp")


class PssmOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libpssm_oracle.so")
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", SRC, "-o", so],
                       check=True, timeout=300)
        L = ctypes.CDLL(so)
        i8p, u8p = ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(ctypes.c_uint8)
        L.pso_scan.restype = None
        L.pso_scan.argtypes = [i8p, ctypes.c_int, u8p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.c_int,
                               ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
        L.pso_align.restype = ctypes.c_int
        L.pso_align.argtypes = [i8p, ctypes.c_int, u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
        self.L = L

    @staticmethod
    def _rows(rows):
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int8).reshape(-1, 25))
        return r, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))

    def scan(self, rows, residues, offsets, gap_open=2, gap_extend=None):
        r, rp = self._rows(rows)
        res = np.ascontiguousarray(residues, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.zeros(len(o) - 1, dtype=np.int32)
        self.L.pso_scan(rp, len(r), res.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                        o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(o) - 1, gap_open,
                        gap_open if gap_extend is None else gap_extend,
                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return out

    def align(self, rows, s, gap=2, gap_extend=None):
        """The dict oracle.align and Database.align return."""
        r, rp = self._rows(rows)
        s = np.ascontiguousarray(s, dtype=np.uint8)
        pos = (ctypes.c_int * 5)()
        cap = len(r) + len(s) + 1
        buf = ctypes.create_string_buffer(cap)
        best = self.L.pso_align(rp, len(r), s.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(s), gap,
                                gap if gap_extend is None else gap_extend, pos, buf, cap)
        return {"score": best, "q_end": pos[0], "s_end": pos[1], "q_begin": pos[2], "s_begin": pos[3],
                "ops": buf.raw[:pos[4]].decode()}


def derived(q, mat):
    """rows[i] = mat[q[i]]: the table a sequence stands for under a matrix."""
    m = np.asarray(mat, dtype=np.int8).reshape(25, 25)
    return np.ascontiguousarray(m[np.asarray(q, dtype=np.int64)], dtype=np.int8).reshape(-1, 25)


def path_score_pssm(rows, s, go, ge, al):
    """Score of an alignment's path under a table (conftest.path_score's rule
    for gaps), whatever the tie rules."""
    i, j, sc, prev = al["q_begin"] - 1, al["s_begin"] - 1, 0, None
    for op in al["ops"]:
        if op == "M":
            sc += int(rows[i][s[j]])
            i += 1
            j += 1
        else:
            sc -= ge if prev == op else go
            if op == "I":
                i += 1
            else:
                j += 1
        prev = op
    assert (i, j) == (al["q_end"], al["s_end"]), "the path ends at the end cell"
    return sc
