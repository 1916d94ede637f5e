"""Argument errors of the C ABI (include/sw_amd.h), as one table of (entry
point, bad argument, expected code): what a caller sees for a bad call is part
of the interface, whichever translation unit of the host driver checks it.

CPU half: every exported function that takes a handle, a database or a PSSM
returns SW_E_INVALID for null with a message, except the three that release
(null is "nothing to release") and the three that return a pointer.  (Seven
of these rows are test_abi.py's and test_opts.py's.)

GPU half: on a live handle, a three-subject database (lengths 0, 5, 70), a
4-residue query and a 4-row PSSM, every row returns SW_E_INVALID; afterwards a
plain scan on the same handle equals the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from hits_support import pack

SW_E_INVALID = -1
I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)
U8P = ctypes.POINTER(ctypes.c_uint8)


def object_functions():
    """name -> parameter text of every declared function with a sw_handle*,
    sw_db* or sw_pssm* parameter (not the `out` double pointers alone)."""
    src = open(os.path.join(REPO, "include", "sw_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"SW_API\s+[^;(]*?\b(sw_\w+)\s*\(([^)]*)\)\s*;", src, re.S):
        if re.search(r"\bsw_(handle|db|pssm)\s*\*(?!\*)", params):
            out[name] = params
    return out


# null is not an error for these: (entry point, what it returns)
NULL_IS_FINE = {"sw_destroy": 0, "sw_db_free": 0, "sw_pssm_free": 0,
                "sw_stream": None, "sw_last_kernel": b"none", "sw_last_intra_kernel": b"none"}


# rows that tests/test_abi.py (test_null_arguments_are_errors_not_crashes) and
# tests/test_opts.py (test_set_opts_argument_errors) already hold
HELD_ELSEWHERE = {"sw_db_create", "sw_scan", "sw_get_timing", "sw_destroy", "sw_set_opts", "sw_get_opts",
                  "sw_db_reset_adaptive"}


def other_error(L):
    """Leave a known message in sw_last_error() and return it: a message read
    after the next call that differs from it is that call's."""
    buf = (ctypes.c_int8 * 625)()
    assert L.sw_builtin_matrix(99, buf) == SW_E_INVALID
    assert L.sw_last_error() == b"unknown matrix id"
    return L.sw_last_error()


def null_args(fn):
    plain = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64)
    return [0 if t in plain else None for t in fn.argtypes]


def test_the_table_covers_the_header():
    names = object_functions()
    assert len(names) >= 48 and set(NULL_IS_FINE) | HELD_ELSEWHERE <= set(names)
    for n in ("sw_scan", "sw_db_save", "sw_pssm_length", "sw_scan_batch_hits_sig", "sw_score_hist", "sw_set_opts"):
        assert n in names
    assert not [n for n in names if n.startswith("sw_group")]


@pytest.mark.parametrize("name", sorted(set(object_functions()) - HELD_ELSEWHERE))
def test_null_object_is_invalid(sw, name):
    L = sw.capi.lib()
    fn = getattr(L, name)
    other = other_error(L)
    got = fn(*null_args(fn))
    if name in NULL_IS_FINE:
        assert got == NULL_IS_FINE[name]
        return
    assert got == SW_E_INVALID
    assert L.sw_last_error() and L.sw_last_error() != other


# ---- the GPU half ---------------------------------------------------------------
def ptr(a, t):
    return a.ctypes.data_as(t)


@pytest.mark.gpu
def test_bad_arguments_on_a_live_handle(sw, oracle, handle):
    torch = pytest.importorskip("torch")
    capi = sw.capi
    L = capi.lib()
    rng = np.random.default_rng(5)
    subs = [rng.integers(0, 20, size=n).astype(np.uint8) for n in (0, 5, 70)]
    res, offs = pack(subs)
    db = sw.Database(handle, res, offs)
    q = rng.integers(0, 20, size=4).astype(np.uint8)
    pssm = sw.Pssm(handle, rng.integers(-4, 8, size=(4, 25)).astype(np.int8))
    h, d, p = handle.ptr, db.ptr, pssm.ptr
    qp = ptr(q, U8P)
    scoring = capi._ScoringArg(capi.builtin_matrix(1), 11, 1)  # (alive for the table: it holds the matrix)
    sc = scoring.ptr()

    keys = np.zeros(2 * 4097, dtype=np.int64)
    scores = np.zeros(8, dtype=np.int32)
    hits = (capi.Hit * (2 * 4097))()
    sigs = (capi.Sig * (2 * 4097))()
    cal = (capi.Calib * 2)()
    nhits = ctypes.c_int32(0)
    als = (capi.Alignment * 4)()
    ops = ctypes.create_string_buffer(4 * 128)
    dev = torch.zeros(16, dtype=torch.int32, device="cuda")
    dkeys = torch.zeros(4097, dtype=torch.int64, device="cuda")
    kp, sp, nh = ptr(keys, I64P), ptr(scores, I32P), ctypes.byref(nhits)
    dv, dk = ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(dkeys.data_ptr())

    # two queries of the batch forms: q twice
    qq = np.concatenate([q, q])
    qqp = ptr(qq, U8P)
    good = np.array([0, 4, 8], dtype=np.int64)
    decreasing = np.array([0, 4, 3], dtype=np.int64)
    too_long = np.array([0, 4, 4 + (1 << 24) + 1], dtype=np.int64)  # by the offsets alone: never read that far

    def offp(a):
        return ptr(a, I64P)

    ids = np.array([1, 2], dtype=np.int32)
    absent = np.array([1, 3], dtype=np.int32)
    qidx = np.array([0, 1], dtype=np.int32)
    idp, abp = ptr(ids, I32P), ptr(absent, I32P)

    rows = []

    def row(what, call):
        rows.append((what, call))

    for k in (0, 4097):
        row("sw_scan_topk k=%d" % k, lambda k=k: L.sw_scan_topk(h, d, qp, 4, sc, k, kp))
        row("sw_scan_pssm_topk k=%d" % k, lambda k=k: L.sw_scan_pssm_topk(h, d, p, 11, 1, k, kp))
        row("sw_scan_pssm_topk_calib k=%d" % k, lambda k=k: L.sw_scan_pssm_topk_calib(h, d, p, 11, 1, k, kp, cal))
        row("sw_scan_batch_topk k=%d" % k, lambda k=k: L.sw_scan_batch_topk(h, d, qqp, offp(good), 2, sc, k, kp))
        row("sw_scan_hits k=%d" % k, lambda k=k: L.sw_scan_hits(h, d, qp, 4, sc, k, hits, nh))
        row("sw_scan_hits_sig k=%d" % k, lambda k=k: L.sw_scan_hits_sig(h, d, qp, 4, sc, k, hits, sigs, nh, cal))
        row("sw_scan_batch_hits k=%d" % k,
            lambda k=k: L.sw_scan_batch_hits(h, d, qqp, offp(good), 2, sc, k, hits, nh))
        row("sw_scan_batch_hits_sig k=%d" % k,
            lambda k=k: L.sw_scan_batch_hits_sig(h, d, qqp, offp(good), 2, sc, k, hits, sigs, nh, cal))
        row("sw_scan_rank_device k=%d" % k, lambda k=k: L.sw_scan_rank_device(h, d, qp, 4, sc, dv, k, None, 0, dk))
        row("sw_topk_device k=%d" % k, lambda k=k: L.sw_topk_device(h, dv, 3, 0, k, dk))
        row("sw_topk_device_ids k=%d" % k, lambda k=k: L.sw_topk_device_ids(h, dv, 3, dv, k, dk))
        row("sw_topk_keys_device k=%d" % k, lambda k=k: L.sw_topk_keys_device(h, dk, 3, k, dk))

    for what, o, nq in (("nq < 0", good, -1), ("decreasing qoffsets", decreasing, 2),
                        ("a query longer than 2^24", too_long, 2)):
        row("sw_scan_batch " + what, lambda o=o, nq=nq: L.sw_scan_batch(h, d, qqp, offp(o), nq, sc, sp))
        row("sw_scan_batch_device " + what, lambda o=o, nq=nq: L.sw_scan_batch_device(h, d, qqp, offp(o), nq, sc, dv))
        row("sw_scan_batch_topk " + what, lambda o=o, nq=nq: L.sw_scan_batch_topk(h, d, qqp, offp(o), nq, sc, 2, kp))
        row("sw_hit_stats_batch " + what,
            lambda o=o, nq=nq: L.sw_hit_stats_batch(h, d, qqp, offp(o), nq, sc, ptr(qidx, I32P), idp, 2, hits))
        row("sw_scan_batch_hits " + what,
            lambda o=o, nq=nq: L.sw_scan_batch_hits(h, d, qqp, offp(o), nq, sc, 2, hits, nh))
        row("sw_scan_batch_hits_sig " + what,
            lambda o=o, nq=nq: L.sw_scan_batch_hits_sig(h, d, qqp, offp(o), nq, sc, 2, hits, sigs, nh, cal))

    for bad in ([0, -1], [2, 0]):
        bq = np.array(bad, dtype=np.int32)
        row("sw_hit_stats_batch qidx %r" % bad,
            lambda bq=bq: L.sw_hit_stats_batch(h, d, qqp, offp(good), 2, sc, ptr(bq, I32P), idp, 2, hits))

    row("sw_align id not in the database", lambda: L.sw_align(h, d, qp, 4, sc, abp, 2, als, ops, 128))
    row("sw_align_pssm id not in the database", lambda: L.sw_align_pssm(h, d, p, 11, 1, abp, 2, als, ops, 128))
    row("sw_hit_stats id not in the database", lambda: L.sw_hit_stats(h, d, qp, 4, sc, abp, 2, hits))
    row("sw_hit_stats_batch id not in the database",
        lambda: L.sw_hit_stats_batch(h, d, qqp, offp(good), 2, sc, ptr(qidx, I32P), abp, 2, hits))
    for stride in (0, -128):
        row("sw_align ops_stride %d" % stride, lambda s=stride: L.sw_align(h, d, qp, 4, sc, idp, 2, als, ops, s))
        row("sw_align_pssm ops_stride %d" % stride,
            lambda s=stride: L.sw_align_pssm(h, d, p, 11, 1, idp, 2, als, ops, s))
    row("sw_scan_hits_sig null sig", lambda: L.sw_scan_hits_sig(h, d, qp, 4, sc, 2, hits, None, nh, cal))
    for go, ge in ((0, 1), (11, 0)):
        row("sw_scan_pssm gaps %d/%d" % (go, ge), lambda go=go, ge=ge: L.sw_scan_pssm(h, d, p, go, ge, sp))
        row("sw_scan_pssm_device gaps %d/%d" % (go, ge),
            lambda go=go, ge=ge: L.sw_scan_pssm_device(h, d, p, go, ge, dv))
        row("sw_scan_pssm_topk gaps %d/%d" % (go, ge),
            lambda go=go, ge=ge: L.sw_scan_pssm_topk(h, d, p, go, ge, 2, kp))
        row("sw_scan_pssm_topk_calib gaps %d/%d" % (go, ge),
            lambda go=go, ge=ge: L.sw_scan_pssm_topk_calib(h, d, p, go, ge, 2, kp, cal))
        row("sw_align_pssm gaps %d/%d" % (go, ge),
            lambda go=go, ge=ge: L.sw_align_pssm(h, d, p, go, ge, idp, 2, als, ops, 128))
    opts = handle.get_opts()
    for size in (0, ctypes.sizeof(capi.Opts) - 4, ctypes.sizeof(capi.Opts) + 4):
        wrong = capi.Opts()
        ctypes.memmove(ctypes.byref(wrong), ctypes.byref(opts), ctypes.sizeof(capi.Opts))
        wrong.size = size
        row("sw_set_opts size %d" % size, lambda w=wrong: L.sw_set_opts(h, ctypes.byref(w)))

    assert len(rows) == 12 * 2 + 6 * 3 + 2 + 4 + 4 + 1 + 10 + 3
    for what, call in rows:
        other = other_error(L)
        rc = call()
        assert rc == SW_E_INVALID, (what, rc, L.sw_last_error())
        assert L.sw_last_error() and L.sw_last_error() != other, what
    assert handle.get_opts().as_dict() == opts.as_dict()

    # the handle and the database are as usable as before
    m = capi.builtin_matrix(1)
    assert np.array_equal(db.scan(q, m, 11, 1), oracle.scan(q, res, offs, m, 11, 1))
    pssm.close()
    db.close()
