#!/usr/bin/env python3
"""Wall time of the hit table against the traceback on C2's shape (DESIGN.md
§4 "Hit table"): Database.synthetic, 570,000 subjects, the 375-aa query
P07327, BLOSUM62 11/1, K = 100 and K = 4096 top hits.

Timed per K, median of five calls after one warm-up, through the C ABI with
preallocated outputs:
  sw_hit_stats   the rows of the K ids
  sw_align       the same ids with ops = NULL (coordinates only)
  sw_scan_hits   scan + top-K + rows
  sw_scan_topk   scan + top-K
and the rows are checked against sw_align's coordinates.  Prints one JSON
line; --out FILE also writes it there.

  python scripts/hits_timing.py [--subjects 570000] [--out profiles/r11_hits/timing.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import _swpkg  # noqa: E402


def median_ms(fn, reps=5):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=570000)
    ap.add_argument("--seed", type=int, default=1782)
    ap.add_argument("--query", default="P07327")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sw = _swpkg.load()
    capi = sw.capi
    L = capi.lib()
    with open(os.path.join(REPO, "tests", "golden", "queries", args.query + ".fasta")) as f:
        q = sw.encode("".join(f.read().split("\n")[1:]))
    h = sw.Handle(0, env_opts=False)
    db = sw.Database.synthetic(h, args.seed, args.subjects)
    sc = capi._ScoringArg(capi.builtin_matrix(capi.MATRIX_BLOSUM62), 11, 1)
    q, qp = capi._u8(q)
    i32p = ctypes.POINTER(ctypes.c_int32)
    res = {"subjects": args.subjects, "query": args.query, "qlen": len(q), "scoring": "BLOSUM62 11/1", "k": {}}
    for k in (100, 4096):
        keys = np.zeros(k, dtype=np.int64)
        keysp = keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        capi._check(L.sw_scan_topk(h.ptr, db._d, qp, len(q), sc.ptr(), k, keysp))
        ids = np.ascontiguousarray(capi.decode_keys(keys)[0], dtype=np.int32)
        idp = ids.ctypes.data_as(i32p)
        rows = (capi.Hit * k)()
        als = (capi.Alignment * k)()
        nh = ctypes.c_int32(0)
        t = {}
        t["sw_hit_stats_ms"], t["sw_hit_stats_all"] = median_ms(
            lambda: capi._check(L.sw_hit_stats(h.ptr, db._d, qp, len(q), sc.ptr(), idp, k, rows)))
        t["sw_align_ms"], t["sw_align_all"] = median_ms(
            lambda: capi._check(L.sw_align(h.ptr, db._d, qp, len(q), sc.ptr(), idp, k, als, None, 0)))
        for r, a in zip(rows, als):
            got = (r.score, r.q_begin, r.q_end, r.s_begin, r.s_end, r.length)
            want = (a.score, a.q_begin, a.q_end, a.s_begin, a.s_end, a.ops_len) if a.score else (0,) * 6
            assert got == want, (r.id, got, want)
        t["sw_scan_hits_ms"], _ = median_ms(
            lambda: capi._check(L.sw_scan_hits(h.ptr, db._d, qp, len(q), sc.ptr(), k, rows, ctypes.byref(nh))))
        t["sw_scan_topk_ms"], _ = median_ms(
            lambda: capi._check(L.sw_scan_topk(h.ptr, db._d, qp, len(q), sc.ptr(), k, keysp)))
        t["hit_stats_not_slower_than_align"] = t["sw_hit_stats_ms"] <= t["sw_align_ms"]
        res["k"][str(k)] = t
    db.close()
    h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
