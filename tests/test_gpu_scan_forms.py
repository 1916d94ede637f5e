"""The form every scan takes (swplan::scan_plan, sw_plan.cpp), pinned to a
recording: for a matrix of databases, scorings, query lengths and sw_opts,
the kernel names the handle reports, the launch count, the block counts of
the coop / pair forms and a checksum of the scores must equal
tests/golden/scan_forms.json, which was recorded before the scan driver was
split into the plan and its enqueue stages.  A change of the plan that is
meant to change a form re-records the file (record(), below) and says so."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

FORMS = os.path.join(GOLDEN, "scan_forms.json")

B62 = (1, 12, 1)   # (builtin matrix, gap open, gap extend): affine
B50 = (0, 2, 2)    # linear
QLENS = (0, 40, 64, 96, 97, 200, 375, 500, 1400)
# no case depends on event timing: the adaptive routes are forced, except
# in the cases made for them
BASE = dict(pair_width=64, intra_i16_first=0, inter_i16_span=0)


def cases():
    """(name, database, sw_opts overrides, scoring, query length)"""
    out = []

    def add(tag, dbname, opts, scoring, qlens):
        for qlen in qlens:
            name = "%s/%s/m%d_%d_%d/q%d" % (tag, dbname, *scoring, qlen)
            out.append((name, dbname, dict(BASE, **opts), scoring, qlen))

    for sc in (B62, B50):
        add("default", "mixed", {}, sc, QLENS)
        add("lpt0", "mixed", {"lpt": 0}, sc, QLENS)
        add("lpt1", "mixed", {"lpt": 1}, sc, (64, 97, 375, 1400))
        add("tri0", "mixed", {"tri_width": 0}, sc, (97, 200, 375, 500))
        add("tail8", "mixed", {"tail_pairs": 8, "pair_width": 256}, sc, (200, 375))
        add("ix2_0", "mixed", {"intra_x2": 0}, sc, (40, 200, 500))
        # past the static int16 bound (qlen + 2) * (max S + go) < 32767
        add("guard0", "mixed", {"int16_guard": 0}, sc, (500, 2000))
        add("guard1", "mixed", {}, sc, (2000,))
        add("y32x8", "mixed", {"inter_variant": "y32x8"}, sc, (40, 200, 500))
        add("32x8", "mixed", {"inter_variant": "32x8"}, sc, (40, 200, 500))
        add("span5", "mixed", {"inter_i16_span": 5}, sc, (40, 200, 500))
        add("i16first", "mixed", {"intra_i16_first": 1}, sc, (40, 200, 500))
        add("default", "short", {}, sc, (40, 97, 375, 1400))
        add("default", "long", {}, sc, (40, 200, 500, 1400))
        add("rows20", "long", {"intra_x2_rows": 20}, sc, (200, 1400))
    # a linear scoring whose matrix + gap does not fit the int8 profile: the
    # affine kernels (BLOSUM62's largest entry is 11)
    add("bias", "mixed", {}, (1, 120, 120), (40, 200))
    return out


def databases(sw, handle):
    """mixed: the merged-launch tests' shape (2,500 synthetic subjects and
    three planted near-copies of the query, long above 700); short: its
    subjects up to 700 residues only; long: every subject a long one."""
    r, o = sw.synth.database(2500, shard=23)
    q0 = sw.synth.query(2000, shard=8)
    extra = [q0[:500], q0[:300], np.concatenate([q0[:500], q0[:500]])]
    subj = [r[o[k]:o[k + 1]] for k in range(len(o) - 1)] + extra

    def make(sel, thr):
        res = np.concatenate(sel)
        offs = np.zeros(len(sel) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(s) for s in sel])
        return sw.Database(handle, res, offs, long_threshold=thr)

    return q0, {"mixed": make(subj, 700),
                "short": make([s for s in subj if len(s) <= 700], 700),
                "long": make([s for s in subj[:600] + extra if len(s) > 64], 64)}


def run(sw, handle):
    """Every case's record, in the order of cases()."""
    saved = handle.get_opts()
    q0, dbs = databases(sw, handle)
    mats = {mid: sw.capi.builtin_matrix(mid) for mid in (0, 1)}
    out = {}
    try:
        for name, dbname, opts, (mid, go, ge), qlen in cases():
            handle.set_opts(saved, **opts)
            db = dbs[dbname]
            scores = db.scan(q0[:qlen], mats[mid], go, ge)
            st = db.stats()
            out[name] = {"last_kernel": handle.last_kernel(),
                         "last_intra_kernel": handle.last_intra_kernel(),
                         "launches": handle.timing()["launches"],
                         "coop_blocks": st["coop_blocks"],
                         "pair_blocks": st["pair_blocks"],
                         "pair_merged": st["pair_merged"],
                         "scores_crc32": zlib.crc32(np.ascontiguousarray(scores, dtype=np.int32).tobytes())}
    finally:
        handle.set_opts(saved)
        for db in dbs.values():
            db.close()
    return out


def record(sw, handle, path=FORMS):
    with open(path, "w") as f:
        json.dump(run(sw, handle), f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def forms(sw, handle):
    return run(sw, handle)


@pytest.mark.gpu
def test_scan_forms_equal_the_recording(forms):
    with open(FORMS) as f:
        want = json.load(f)
    assert sorted(forms) == sorted(want), "the matrix of cases and the recording differ"
    diff = {k: (forms[k], want[k]) for k in want if forms[k] != want[k]}
    assert not diff, "%d of %d cases differ, e.g. %s" % (len(diff), len(want), sorted(diff.items())[:3])


@pytest.mark.gpu
def test_scan_forms_cover_every_form(forms):
    """The matrix is worth replaying only while it reaches each form."""
    names = " ".join(r["last_kernel"] for r in forms.values())
    for part in ("none", "+lpt+drain", "+tri", "+tail", "<48,", "+int16[0,5)", "sw_inter_x2p<", "sw_inter_x2s<32,8,affine>",
                 "sw_inter<32,8,affine>", "sw_inter<64,8,linear>", "sw_inter<32,8,linear>"):
        assert part in names, part
    intra = " ".join(r["last_intra_kernel"] for r in forms.values())
    for part in ("sw_intra_x2<20>", ",int16>", "sw_intra<"):
        assert part in intra, part
    assert forms["bias/mixed/m1_120_120/q200"]["last_kernel"] == "sw_inter<32,8,affine>"
    assert any(r["coop_blocks"] for r in forms.values())
