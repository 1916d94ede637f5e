"""What the seam probes (tests/seam_support.py) would see, proved on the CPU:
tests/native/seam_check.cpp restates the recurrence and mis-carries one
quantity across one row or column seam.

1. Without a fault it equals oracle.scan on every probe, twin and control
   subject under the five scorings.
2. For every seam of every row window and of the column window, every scoring
   and every fault observable under it, at least one probe's score changes.
   The faults: the gap state's carry (F down a column, E along a row) dropped,
   + ge, - ge; H as the gap's opening source dropped, + ge, - ge.  Exempt: the
   dropped and - ge carry where open <= extend (linear gaps and the
   open-below-extend scoring): H - go dominates the carried state in every
   cell there (seam_support.gap_state_dominated), no input can see them.
   Nothing else is exempt.  Every seam of the windows is run, not only the
   table's.
3. Every (form, gap model, seam kind) of seam_support.FORMS has a seam inside
   a row window, and the column window covers every residue mod 64.
4. Control (printed, not gated): random 400-residue subjects and a dropped or
   - ge F carry at rows 250..261 under the two affine scorings: how many
   (subject, row) pairs notice.  Measured: 11 of 1,440 (1 in 131).
5. Every probe's score is at least its gapped alignment's, which beats either
   flank alone: the flanks are long enough.

Time on the build machine: 12 s for the module (16 cores; the checker's
fault-free scores of 2,000 subjects x 5 scorings and its 9,000 faulty runs
spread over the cores take 6 s of it, the oracle's scans 1 s), so every seam
of the windows is run, not only the table's rows and their neighbours."""
import numpy as np
import pytest

import seam_support as ss


@pytest.fixture(scope="module")
def probes():
    return ss.build()


@pytest.fixture(scope="module")
def checked(probes, oracle, tmp_path_factory):
    """One run of the checker: the fault-free scores, the fault tasks of
    condition 2 and the control's."""
    tmp = tmp_path_factory.mktemp("seam")
    exe = ss.build_checker(tmp)
    mats = [oracle.matrix(0), oracle.matrix(1)]
    scorings = [(mid, go, ge) for mid, go, ge in ss.SCORINGS]
    tasks, labels = [], []
    for k, (mid, go, ge) in enumerate(ss.SCORINGS):
        dominated = ss.gap_state_dominated(go, ge)
        seams = [("r", s) for lo, hi, _, _ in ss.ROW_WINDOWS for s in range(lo, hi + 1)]
        seams += [("c", s) for s in range(ss.COL_WINDOW[0], ss.COL_WINDOW[1] + 1)]
        for axis, s in seams:
            for fault in range(6):
                if dominated and fault in (0, 2):
                    continue
                across = ss.candidates(probes.meta, axis, s, fault, dominated)
                tasks.append((k, 0 if axis == "r" else 1, s, fault, across))
                labels.append(("probe", k, axis, s, fault))
    randoms = [k for k, m in enumerate(probes.meta) if m[3] == "random"]
    for k, (mid, go, ge) in enumerate(ss.SCORINGS):
        if ss.gap_state_dominated(go, ge):
            continue
        for s in range(250, 262):
            for fault in (0, 2):
                for r in randoms:
                    tasks.append((k, 0, s, fault, [r]))
                    labels.append(("control", k, r, s, fault))
    base, out = ss.run_checker(exe, tmp, mats, scorings, probes.q, probes.subs, tasks)
    return mats, base, tasks, labels, out


def test_restatement_equals_oracle(probes, oracle, checked):
    mats, base, _, _, _ = checked
    for k, (mid, go, ge) in enumerate(ss.SCORINGS):
        want = oracle.scan(probes.q, probes.res, probes.offs, mat=mats[mid], gap_open=go, gap_extend=ge)
        bad = np.nonzero(base[k] != want)[0]
        assert bad.size == 0, ((mid, go, ge), bad[:10], base[k][bad[:10]], want[bad[:10]])


def test_gapped_alignment_is_the_optimum(probes, checked):
    """Each probe's score is the copy's score less the gap, or better: the
    flanks are long enough that the gapped alignment beats either flank alone
    (a probe the DP scores through one flank only would see no seam)."""
    mats, base, _, _, _ = checked
    for k, (mid, go, ge) in enumerate(ss.SCORINGS):
        diag = np.diag(mats[mid]).astype(np.int64)[probes.q]
        for j, (axis, p, L, kind) in enumerate(probes.meta):
            if kind != "probe":
                continue
            lo, hi = (p, p + L) if axis == "r" else (p, p)
            gapped = diag[:lo].sum() + diag[hi:].sum() - min(go + (L - 1) * ge, L * go)
            assert base[k][j] >= gapped > max(diag[:lo].sum(), diag[hi:].sum()), ((mid, go, ge), axis, p, L)


def test_every_fault_is_seen_at_every_seam(probes, checked):
    _, _, tasks, labels, out = checked
    missed, n = [], 0
    for (k, axis, seam, fault, idx), lab, (hit, _, tried) in zip(tasks, labels, out):
        if lab[0] != "probe":
            continue
        n += 1
        assert idx, ("no probe lies across", lab)
        if hit < 0:
            missed.append((ss.SCORINGS[k], "row" if axis == 0 else "column", seam, ss.FAULTS[fault], tried))
    assert n > 3000
    assert not missed, (len(missed), missed[:20])


def test_seam_table_and_windows():
    for name, (layout, qlen, gaps, opts, shape_of) in ss.FORMS.items():
        for g in gaps:
            shape = shape_of(g == "a")
            table = ss.row_seams(shape, qlen)
            for kind in ss.required_kinds(shape, qlen):
                assert ss.in_windows(table.get(kind, [])), (name, g, kind, table.get(kind))
    # RI 16 and 20: one chunk holds the query (the docstring's statement)
    assert 64 * 16 > ss.QLEN and "chunk" not in ss.row_seams(("intra", 20), ss.QLEN)
    assert "chunk" in ss.row_seams(("intra", 4), ss.QLEN) and "chunk" in ss.row_seams(("intra", 8), ss.QLEN)
    # the short last pass of both pass heights (29 .. 56 rows left of 64)
    assert ss.short_rows(ss.QLEN, 64) == (28, 512) and ss.short_rows(ss.QLEN, 96) == (44, 480)
    lo, hi = ss.COL_WINDOW
    assert hi - lo + 1 >= 72
    # every long run starts at, and ends on, every residue mod 64
    assert {c % 64 for c in range(lo, hi + 1)} == set(range(64))
    # the scaled scorings stay inside the API's entries and the admission bound
    for mid, k, go, ge in ss.RESCUE_SCORINGS:
        mx = {0: 15, 1: 11}[mid] * k
        assert mx <= 100 and 2 * mx + 27 * ge + go < 1024


def test_probe_layout(probes):
    lens = np.diff(probes.offs)
    kinds = np.array([m[3] for m in probes.meta])
    assert lens[kinds == "probe"].max() < ss.SPLIT_THRESHOLD < lens[kinds == "twin"].min()
    assert lens[kinds != "random"].min() > 64
    assert 1000 <= len(lens) <= 2600, len(lens)
    assert probes.res.max() < 20


def test_control_random_subjects(checked, capsys):
    """Recorded, not gated: how seldom a random subject notices."""
    _, _, _, labels, out = checked
    pairs = {}
    for lab, (hit, _, _) in zip(labels, out):
        if lab[0] == "control":
            key = (lab[1], lab[2], lab[3])
            pairs[key] = pairs.get(key, False) or hit >= 0
    seen = sum(pairs.values())
    with capsys.disabled():
        print("\nSEAM CONTROL: %d of %d (random subject, row) pairs notice a dropped or -ge F carry"
              % (seen, len(pairs)))
    assert len(pairs) == 2 * 12 * ss.N_RANDOM
