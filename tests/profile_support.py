"""numpy model of the iterated profile search (include/sw_amd.h "iterated
profile search"): the query-anchored rows replayed from an alignment's ops,
the integer profile tables, the step from tables to a PSSM, and the loop.
tests/test_profile_cpu.py and tests/test_gpu_profile.py compare the library
against these.

The tables are integers (exact).  The PSSM's entries are rounded doubles: the
model also returns the unrounded values, and a test first asserts that none
of ITS inputs' values lies within 1e-6 of a half-integer (two correct double
evaluations differ by ~1e-13 there), then compares exactly."""
import numpy as np

import calib_support as cs
import rank_support as rs

GAP, NONE, CODES, ALPHABET = 25, 26, 20, 25
ONE = 1 << 30
# Swiss-Prot composition (percent), codes 0..19 (the package's synth.SWISSPROT_FREQ;
# restated so that the model stands on its own)
FREQ = np.array([8.25, 5.53, 4.06, 5.45, 1.37, 3.93, 6.75, 7.07, 2.27, 5.96,
                 9.66, 5.84, 2.42, 3.86, 4.70, 6.56, 5.34, 1.08, 2.92, 6.87])


def background():
    return FREQ / FREQ.sum()


# ---- step 1: rows ------------------------------------------------------------
def row_of(qlen, s, al):
    """The row of one alignment (a dict with q_begin, s_begin 1-based and ops,
    as PssmOracle.align returns): M -> the subject's code, I -> GAP, D dropped,
    NONE elsewhere."""
    row = np.full(qlen, NONE, dtype=np.uint8)
    if al["score"] <= 0:
        return row
    i, j = al["q_begin"] - 1, al["s_begin"] - 1
    for op in al["ops"]:
        if op == "M":
            row[i] = s[j]
            i += 1
            j += 1
        elif op == "I":
            row[i] = GAP
            i += 1
        else:
            j += 1
    return row


def msa_of(qlen, master, subjects, aligns):
    rows = [np.full(qlen, NONE, dtype=np.uint8) if master is None else np.asarray(master, dtype=np.uint8)]
    rows += [row_of(qlen, s, al) for s, al in zip(subjects, aligns)]
    return np.array(rows, dtype=np.uint8).reshape(len(rows), qlen)


# ---- step 2: tables ----------------------------------------------------------
def tables(msa):
    """(cnt uint32 [qlen][20], weight uint64 [nrows], wsum uint64 [qlen][20])."""
    msa = np.asarray(msa, dtype=np.uint8)
    nrows, qlen = msa.shape
    counted = msa < CODES
    code = np.where(counted, msa, 0).astype(np.int64)
    cnt = np.zeros((qlen, CODES), dtype=np.int64)
    for a in range(CODES):
        cnt[:, a] = (msa == a).sum(axis=0)
    k = (cnt > 0).sum(axis=1)
    term = np.zeros((qlen, CODES), dtype=np.int64)
    nz = cnt > 0
    term[nz] = ONE // (np.broadcast_to(k[:, None], cnt.shape)[nz] * cnt[nz])
    t = term[np.arange(qlen)[None, :], code] * counted  # [nrows][qlen]
    u = t.sum(axis=1)
    cov = counted.sum(axis=1)
    weight = np.where(cov > 0, u // np.maximum(cov, 1), 0).astype(np.int64)
    wsum = np.zeros((qlen, CODES), dtype=np.int64)
    for a in range(CODES):
        wsum[:, a] = (weight[:, None] * (msa == a)).sum(axis=0)
    return cnt.astype(np.uint32), weight.astype(np.uint64), wsum.astype(np.uint64)


# ---- step 3: from tables to a PSSM ----------------------------------------------
def _lambda_f(m, p, lam):
    return float((np.outer(p, p) * np.exp(lam * m)).sum() - 1.0)


def matrix_lambda(mat):
    """The positive root of sum p_a p_b exp(lambda s[a][b]) = 1 (None: none),
    by the header's bisection."""
    m = np.asarray(mat, dtype=np.float64).reshape(25, 25)[:CODES, :CODES]
    p = background()
    if not (np.outer(p, p) * m).sum() < 0 or not (m > 0).any():
        return None
    hi = 1.0
    while not _lambda_f(m, p, hi) > 0:
        hi *= 2
    lo = hi
    while not _lambda_f(m, p, lo) < 0:
        lo *= 0.5
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return lo
        if _lambda_f(m, p, mid) > 0:
            hi = mid
        else:
            lo = mid


def pssm_from_counts(cnt, wsum, prior_rows, mat, pseudo=10.0):
    """(rows int8 [qlen][25], raw): raw[i][a] is the unrounded entry (NaN where
    the prior is carried over)."""
    cnt = np.asarray(cnt, dtype=np.int64).reshape(-1, CODES)
    wsum = np.asarray(wsum, dtype=np.uint64).reshape(-1, CODES)
    prior = np.asarray(prior_rows, dtype=np.int8).reshape(-1, ALPHABET)
    m = np.asarray(mat, dtype=np.float64).reshape(25, 25)[:CODES, :CODES]
    lam = matrix_lambda(mat)
    assert lam is not None
    p = background()
    e = np.exp(lam * m)  # [b][a], b the query-side code
    rows = prior.copy()
    raw = np.full((len(cnt), CODES), np.nan)
    for i in range(len(cnt)):
        T = int(wsum[i].astype(object).sum())
        if T == 0:
            continue
        f = np.array([int(w) / T for w in wsum[i]], dtype=np.float64)
        alpha = max(int((cnt[i] > 0).sum()), 1) - 1
        g = p * (f @ e)
        Q = (alpha * f + pseudo * g) / (alpha + pseudo)
        raw[i] = np.log(Q / p) / lam
        # llround: half away from zero
        r = np.where(raw[i] >= 0, np.floor(raw[i] + 0.5), -np.floor(-raw[i] + 0.5))
        rows[i, :CODES] = np.clip(r, -100, 100).astype(np.int8)
    return rows, raw


def half_margin(raw):
    """The smallest distance of an unrounded entry from a half-integer."""
    v = raw[~np.isnan(raw)]
    return float(np.abs(v - np.floor(v) - 0.5).min()) if v.size else 1.0


# ---- the loop --------------------------------------------------------------------
def refine_model(po, rows, master, subjects, go, ge, mat, pseudo=10.0):
    """The next table from the current one and the included subjects."""
    aligns = [po.align(rows, s, go, ge) for s in subjects]
    msa = msa_of(len(rows), master, subjects, aligns)
    cnt, weight, wsum = tables(msa)
    new, raw = pssm_from_counts(cnt, wsum, rows, mat, pseudo)
    return new, raw, msa


def select_model(capi, cal, scores, lengths, k, max_evalue, ids=None):
    """(result ids in key order, n_pass) of one key pass and selection: the
    rank table and the cutoff are the library's host-only functions of a
    Calib.  scores and lengths are per SUBJECT; ids (default 0..n-1) are the
    subjects' result ids, which the keys' tie order follows."""
    n = len(scores)
    if n == 0:
        return np.zeros(0, dtype=np.int64), 0
    max_len = int(np.max(lengths))
    adj = capi.sig_rank_table(cal, max_len)
    r_min = capi.sig_rank_min(cal, max_evalue)
    sel, count = rs.ranked(scores, lengths, np.arange(n) if ids is None else np.asarray(ids, dtype=np.int64), adj, r_min, k)
    return rs.key_ids(sel), count


def search_iter_model(capi, po, q, mat, go, ge, res, offs, rounds, inclusion_evalue=1e-3, include_max=4096,
                      pseudo=10.0, k=500, max_evalue=None, ids=None):
    """The loop of sw_search_iter over a database whose subjects have the
    result ids `ids` (default 0..n-1): a dict of rounds (each: the included
    result ids as a sorted list and in key order, the number that passed the
    inclusion bound), converged, rounds_run, report ids / scores / n_pass, the
    last table; lengths per subject and index_of (result id -> subject)."""
    m = np.asarray(mat, dtype=np.int8).reshape(25, 25)
    q = np.asarray(q, dtype=np.uint8)
    offs = np.asarray(offs, dtype=np.int64)
    lengths = np.diff(offs)
    subj = [res[offs[i]:offs[i + 1]] for i in range(len(lengths))]
    ids = np.arange(len(lengths), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    index_of = {int(r): i for i, r in enumerate(ids)}
    assert len(index_of) == len(lengths)
    rows = np.ascontiguousarray(m[q.astype(np.int64)], dtype=np.int8).reshape(-1, 25)
    out = {"rounds": [], "converged": False, "margin": 1.0}
    prev = None
    for t in range(1, rounds + 1):
        scores = po.scan(rows, res, offs, go, ge)
        cal = capi.calib_fit(cs.table(scores, lengths), len(q))
        inc, passed = select_model(capi, cal, scores, lengths, include_max, inclusion_evalue, ids)
        cur = sorted(int(i) for i in inc)
        out["rounds"].append({"ids": cur, "order": [int(i) for i in inc], "n_pass": passed, "calib": cal, "table": rows})
        out["rounds_run"] = t
        same = prev is not None and cur == prev
        prev = cur
        if same:
            out["converged"] = True
        if same or t == rounds:
            break
        rows, raw, _ = refine_model(po, rows, q, [subj[index_of[int(i)]] for i in inc], go, ge, m, pseudo)
        out["margin"] = min(out["margin"], half_margin(raw))
    rep, n_pass = select_model(capi, cal, scores, lengths, k, float("inf") if max_evalue is None else max_evalue, ids)
    out.update(ids=[int(i) for i in rep], scores=[int(scores[index_of[int(i)]]) for i in rep], n_pass=n_pass, rows=rows,
               calib=cal, lengths=lengths, index_of=index_of)
    return out


def family_database(seed=7, n_family=60, n_random=3000):
    """The family hidden among random subjects (the issue's generator): (query,
    residues, offsets); subjects 0 .. n_family - 1 are the members."""
    p = background()
    rng = np.random.default_rng(seed)
    draw = lambda n: rng.choice(20, size=n, p=p).astype(np.uint8)  # noqa: E731
    anc = draw(150)

    def member():
        s = anc.copy()
        m = rng.random(150) < 0.6
        s[m] = draw(m.sum())
        d = rng.integers(10, 130)
        s = np.delete(s, slice(d, d + 3))
        i = rng.integers(10, 130)
        s = np.insert(s, i, draw(2))
        return np.concatenate([draw(rng.integers(0, 40)), s, draw(rng.integers(0, 40))])

    fam = [member() for _ in range(n_family + 1)]
    rand = [draw(int(np.clip(np.rint(np.exp(rng.normal(np.log(200), 0.5))), 30, 900))) for _ in range(n_random)]
    subj = fam[1:] + rand
    offs = np.zeros(len(subj) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subj])
    return fam[0], np.concatenate(subj).astype(np.uint8), offs


# ---- inputs of the limits modules (tests/test_profile_limits_inputs.py, tests/test_gpu_profile_limits.py) ------
def pack(subjects):
    offs = np.zeros(len(subjects) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in subjects])
    res = np.concatenate(subjects).astype(np.uint8) if len(subjects) else np.zeros(0, dtype=np.uint8)
    return res, offs


def align_group_ends(qlen, slens, budget=1 << 30):
    """swplan::align_groups restated: hits are taken in order, and a group
    closes before the hit whose (qlen + slen + 1) * (qlen + 1) direction bytes
    would take it past the budget (a group holds at least one hit)."""
    ends, used, k0 = [], 0, 0
    for k, L in enumerate(slens):
        b = (qlen + int(L) + 1) * (qlen + 1)
        if k > k0 and used + b > budget:
            ends.append(k)
            k0, used = k, 0
        used += b
    if len(slens):
        ends.append(len(slens))
    return ends


def planted(rng, src, sub_rate, codes, flank):
    """src with substitutions over `codes` codes, one deletion and one insertion
    of 1..3 residues in its middle third / last third, and random flanks of
    flank[0] .. flank[1] - 1 residues."""
    s = src.copy()
    m = rng.random(len(s)) < sub_rate
    s[m] = rng.integers(0, codes, size=int(m.sum()))
    n = len(s)
    d = int(rng.integers(n // 3, n // 2))
    i = int(rng.integers(n // 2 + 10, 2 * n // 3 + 10))
    s = np.insert(s, i, rng.integers(0, 20, size=int(rng.integers(1, 4))))
    s = np.delete(s, slice(d, d + int(rng.integers(1, 4))))
    return np.concatenate([rng.integers(0, codes, size=int(rng.integers(*flank))), s,
                           rng.integers(0, codes, size=int(rng.integers(*flank)))]).astype(np.uint8)


def many_hits_input(seed=5):
    """The many-hits input: (query of 600 residues, 30 positions of them in the
    codes 20..24 (the two ends hold X, which no piece covers), 47 distinct
    subjects of 380..550 residues, 4,096 ids: 88 random permutations of the 47,
    cut)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 20, size=600).astype(np.uint8)
    amb = rng.choice(np.arange(1, 599), size=28, replace=False)
    q[amb] = rng.integers(20, 25, size=28)
    q[0] = q[599] = 23
    subjects = []
    for _ in range(47):
        n = int(rng.integers(365, 470))
        a = int(rng.integers(1, 599 - n))
        subjects.append(planted(rng, q[a:a + n], 0.30, 25, (10, 36)))
    ids = np.concatenate([rng.permutation(47) for _ in range(88)])[:4096].astype(np.int32)
    return q, subjects, ids


def custom_ids(n, seed=3):
    """Result ids 7 + 3 p(i), p a random injection into 0 .. 4 n - 1 that takes
    the value 4 n - 1: shuffled, with gaps, the largest above 10 n."""
    p = np.random.default_rng(seed).permutation(4 * n)[:n]
    p[np.argmax(p)] = 4 * n - 1
    return (7 + 3 * p).astype(np.int32)


FAMILY_LONG_THRESHOLD = 190  # family members (147..229 residues) fall on both sides


def envelope_input(seed=17):
    """The envelope input: (consensus of 375 codes over all 25, the
    position-specific table (entries -8..12, the consensus entry 13..15),
    150 subjects over 25 codes, ids).  Subjects 0..39 are planted: the
    consensus itself, then copies with 3 to 12 % substitutions, one deletion and
    one insertion of 1..3 each and flanks; the others are random, 30..400
    residues.  ids: the planted ones, ten random ones, and two repeats."""
    rng = np.random.default_rng(seed)
    q0 = rng.integers(0, 25, size=375).astype(np.uint8)
    t = rng.integers(-8, 13, size=(375, 25))
    t[np.arange(375), q0] = rng.integers(13, 16, size=375)
    subjects = [q0.copy()]
    for k in range(39):
        subjects.append(planted(rng, q0, 0.03 + 0.09 * k / 38, 25, (0, 30)))
    subjects += [rng.integers(0, 25, size=int(n)).astype(np.uint8) for n in rng.integers(30, 401, size=110)]
    order = rng.permutation(150)
    subjects = [subjects[k] for k in order]
    where = np.argsort(order)  # where[k]: the index of what was subject k
    ids = np.concatenate([where[:40], where[40:50], where[[0, 7]]]).astype(np.int32)
    return q0, np.ascontiguousarray(t, dtype=np.int8), subjects, ids


def scaled_table(t):
    """A table's entries stretched to -100 .. 100: the positive ones by 100 / 13
    (13 and above: 100), the negative ones by 100 / 8."""
    t = np.asarray(t, dtype=np.int64)
    return np.where(t > 0, np.minimum(t * 100 // 13, 100), -((-t) * 100 // 8)).astype(np.int8)


def matrix_100():
    """100 on the diagonal, -100 elsewhere."""
    m = np.full((25, 25), -100, dtype=np.int8)
    np.fill_diagonal(m, 100)
    return m


def envelope_scorings(q0, table, blosum62):
    """name -> (rows, gap_open, gap_extend, the refine's matrix)."""
    m100 = matrix_100()
    return {"specific-1-4": (table, 1, 4, blosum62), "specific-1000-1000": (table, 1000, 1000, blosum62),
            "scaled-28-28": (scaled_table(table), 28, 28, blosum62), "scaled-40-3": (scaled_table(table), 40, 3, blosum62),
            "m100-11-1": (np.ascontiguousarray(m100[q0.astype(np.int64)]), 11, 1, m100)}


def envelope_master(name, q0):
    """The master of an envelope refine: the consensus; under the 100 / -100
    matrix every ninth position holds another residue, so that those columns
    count two codes (a mismatch never lies on a path there, a gap pair is
    cheaper) and the unrounded entries leave the clamp's range."""
    if name != "m100-11-1":
        return q0
    m = q0.copy()
    m[::9] = (q0[::9] + 1) % 20
    return m


def clamp_rows(seed=1):
    """40 rows x 30 columns as a family's alignment makes them (row 0 the
    master); column 4 holds one W (code 17, the rarest) in row 0 and an A
    everywhere else."""
    rng = np.random.default_rng(seed)
    master = rng.integers(0, 20, size=30).astype(np.uint8)
    msa = np.tile(master, (40, 1))
    sub = rng.random((40, 30)) < 0.25
    sub[0] = False
    msa[sub] = rng.integers(0, 25, size=int(sub.sum()))
    msa[rng.random((40, 30)) < 0.05] = GAP
    msa[0] = master
    for r in range(1, 40):
        a, b = sorted(int(x) for x in rng.integers(0, 31, size=2))
        msa[r, :min(a, 3)] = NONE
        msa[r, max(b, 27):] = NONE
    msa[:, 4] = 0
    msa[0, 4] = 17
    return msa.astype(np.uint8)
