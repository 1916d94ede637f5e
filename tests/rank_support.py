"""numpy restatement of the ranking by E-value (include/sw_amd.h "ranking by
E-value"): the rank value r, its key, the selection of the k best keys and
the count of subjects that pass a cutoff, given an adjustment table adj.
Integers only (Python ints / int64): no tolerance anywhere."""
import numpy as np

SCALE = 4096
R_FLOOR = -2 ** 32 + 1
R_CEIL = 2 ** 32 - 1
R_NONE = 2 ** 32
MAX_SCORE = 2 ** 20 - 1
PAD = np.iinfo(np.int64).min


def rank_values(scores, lengths, adj):
    """r(s, L) of every subject: int64 array."""
    s = np.asarray(scores, dtype=np.int64)
    L = np.asarray(lengths, dtype=np.int64)
    a = np.asarray(adj, dtype=np.int64)[np.clip(L, 0, len(adj) - 1)]
    r = np.clip(np.clip(s, 0, MAX_SCORE) * SCALE - a, R_FLOOR, R_CEIL)
    return np.where((s <= 0) | (L <= 0), R_FLOOR, r)


def keys(r, ids, r_min=R_FLOOR):
    """Every subject's key (PAD below r_min), in the subjects' order."""
    r = np.asarray(r, dtype=np.int64)
    k = r * 2 ** 31 + (2 ** 31 - 1 - np.asarray(ids, dtype=np.int64))
    return np.where(r >= r_min, k, PAD)


def select(all_keys, k):
    """The k best keys, best first, padded with PAD."""
    srt = np.sort(np.asarray(all_keys, dtype=np.int64))[::-1][:k]
    return np.concatenate([srt, np.full(k - len(srt), PAD, dtype=np.int64)])


def count(r, r_min):
    return int((np.asarray(r, dtype=np.int64) >= r_min).sum())


def key_ids(sel):
    """The result ids of selected keys (PAD entries dropped)."""
    sel = np.asarray(sel, dtype=np.int64)
    sel = sel[sel != PAD]
    return (2 ** 31 - 1 - (sel & (2 ** 31 - 1))).astype(np.int64)


def ranked(scores, lengths, ids, adj, r_min, k):
    """(selected keys [k], count) of a score vector indexed by SUBJECT."""
    r = rank_values(scores, lengths, adj)
    return select(keys(r, ids, r_min), k), count(r, r_min)


def ranked_groups(nq, slots, score_bytes):
    budget = score_bytes if score_bytes else 256 << 20
    rows = budget // (4 * slots) if slots > 0 else nq
    return max(1, min(nq, rows))
