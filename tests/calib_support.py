"""The calibration's definitions (include/sw_amd.h, "E-values and bit scores")
restated in numpy: the length bin, the count table, the trimmed regression,
the status bits and the significance of a hit.  tests/test_calib_cpu.py and
tests/test_gpu_calib.py compare the library against these."""
import numpy as np

LBINS, SBINS = 128, 512
CLIPPED, FEW, DEGENERATE = 1, 2, 4
PI_SQRT6 = np.pi / np.sqrt(6.0)
GAMMA = 0.57721566490153286061


def length_bin(L):
    """b = 4 e + f for lengths L >= 1 (array): e = floor(log2 L) from the bit
    length, f = the two bits below the leading bit."""
    L = np.asarray(L, dtype=np.int64)
    e = np.array([int(v).bit_length() - 1 for v in L.ravel()], dtype=np.int64).reshape(L.shape)
    f = np.where(e >= 2, (L >> np.maximum(e - 2, 0)) & 3, (L << np.maximum(2 - e, 0)) & 3)
    return 4 * e + f


def length_bin_fast(L):
    """length_bin for long arrays (L < 2^52: frexp is exact there)."""
    L = np.asarray(L, dtype=np.int64)
    e = np.frexp(L.astype(np.float64))[1].astype(np.int64) - 1
    f = np.where(e >= 2, (L >> np.maximum(e - 2, 0)) & 3, (L << np.maximum(2 - e, 0)) & 3)
    return 4 * e + f


def abscissa():
    b = np.arange(LBINS)
    e, f = b >> 2, b & 3
    return np.log(np.ldexp(1.0 + (f + 0.5) / 4.0, e))


def table(scores, lengths):
    """uint32 [128, 512]: one count per subject of length >= 1 at
    [bin, clamp(score, 0, 511)] (scores and lengths per SUBJECT)."""
    scores = np.asarray(scores, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    ok = lengths > 0
    H = np.zeros((LBINS, SBINS), dtype=np.uint32)
    np.add.at(H, (length_bin_fast(lengths[ok]), np.clip(scores[ok], 0, SBINS - 1)), 1)
    return H


def fit(H, qlen):
    """The trimmed weighted regression of score on x_b: a dict with sw_calib's
    fields but size and n_skipped."""
    H = np.asarray(H, dtype=np.int64).reshape(LBINS, SBINS)
    out = {"qlen": int(qlen), "n_db": int(H.sum()), "n_clipped": int(H[:, SBINS - 1].sum()), "status": 0, "fits": 0}
    if out["n_clipped"] * 100 > out["n_db"]:
        out["status"] |= CLIPPED
    b, s = np.nonzero(H[:, :SBINS - 1])
    w = H[b, s].astype(np.float64)
    x = abscissa()[b]
    s = s.astype(np.float64)
    keep = np.ones(len(w), dtype=bool)
    degenerate, bins_kept = True, 0
    for rnd in range(1, 9):
        wk, xk, sk = w[keep], x[keep], s[keep]
        W = wk.sum()
        bins_kept = len(np.unique(b[keep]))
        out["n_fit"] = int(W)
        ms = (wk * sk).sum() / W if W > 0 else 0.0
        degenerate = True
        out.update(a=ms, c=0.0, sigma=0.0)
        if W < 3 or bins_kept < 2:
            break
        mx = (wk * xk).sum() / W
        Sxx = (wk * (xk - mx) * (xk - mx)).sum()
        Sxy = (wk * (xk - mx) * (sk - ms)).sum()
        if not Sxx > 0:
            break
        c = Sxy / Sxx
        a = ms - c * mx
        r = sk - a - c * xk
        sigma = np.sqrt((wk * r * r).sum() / (W - 2))
        if not sigma > 0:
            break
        degenerate = False
        out.update(a=a, c=c, sigma=sigma, fits=rnd)
        if rnd == 8:
            break
        t = (s - a - c * x) / sigma
        nxt = ~((t > 5) | (t < -5))
        if np.array_equal(nxt, keep):
            break
        keep = nxt
    if degenerate:
        out["status"] |= DEGENERATE
    if bins_kept < 3 or out["n_fit"] < 500:
        out["status"] |= FEW
    return out


def sig(cal, score, slen):
    """(evalue, bits, z) of a hit under fit()'s dict."""
    n_db = float(cal["n_db"])
    if cal["status"] & DEGENERATE or not cal["sigma"] > 0 or slen <= 0 or score <= 0 or cal["qlen"] <= 0:
        return n_db, 0.0, 0.0
    z = (score - cal["a"] - cal["c"] * np.log(float(slen))) / cal["sigma"]
    t = PI_SQRT6 * z + GAMMA
    with np.errstate(over="ignore"):
        e = n_db * -np.expm1(-np.exp(-t))
    return float(e), float((t + np.log(float(cal["qlen"]) * float(slen))) / np.log(2.0)), float(z)


def evalues(cal, scores, lengths):
    """sig()'s E-values for arrays (degenerate calibrations aside)."""
    scores = np.asarray(scores, dtype=np.float64)
    lengths = np.asarray(lengths, dtype=np.float64)
    ok = (lengths > 0) & (scores > 0)
    z = (scores - cal["a"] - cal["c"] * np.log(np.where(ok, lengths, 1.0))) / cal["sigma"]
    with np.errstate(over="ignore"):
        e = cal["n_db"] * -np.expm1(-np.exp(-(PI_SQRT6 * z + GAMMA)))
    return np.where(ok, e, float(cal["n_db"]))
