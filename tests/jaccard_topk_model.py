"""A numpy restatement of K25's decision (csrc/jaccard_topk.hip: launches A, A' and B), shared by
tests/test_jaccard_topk_host.py (which checks it against the canonical float32 words) and the GPU tests (which derive
from it the queries the device must leave unresolved).  The rows, the pack, the sides, the word-to-quotient map and
the canonical words are tests/test_jaccard_filter_host.py's (K24); here are only the three steps K25 adds.  Not a test
module: nothing in it is collected."""
import numpy as np

import test_jaccard_filter_host as K24

U = K24.U
NQ, NG = K24.NA, K24.NB
AB = ((-1.0, 0.0), (1.0, 0.0), (-0.5, 0.25))
K_SAMPLE = ((1, 128), (10, 128), (64, 128), (10, 520), (64, 520))
F32_MIN_NORMAL = float(np.float32(1.17549435e-38))


def rows(d, dts, nonneg):
    """The adversarial 300 x 520 rows of K24's host test, as float64 values of the given storage dtypes."""
    a, b, _, _ = K24._adversarial(d, dts[0], dts[1], nonneg)
    return a, b


def sample_of(n_g, k, sample_rows):
    """l2t_sample: the caller's sample (0 / None: the default), at least k, a multiple of 128, at most the gallery."""
    s = sample_rows if sample_rows else min(65536, max(1024, max(k, 8) * (n_g // 128)))
    s = (max(s, k) + 127) // 128 * 128
    return min(s, max(n_g, 1))


def intervals(a, b):
    """jacf_interval of every pair on the grid of both sets: (ilo, ihi, ulo, uhi), ilo / ihi NaN without one."""
    d = a.shape[1]
    lo, s = K24._grid(a, b)
    qa, ea, Qa, Sa = K24._pack(a, lo, s)
    qb, eb, Qb, Sb = K24._pack(b, lo, s)
    sad = np.zeros((a.shape[0], b.shape[0]), np.int64)
    for k0 in range(0, d, 64):
        sad += np.abs(qa[:, None, k0:k0 + 64] - qb[None, :, k0:k0 + 64]).sum(axis=2)
    pa, wa = K24._side(ea, Sa, Qa, float(d), lo, s)
    pb, wb = K24._side(eb, Sb, Qb, float(d), lo, s)
    with np.errstate(invalid="ignore", over="ignore"):
        m = s * sad.astype(np.float64)
        P = pa[:, None] + pb[None, :]
        W = ((wa[:, None] + wb[None, :]) + 16.0 * U * m) * (1.0 + 1e-9) + 1e-280
        ih, uh = 0.5 * (P - m), 0.5 * (P + m)
        ulo, uhi = uh - W, uh + W
        ok = (W < 1e300) & (ulo > 0.0) & (uhi < 1e300)
        return np.where(ok, ih - W, np.nan), np.where(ok, ih + W, np.nan), ulo, uhi


def f32_up(x):
    """l2t_f32_up: the least float32 at or above x, or one close to it (never below); NaN -> +inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = x.astype(np.float32)
        low = f.astype(np.float64) < x
        up = np.where(f == 0, np.float32(F32_MIN_NORMAL), np.nextafter(f, np.float32(np.inf)))
        return np.where(np.isnan(x), np.float32(np.inf), np.where(low, up, f))


def bounds(ilo, ihi, ulo, uhi, pos):
    """Launch A: every pair's upper bound on the key s q as the float32 it is stored as."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        num = ihi if pos else ilo
        den = np.where((num >= 0.0) == pos, ulo, uhi)
        e = num / den
        w = 8.0 * U * np.abs(e) + 1e-300
        return f32_up(e + w if pos else -(e - w))


def next32(t):
    """jact_next32: the float32 after t (FLT_MAX steps to +inf)."""
    with np.errstate(over="ignore"):
        return np.float32(1e-45) if t == 0 else np.nextafter(np.float32(t), np.float32(np.inf))


def widen(tau, alpha, beta):
    """jact_widen: (the quotient-space threshold or NaN, the number of the accepted guess -- 1 is the first -- or 0)."""
    pos = alpha > 0.0
    if not np.isfinite(tau):
        return np.nan, 0
    q_tau = float(tau) if pos else -float(tau)
    with np.errstate(over="ignore"):
        t = np.float32(alpha * q_tau + beta)
    for it in range(12):
        if not np.isfinite(t):
            return np.nan, 0
        tn = next32(t)
        if not np.isfinite(tn):
            return np.nan, 0
        tl, tu = K24._thresholds(tn, alpha, beta)
        if np.isnan(tl):
            return np.nan, 0
        if (q_tau < tl) if pos else (q_tau > tu):
            return (tu if pos else tl), it + 1
        t = tn
    return np.nan, 0


def decide(a, b, alpha, beta, k, sample_rows, iv=None):
    """Launches A, A' and B: (thr [n_q] -- NaN: no threshold --, guess [n_q], cand [n_q, n_g] bool: the columns launch
    B appends for a query that has a threshold)."""
    ilo, ihi, ulo, uhi = intervals(a, b) if iv is None else iv
    pos = alpha > 0.0
    ns = sample_of(b.shape[0], k, sample_rows)
    ub = bounds(ilo[:, :ns], ihi[:, :ns], ulo[:, :ns], uhi[:, :ns], pos)
    tau = np.sort(ub, axis=1)[:, k - 1]
    thr = np.empty(a.shape[0])
    guess = np.zeros(a.shape[0], np.int64)
    for i in range(a.shape[0]):
        thr[i], guess[i] = widen(tau[i], alpha, beta)
    with np.errstate(invalid="ignore", over="ignore"):
        T = thr[:, None]
        if pos:
            out = ilo > T * np.where(T >= 0.0, uhi, ulo)   # jacf_gt
        else:
            out = ihi < T * np.where(T >= 0.0, ulo, uhi)   # jacf_lt
    return thr, guess, ~out


def unresolved(thr, cand, k, cand_cap):
    """The queries launch C marks -2: no threshold, a list above cand_cap, or fewer than k candidates."""
    n = cand.sum(axis=1)
    return np.isnan(thr) | (n > cand_cap) | (n < k)


def order(words):
    """The top-k order of one query's canonical float32 words: (word asc, index asc), -0 == +0, NaN last in index
    order -- a stable argsort."""
    w = np.where(words == 0, np.float32(0), words)
    return np.argsort(w, kind="stable")
