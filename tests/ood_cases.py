"""Numpy restatement of out-of-distribution detection (protoasnet_amd/ood.py, csrc/ood.hip, include/protoasnet_amd.h) and the seeded
case generators of its tests.  The reference has no code for any of this: the restatement IS the specification the kernels are held to
-- kNN distances, indices, moments, maxsim and normalised rows bitwise, flags and tallies as integers, energy and Mahalanobis to a
derived bound.  A HIGHER score means MORE out-of-distribution."""
import math

import numpy as np

TALLY_NAMES = ("id_rows", "id_flagged", "ood_rows", "ood_flagged", "nan_rows", "id_correct_kept", "id_kept", "id_correct_flagged")
DEFAULT_CHUNK = 256  # pasn_ood_moment_chunk(); the CPU tests check that the library says the same


# ---- scores that need no fit -------------------------------------------------------------------------------------------------------------
def maxsim_ref(sim) -> np.ndarray:
    s = np.asarray(sim, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        out = (np.float32(1.0) - s.max(axis=1)).astype(np.float32)  # (numpy's max propagates a NaN)
    out[np.isnan(s).any(1)] = np.nan
    return out


def energy_ref(logits, K_real: int, rounded: bool = True) -> np.ndarray:
    """-(m + log(sum_k exp(l_k - m))) in float64 over the first K_real logits, the sum in class order; one rounding to float32."""
    l = np.asarray(logits, dtype=np.float32)[:, :K_real].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = l.max(axis=1)
        s = np.zeros(len(l))
        for k in range(K_real):
            s = s + np.exp(l[:, k] - m)
        e = -(m + np.log(s))
        e[np.isnan(l).any(1)] = np.nan
        return e.astype(np.float32) if rounded else e


def normalize_ref(x) -> np.ndarray:
    """n2 = the float32 sum of squares in column order, each operation rounded on its own; y = x / sqrt(n2); a zero row is copied."""
    x = np.asarray(x, dtype=np.float32)
    n2 = np.zeros(len(x), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(x.shape[1]):
            n2 = n2 + x[:, j] * x[:, j]
        y = x / np.sqrt(n2)[:, None]
    y[n2 == 0] = x[n2 == 0]
    return y.astype(np.float32)


# ---- k nearest bank rows -----------------------------------------------------------------------------------------------------------------
def dist_ref(q, bank, fma: bool = False) -> np.ndarray:
    """d (Mq, Mb) float32: acc = acc + t * t, t = q[i][j] - bank[m][j], from 0 for j ascending; numpy rounds every float32 operation on
    its own.  ``fma=True`` is NOT the definition: the product kept exact (float64 holds it) and added with one rounding, as a fused
    multiply-add would -- what the device code must not do."""
    q, bank = np.asarray(q, dtype=np.float32), np.asarray(bank, dtype=np.float32)
    acc = np.zeros((len(q), len(bank)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(q.shape[1]):
            t = q[:, None, j] - bank[None, :, j]
            if fma:
                t64 = t.astype(np.float64)
                acc = (t64 * t64 + acc.astype(np.float64)).astype(np.float32)
            else:
                acc = acc + t * t
    return acc


def knn_ref(q, bank, k: int, self_base: int = -1, fma: bool = False):
    """(dist (Mq, k) float32, index (Mq, k) int32, status (2,) int64): the k eligible rows of smallest d in ascending d, the lower bank
    index first on ties; fill +inf / -1; a query holding a NaN gets NaN / -1.  Not eligible: a bank row holding a NaN, the row
    self_base + i (self_base >= 0), a pair whose d is NaN."""
    q, bank = np.asarray(q, dtype=np.float32), np.asarray(bank, dtype=np.float32)
    Mq, Mb = len(q), len(bank)
    d = dist_ref(q, bank, fma)
    bnan, qnan = np.isnan(bank).any(1), np.isnan(q).any(1)
    d[:, bnan] = np.nan
    if self_base >= 0:
        i = np.arange(Mq)
        ok = self_base + i < Mb
        d[i[ok], self_base + i[ok]] = np.nan
    order = np.argsort(d, axis=1, kind="stable")[:, :k]  # NaN sorts last; stable: the lower index first on ties
    dist = np.full((Mq, k), np.inf, dtype=np.float32)
    index = np.full((Mq, k), -1, dtype=np.int32)
    got = np.take_along_axis(d, order, 1)
    live = ~np.isnan(got)
    kk = order.shape[1]
    dist[:, :kk][live] = got[live]
    index[:, :kk][live] = order[live]
    dist[qnan], index[qnan] = np.nan, -1
    return dist, index, np.array([bnan.sum(), qnan.sum()], dtype=np.int64)


# ---- class-conditional Gaussians -----------------------------------------------------------------------------------------------------------
def moments_ref(x, labels, K: int, chunk: int = DEFAULT_CHUNK, prev=None):
    """{n (K,) int64, sum (K, E), scatter (E, E) float64, skipped (2,) int64} in the defined order: chunks of `chunk` consecutive rows,
    each summed from 0.0 in row order, the partials added in chunk order from 0.0; `prev`: then added onto an earlier result."""
    x32 = np.asarray(x, dtype=np.float32)
    x, L = x32.astype(np.float64), np.asarray(labels).astype(np.int64)
    M, E = x.shape
    in_range = (L >= 0) & (L < K)
    bad = np.isnan(x32).any(1)
    valid = in_range & ~bad
    n = np.bincount(L[valid], minlength=K).astype(np.int64)
    s, sc = np.zeros((K, E)), np.zeros((E, E))
    for r0 in range(0, M, chunk):
        ps, psc = np.zeros((K, E)), np.zeros((E, E))
        for i in range(r0, min(M, r0 + chunk)):
            if valid[i]:
                ps[L[i]] = ps[L[i]] + x[i]
                psc = psc + np.outer(x[i], x[i])
        s, sc = s + ps, sc + psc
    out = {"n": n, "sum": s, "scatter": sc, "skipped": np.array([(~in_range).sum(), (in_range & bad).sum()], dtype=np.int64)}
    if prev is not None:
        out = {k: prev[k] + out[k] for k in out}
    return out


def gaussian_fit_ref(n, s, scatter, shrink: float = 1e-6):
    """(mu (K, E), W (E, E)): class means (NaN without rows), pooled within-class covariance over N - C, ridge shrink tr / E, W = L^-1."""
    n = np.asarray(n, dtype=np.int64)
    K, E = s.shape
    N, C = int(n.sum()), int((n > 0).sum())
    if N < E + C:
        raise ValueError(f"needs at least {E + C} valid rows, got {N}")
    mu = np.full((K, E), np.nan)
    within = np.array(scatter, dtype=np.float64)
    for c in range(K):
        if n[c] > 0:
            mu[c] = s[c] / float(n[c])
            within = within - float(n[c]) * np.outer(mu[c], mu[c])
    cov = within / float(N - C)
    cov = cov + float(shrink) * (np.trace(cov) / E) * np.eye(E)
    return mu, np.tril(np.linalg.inv(np.linalg.cholesky(cov)))


def mahalanobis_ref(x, mu, W):
    """(m (M, K) float64, bound (M, K), score (M,) float32, argclass (M,) int32); bound = 4 E 2^-52 sum_i (sum_j |W_ij| |x_j - mu_cj|)^2:
    a dot product of E terms summed in any order is within E 2^-53 sum |terms| (to first order) of exact; squaring y_i doubles the
    relative error of each term of the outer sum, whose own summation adds as much again -- 4 E 2^-52 covers both sides (the device's
    and this restatement's)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    M, E = x.shape
    K = len(mu)
    m, bound = np.full((M, K), np.nan), np.full((M, K), np.nan)
    for c in range(K):
        d = x - mu[c][None, :]
        y = d @ W.T
        m[:, c] = (y * y).sum(1)
        bound[:, c] = 4.0 * E * 2.0 ** -52 * ((np.abs(d) @ np.abs(W).T) ** 2).sum(1)
    fitted = np.isfinite(mu[:, 0])
    arg, best = np.full(M, -1, dtype=np.int32), np.zeros(M)
    for c in np.flatnonzero(fitted):  # the first smallest among the classes with a finite mean; a NaN m_c never wins
        with np.errstate(invalid="ignore"):
            take = np.where(arg < 0, ~np.isnan(m[:, c]), m[:, c] < best)
        best, arg = np.where(take, m[:, c], best), np.where(take, c, arg).astype(np.int32)
    with np.errstate(over="ignore"):
        score = np.where(arg >= 0, best, np.nan).astype(np.float32)
    return m, bound, score, arg


# ---- thresholds, flags, tallies ------------------------------------------------------------------------------------------------------------
def threshold_ref(scores, tpr: float):
    """(tau float32, n, r, nan): the r-th smallest non-NaN score, r = ceil((n + 1)(1 - alpha)) with alpha = 1 - tpr formed on the host
    (pasn_conformal_quantiles' arithmetic), +inf when r > n."""
    s = np.asarray(scores, dtype=np.float32)
    v = np.sort(s[~np.isnan(s)])
    n = int(v.size)
    alpha = 1.0 - float(tpr)
    r = int(math.ceil(float(n + 1) * (1.0 - alpha)))
    return (np.float32(np.inf) if r > n else v[r - 1]), n, r, int(np.isnan(s).sum())


def tally_ref(scores, kind, tau, correct=None):
    """(flags (A, M) uint8, tallies (A, 8) int64): flagged iff score > tau or the score is NaN; TALLY_NAMES."""
    s, kind, tau = np.asarray(scores, dtype=np.float32), np.asarray(kind).astype(np.int64), np.asarray(tau, dtype=np.float32)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        flags = ((s[None, :] > tau[:, None]) | nan[None, :]).astype(np.uint8)
    idr, ood = kind == 0, kind == 1
    t = np.zeros((len(tau), 8), dtype=np.int64)
    for a in range(len(tau)):
        f = flags[a].astype(bool)
        t[a, :5] = [idr.sum(), (idr & f).sum(), ood.sum(), (ood & f).sum(), ((idr | ood) & nan).sum()]
        if correct is not None:
            ok = np.asarray(correct) != 0
            t[a, 5:] = [(idr & ~f & ok).sum(), (idr & ~f).sum(), (idr & f & ok).sum()]
    return flags, t


def auroc_ref(scores, kind) -> float:
    """Mann-Whitney with ties counted 1/2, shifted rows (kind 1) positive; rows of another kind or with a NaN score do not enter."""
    s, kind = np.asarray(scores, dtype=np.float32), np.asarray(kind)
    ok = ~np.isnan(s)
    pos, neg = s[ok & (kind == 1)], s[ok & (kind == 0)]
    if not len(pos) or not len(neg):
        return float("nan")
    u2 = int((2 * (neg[None, :] < pos[:, None]).astype(np.int64) + (neg[None, :] == pos[:, None])).sum())
    return u2 / (2.0 * len(pos) * len(neg))


def cine_mean_ref(scores, offsets, rows) -> np.ndarray:
    """A cine's score: the float64 mean of its clips' float32 scores, added in the listed order; one cast to float32."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    out = np.empty(len(offsets) - 1, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(out)):
            acc = 0.0
            for i in rows[offsets[g]: offsets[g + 1]]:
                acc = acc + s[i]
            out[g] = np.float32(acc / float(offsets[g + 1] - offsets[g])) if offsets[g + 1] > offsets[g] else np.nan
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def emb_case(M: int, E: int, seed: int, levels: int = 0) -> np.ndarray:
    """(M, E) float32 rows in [-1, 1); ``levels`` > 0 quantises every coordinate to that many values, so exact ties are the rule."""
    rng = np.random.default_rng(seed)
    if levels:
        return (rng.integers(0, levels, (M, E)).astype(np.float32) / np.float32(levels) - np.float32(0.5)).astype(np.float32)
    return (rng.random((M, E), dtype=np.float32) * 2 - 1).astype(np.float32)


def mixture_case(M: int, E: int, K: int, seed: int, shift: float = 0.0, spread: float = 3.0):
    """(x (M, E) float32, labels (M,) int32): K Gaussian blobs with fixed centres (the centres depend on (E, K) only, not on the seed),
    unit variance, plus ``shift`` on every coordinate."""
    centres = np.random.default_rng(1000 * E + K).normal(0.0, spread, (K, E))
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, K, M).astype(np.int32)
    x = centres[labels] + rng.normal(0.0, 1.0, (M, E)) + shift
    return x.astype(np.float32), labels
