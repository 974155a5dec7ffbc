"""Float64 / int64 numpy restatement of split conformal prediction (protoasnet_amd/conformal.py, csrc/conformal.hip,
include/protoasnet_amd.h) and the seeded case generators of its tests.  The reference has no code for any of this: the restatement IS
the specification the kernels are held to -- scores and thresholds bitwise, masks and tallies as integers."""
import math
from fractions import Fraction

import numpy as np

import bootstrap_cases as bc
import calibration_cases as cc

KINDS = ("lac", "aps", "raps")
PAD, NAN = -1, -2  # `stratum` of a row that is not valid


def tally_words(K: int) -> int:
    return 3 + 4 * (K + 1) + 2 * K


# ---- scores ------------------------------------------------------------------------------------------------------------------------------
def uniforms(M: int, seed: int, salt: int) -> np.ndarray:
    """U_i = word 0 of philox4x32_10(counter (i lo, i hi, salt, 0), key (seed lo, seed hi)) * 2^-32, float64."""
    i = np.arange(M, dtype=np.uint64)
    ctr = np.stack([i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full_like(i, salt), np.zeros_like(i)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return bc.philox4x32_10(ctr, key)[:, 0].astype(np.float64) * 2.0 ** -32


def ranking(probs) -> np.ndarray:
    """order[i][r] = the class of rank r + 1: descending probability, the lower class first on ties."""
    return np.argsort(-np.asarray(probs, dtype=np.float32), axis=1, kind="stable")


def nan_rows(probs) -> np.ndarray:
    return np.isnan(np.asarray(probs, dtype=np.float32)).any(1)


def scores_ref(probs, kind="aps", randomized=True, seed=0, lam=0.0, k_reg=1, salt=0, fused=False, rounded=True) -> np.ndarray:
    """The (M, K) float32 score table.  Every step is one float64 operation (numpy never contracts), then one rounding to float32; every
    score of a row that holds a NaN is NaN.  ``fused=True`` is NOT the definition: ``acc + U p`` with ONE rounding, as a fused
    multiply-add would compute it (exact rational arithmetic, rounded to float64 once) -- what the device code must not do.
    ``rounded=False`` returns the float64 values before the one rounding."""
    p32 = np.asarray(probs, dtype=np.float32)
    p = p32.astype(np.float64)
    M, K = p.shape
    bad = nan_rows(p32)
    if kind == "lac":
        s = 1.0 - p
    else:
        order = ranking(np.where(bad[:, None], 0, p32))
        ps = np.take_along_axis(p, order, 1)
        acc = np.concatenate([np.zeros((M, 1)), np.cumsum(ps, axis=1)[:, :-1]], 1)  # cumsum adds in order: the running sum
        U = uniforms(M, seed, salt) if randomized else np.ones(M)
        if fused:
            ss = np.array([[float(Fraction(a) + Fraction(u) * Fraction(x)) if np.isfinite(a + x) else a + u * x for a, x in zip(ra, rp)]
                           for ra, rp, u in zip(acc.tolist(), ps.tolist(), U.tolist())]).reshape(M, K)
        else:
            ss = acc + U[:, None] * ps
        if kind == "raps":
            ss = ss + lam * np.maximum(0, np.arange(1, K + 1) - k_reg).astype(np.float64)[None, :]
        elif kind != "aps":
            raise ValueError(kind)
        s = np.empty((M, K))
        np.put_along_axis(s, order, ss, 1)
    if rounded:
        with np.errstate(over="ignore", invalid="ignore"):
            s = s.astype(np.float32)
    s[bad] = np.nan
    return s


def strata_ref(probs, labels):
    """stratum_i: the label of a valid row, PAD for a padding row, NAN for a row that holds a NaN."""
    labels = np.asarray(labels).astype(np.int64)
    K = np.asarray(probs).shape[1]
    bad = nan_rows(probs)
    return np.where(bad, NAN, np.where((labels >= 0) & (labels < K), labels, PAD)).astype(np.int32)


def own_ref(table, stratum) -> np.ndarray:
    own = np.full(len(stratum), np.nan, dtype=np.float32)
    ok = stratum >= 0
    own[ok] = table[np.flatnonzero(ok), stratum[ok]]
    return own


# ---- thresholds --------------------------------------------------------------------------------------------------------------------------
def quantile_ref(values, alpha: float):
    """(q, n, r): r = ceil((n + 1)(1 - alpha)) in float64, q the r-th smallest as float32, +inf when r > n."""
    v = np.sort(np.asarray(values, dtype=np.float32))
    n = int(v.size)
    r = int(math.ceil(float(n + 1) * (1.0 - float(alpha))))
    return (np.float32(np.inf) if r > n else v[r - 1]), n, r


def calibrate_ref(probs, labels, alphas, kind="aps", randomized=True, seed=0, lam=0.0, k_reg=1):
    """{qhat (1 + K, A) float32, n (1 + K,) int64, r (1 + K, A) int64}; the uniforms of calibration carry salt 0."""
    K = np.asarray(probs).shape[1]
    table = scores_ref(probs, kind, randomized, seed, lam, k_reg, salt=0)
    st = strata_ref(probs, labels)
    own = own_ref(table, st)
    qhat = np.empty((K + 1, len(alphas)), dtype=np.float32)
    n, r = np.empty(K + 1, dtype=np.int64), np.empty((K + 1, len(alphas)), dtype=np.int64)
    for s in range(K + 1):
        rows = own[st >= 0] if s == 0 else own[st == s - 1]
        for a, alpha in enumerate(alphas):
            qhat[s, a], n[s], r[s, a] = quantile_ref(rows, alpha)
    return {"qhat": qhat, "n": n, "r": r}


# ---- sets and tallies --------------------------------------------------------------------------------------------------------------------
def sets_ref(table, qhat, labels=None, u=None, mondrian=False):
    """(masks (A, M) uint16, tallies (A, T) int64) from a float32 score table and float32 thresholds (1 + K, A)."""
    table, qhat = np.asarray(table, dtype=np.float32), np.asarray(qhat, dtype=np.float32)
    M, K = table.shape
    A = qhat.shape[1]
    bad = np.isnan(table).any(1)
    if labels is None:
        labelled, L = np.zeros(M, bool), np.zeros(M, np.int64)
        enters = ~bad
    else:
        L = np.asarray(labels).astype(np.int64)
        labelled = (L >= 0) & (L < K)
        enters = labelled & ~bad
        L = np.where(labelled, L, 0)
    masks = np.zeros((A, M), dtype=np.uint16)
    tallies = np.zeros((A, tally_words(K)), dtype=np.int64)
    if u is not None:
        u32 = np.asarray(u, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            has_u = (u32 >= 0) & (u32 <= 1)
        uq = (np.where(has_u, u32, 0).astype(np.float64) * 4294967296.0).astype(np.uint64)
    o_size, o_cov, o_u, o_un, o_cn = 3, 3 + (K + 1), 3 + 2 * (K + 1), 3 + 3 * (K + 1), 3 + 4 * (K + 1)
    for a in range(A):
        thr = qhat[1:, a][None, :] if mondrian else qhat[0, a]
        with np.errstate(invalid="ignore"):
            inset = table <= thr  # a NaN score compares false
        masks[a] = (inset.astype(np.uint32) << np.arange(K, dtype=np.uint32)[None, :]).sum(1).astype(np.uint16)
        size = inset.sum(1)
        t = tallies[a]
        t[0], t[2] = enters.sum(), bad.sum()
        t[o_size: o_size + K + 1] = np.bincount(size[enters], minlength=K + 1)
        if u is not None:
            m = enters & has_u
            t[o_un: o_un + K + 1] = np.bincount(size[m], minlength=K + 1)
            for sz in range(K + 1):
                t[o_u + sz] = int(uq[m & (size == sz)].sum(dtype=np.uint64))  # integers below 2^53: exact
        cov = inset[np.arange(M), L] & enters & labelled
        t[1] = cov.sum()
        t[o_cov: o_cov + K + 1] = np.bincount(size[cov], minlength=K + 1)
        t[o_cn: o_cn + K] = np.bincount(L[enters & labelled], minlength=K)
        t[o_cn + K: o_cn + 2 * K] = np.bincount(L[cov], minlength=K)
    return masks, tallies


def predict_ref(probs, fit: dict, alphas, labels=None, u=None, mondrian=False, kind="aps", randomized=True, seed=0, lam=0.0, k_reg=1):
    """``predict_sets`` restated: the score table of prediction carries salt 1."""
    return sets_ref(scores_ref(probs, kind, randomized, seed, lam, k_reg, salt=1), fit["qhat"], labels, u, mondrian)


def summary_ref(tallies, alphas, K: int, has_labels=True, has_u=True):
    """What ``ConformalSets.summary()`` returns, from the integer tallies."""
    nan = float("nan")

    def div(a, b):
        return float(a) / float(b) if b else nan

    out = []
    for alpha, w in zip(alphas, np.asarray(tallies)):
        size, cov_size, uq, un = (w[3 + j * (K + 1): 3 + (j + 1) * (K + 1)] for j in range(4))
        cn, ccov = w[3 + 4 * (K + 1): 3 + 4 * (K + 1) + K], w[3 + 4 * (K + 1) + K:]
        rows = int(w[0])
        by_size = [div(c, s) if has_labels else nan for c, s in zip(cov_size, size)]
        seen = [x for x, s in zip(by_size, size) if s]
        out.append({"alpha": float(alpha), "rows": rows, "nan_rows": int(w[2]), "coverage": div(w[1], rows) if has_labels else nan,
                    "mean_size": div(sum(k * int(s) for k, s in enumerate(size)), rows), "empty": div(size[0], rows),
                    "singleton": div(size[1], rows), "singleton_accuracy": div(cov_size[1], size[1]) if has_labels else nan,
                    "size_hist": [int(s) for s in size], "class_n": [int(c) for c in cn],
                    "class_coverage": [div(c, m) if has_labels else nan for c, m in zip(ccov, cn)], "coverage_by_size": by_size,
                    "min_coverage_by_size": min(seen) if has_labels and seen else nan,
                    "u_by_size": [div(float(q) * 2.0 ** -32, m) if has_u else nan for q, m in zip(uq, un)]})
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def conf_case(M: int, K: int, seed: int, pad: bool = True, nan: bool = True, one: bool = True):
    """``calibration_cases.prob_case`` rows (over-confident, some wrong, one in eight padding) with, past 16 rows, a few rows holding a NaN
    (one of them with a valid label, one padding) and a row whose top probability is exactly 1.0f."""
    probs, labels = cc.prob_case(M, K, seed, pad=pad)
    probs = probs.copy()
    if M > 16 and nan:
        probs[3, 1] = np.nan
        probs[M // 2, :] = np.nan
        labels[M // 2] = -1
        labels[3] = 1
    if M > 16 and one:
        probs[5] = 0.0
        probs[5, K - 1] = 1.0
        labels[5] = K - 1
    return probs, labels


def u_case(M: int, seed: int) -> np.ndarray:
    """An uncertainty (M,) float32 with exact 0.0 and 1.0, and past 8 rows a NaN and a value above 1 (rows that carry no u)."""
    u = np.random.default_rng(seed).random(M).astype(np.float32)
    special = [0.0, 1.0] + ([np.nan, 1.5] if M > 8 else [])
    u[: min(M, len(special))] = special[:M]
    return u
