"""Float64 / int64 numpy restatement of the ordinal evaluation (protoasnet_amd/ordinal.py, csrc/ordinal.hip, include/protoasnet_amd.h)
and the seeded case generators of its tests.  The reference has no code for any of this: the restatement IS the specification the kernels
are held to.  Everything is vectorised over the distinct scores (np.unique, bincount, cumsum); a replicate is the sample with integer
weights, and the draws are tests/bootstrap_cases.py's own."""
import numpy as np

import bootstrap_cases as bc
import selective_cases as sc

AGREEMENT_NAMES = ("mae", "within_one", "under", "over", "kappa_linear", "kappa_quadratic")
NAN = float("nan")


# ---- agreement ---------------------------------------------------------------------------------------------------------------------------
def agreement_ref(cm) -> np.ndarray:
    """(6,) fp64 from one confusion matrix [true][pred]: integer sums, then ONE fp64 expression each."""
    cm = np.asarray(cm, dtype=np.int64)
    K = cm.shape[0]
    i, j = np.indices((K, K))
    d = np.abs(i - j).astype(np.int64)
    n = int(cm.sum())
    if n == 0:
        return np.full(6, NAN)
    r, c = cm.sum(1), cm.sum(0)
    rc = np.outer(r, c)
    dn = np.float64(n)
    out = [np.float64(int((d * cm).sum())) / dn, np.float64(int(cm[d <= 1].sum())) / dn, np.float64(int(cm[j < i].sum())) / dn,
           np.float64(int(cm[j > i].sum())) / dn]
    for w in (d, d * d):
        A, E = int((w * cm).sum()), int((w * rc).sum())
        out.append(np.float64(1.0) - (dn * np.float64(A)) / np.float64(E) if E != 0 else NAN)
    return np.array(out, dtype=np.float64)


def confusion_ref(probs, labels, w=None) -> np.ndarray:
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels)
    K = probs.shape[1]
    ok = (labels >= 0) & (labels < K)
    w = np.ones(len(labels), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (labels[ok], probs[ok].argmax(1)), w[ok])  # numpy's argmax is the first largest
    return cm


# ---- cuts --------------------------------------------------------------------------------------------------------------------------------
def cut_scores_ref(probs) -> np.ndarray:
    """(K - 1, M) float32: s_c = p[c] + p[c + 1] + ... + p[K - 1], every add rounded to fp32, in that order."""
    p = np.asarray(probs, dtype=np.float32)
    K = p.shape[1]
    out = []
    for c in range(1, K):
        s = p[:, c].copy()
        for k in range(c + 1, K):
            s = (s + p[:, k]).astype(np.float32)
        out.append(s)
    return np.stack(out)


def weights_ref(counts_b, labels, K: int, groups=None) -> np.ndarray:
    """(M,) int64: the number of copies of every row in one replicate (0: padding, or a row that no group lists)."""
    labels = np.asarray(labels)
    M = labels.shape[0]
    offsets, rows = bc.identity_groups(M) if groups is None else (np.asarray(groups[0]), np.asarray(groups[1]))
    w = np.zeros(M, dtype=np.int64)
    w[rows] = np.repeat(np.asarray(counts_b, dtype=np.int64), np.diff(offsets))
    w[(labels < 0) | (labels >= K)] = 0
    return w


def cut_ref(s, pos, w, specificities=(), sensitivities=(), fixed=()):
    """One cut with integer weights: dict(P, N, u2, auc, ap, theta (T,) float32, tally (T, 2) int64, fix (F, 2) int64); the operating
    points are the specificities, the sensitivities, then Youden's."""
    s, pos, w = np.asarray(s, dtype=np.float32), np.asarray(pos, dtype=bool), np.asarray(w, dtype=np.int64)
    T = len(specificities) + len(sensitivities) + 1
    P, N = int(w[pos].sum()), int(w[~pos].sum())
    fix = np.array([[int(w[pos & (s >= np.float32(t))].sum()), int(w[~pos & (s >= np.float32(t))].sum())] for t in fixed],
                   dtype=np.int64).reshape(len(fixed), 2)
    live = w > 0
    v, inv = np.unique(s[live], return_inverse=True)  # ascending distinct scores of the rows with weight
    tp = np.zeros(len(v), dtype=np.int64)
    fp = np.zeros(len(v), dtype=np.int64)
    np.add.at(tp, inv[pos[live]], w[live][pos[live]])
    np.add.at(fp, inv[~pos[live]], w[live][~pos[live]])
    TP, FP = np.cumsum(tp[::-1])[::-1], np.cumsum(fp[::-1])[::-1]  # at scores >= v
    nlt = N - FP  # negative weight strictly below v
    u2 = int((tp * (2 * nlt + fp)).sum())
    out = {"P": P, "N": N, "u2": u2, "fix": fix}
    if P == 0 or N == 0:
        out.update(auc=NAN, ap=NAN, theta=np.full(T, np.nan, dtype=np.float32), tally=np.zeros((T, 2), dtype=np.int64))
        return out
    out["auc"] = float(np.float64(u2) / (2.0 * np.float64(P) * np.float64(N)))
    has = tp > 0
    out["ap"] = float(np.sum((tp[has].astype(np.float64) / np.float64(P)) * (TP[has].astype(np.float64) / (TP[has] + FP[has]).astype(np.float64))))
    cand = np.concatenate([v, np.array([np.inf], dtype=np.float32)])  # ascending; +inf: nobody positive
    cTP, cFP = np.concatenate([TP, [0]]).astype(np.int64), np.concatenate([FP, [0]]).astype(np.int64)
    pick = []
    for tau in specificities:  # the smallest candidate that reaches the specificity
        pick.append(int(np.nonzero((N - cFP).astype(np.float64) / np.float64(N) >= tau)[0][0]))
    for tau in sensitivities:  # the largest candidate that reaches the sensitivity
        pick.append(int(np.nonzero(cTP.astype(np.float64) / np.float64(P) >= tau)[0][-1]))
    J = cTP * N - cFP * P
    pick.append(len(J) - 1 - int(np.argmax(J[::-1])))  # ties to the larger theta
    out["theta"] = cand[pick].astype(np.float32)
    out["tally"] = np.stack([cTP[pick], cFP[pick]], axis=1)
    return out


def screen_ref(probs, labels, specificities=(0.9,), sensitivities=(0.9,), groups=None, B: int = 0, seed: int = 0, fixed=None, counts=None):
    """``ordinal.screen``'s outputs as numpy arrays (row b < B replicate b, row B the sample): pn (B + 1, C, 2), u2 (B + 1, C), stats
    (B + 1, C, 2), op_theta (B + 1, C, T) float32, op_tally (B + 1, C, T, 2), fix_tally (B + 1, C, F, 2).  ``fixed``: (C, F) float32.
    ``counts`` (B, G): the resamples, instead of bootstrap_cases' own draws."""
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels)
    M, K = probs.shape
    C, T = K - 1, len(specificities) + len(sensitivities) + 1
    fixed = np.zeros((C, 0), dtype=np.float32) if fixed is None else np.asarray(fixed, dtype=np.float32).reshape(C, -1)
    F = fixed.shape[1]
    G = M if groups is None else len(groups[0]) - 1
    if counts is None:
        counts = bc.counts_ref(G, B, seed) if B else np.zeros((0, G), dtype=np.int32)
    counts = np.concatenate([np.asarray(counts, dtype=np.int64).reshape(B, G), np.ones((1, G), dtype=np.int64)])
    scores = cut_scores_ref(probs)
    out = {"pn": np.zeros((B + 1, C, 2), dtype=np.int64), "u2": np.zeros((B + 1, C), dtype=np.int64), "stats": np.zeros((B + 1, C, 2)),
           "op_theta": np.zeros((B + 1, C, T), dtype=np.float32), "op_tally": np.zeros((B + 1, C, T, 2), dtype=np.int64),
           "fix_tally": np.zeros((B + 1, C, F, 2), dtype=np.int64)}
    for b in range(B + 1):
        w = weights_ref(counts[b], labels, K, groups)
        for c in range(C):
            r = cut_ref(scores[c], labels >= c + 1, w, specificities, sensitivities, fixed[c])
            out["pn"][b, c] = r["P"], r["N"]
            out["u2"][b, c] = r["u2"]
            out["stats"][b, c] = r["auc"], r["ap"]
            out["op_theta"][b, c], out["op_tally"][b, c], out["fix_tally"][b, c] = r["theta"], r["tally"], r["fix"]
    return out


def expand(probs, labels, w):
    """The replicate as a plain row list (np.repeat): what an unweighted implementation is fed."""
    idx = np.repeat(np.arange(len(labels)), np.asarray(w, dtype=np.int64))
    return np.asarray(probs)[idx], np.asarray(labels)[idx]


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def ordinal_case(M: int, K: int, seed: int, denom: int = 16, pad: float = 0.0):
    """(probs (M, K) float32 in 1 / denom steps: every cut score is exact and full of ties; labels (M,) int32, the grade driving the
    probabilities so that neighbouring grades are confused most; ``pad``: the share of padding rows (label -1 or K), interleaved)."""
    rng = np.random.default_rng(seed)
    labels = (np.arange(M) % K).astype(np.int32)
    z = -0.8 * (np.arange(K)[None, :] - labels[:, None] - 0.6 * rng.standard_normal((M, 1))) ** 2 + 0.5 * rng.standard_normal((M, K))
    probs = (np.round(sc.softmax64(z) * denom) / denom).astype(np.float32)
    if pad > 0.0 and M > K:
        bad = rng.random(M) < pad
        bad[:K] = False
        labels[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, K).astype(np.int32)
    return probs, labels
