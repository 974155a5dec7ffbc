"""Float64 / int64 numpy restatement of the grouped bootstrap (protoasnet_amd/bootstrap.py, csrc/bootstrap.hip,
include/protoasnet_amd.h) and the seeded case generators of its tests.  The reference has no code for any of this: the restatement IS the
specification the kernels are held to.  Every statistic of a replicate is an existing restatement (tests/selective_cases.py) applied to
the replicate's expanded row list."""
import numpy as np

import selective_cases as sc

M0, M1 = 0xD2511F53, 0xCD9E8D57  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments
MASK = np.uint64(0xFFFFFFFF)
STAT_NAMES = ("acc", "bal_acc", "f1_mean", "auc", "aurc", "error_auroc")


# ---- draws -------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: ``counter`` (..., 4) and ``key`` (..., 2) of 32-bit words -> (..., 4) uint32."""
    c = [np.asarray(counter)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) & MASK for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # < 2^64: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def draws_ref(G: int, b: int, seed: int) -> np.ndarray:
    """The G units replicate ``b`` draws: draw d is word d & 3 of the call with counter (d >> 2, b, 0, 0); unit = (r * G) >> 32."""
    q = np.arange((G + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, b), np.zeros_like(q), np.zeros_like(q)], -1)
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)).reshape(-1)[:G]
    return ((r.astype(np.uint64) * np.uint64(G)) >> np.uint64(32)).astype(np.int64)


def counts_ref(G: int, B: int, seed: int = 0, b0: int = 0) -> np.ndarray:
    """(B, G) int32: counts[b][g] = the number of draws of replicate b0 + b that landed on g."""
    return np.stack([np.bincount(draws_ref(G, b0 + b, seed), minlength=G) for b in range(B)]).astype(np.int32)


# ---- a replicate -------------------------------------------------------------------------------------------------------------------------
def identity_groups(M: int):
    return np.arange(M + 1, dtype=np.int64), np.arange(M, dtype=np.int32)


def replicate_rows(counts_b: np.ndarray, labels: np.ndarray, K_real: int, groups=None) -> np.ndarray:
    """The expanded row list of one replicate: every valid row of group g ``counts_b[g]`` times, in ascending row index."""
    labels = np.asarray(labels)
    M = labels.shape[0]
    offsets, rows = identity_groups(M) if groups is None else (np.asarray(groups[0]), np.asarray(groups[1]))
    w = np.zeros(M, dtype=np.int64)  # a row no group lists never enters
    w[rows] = np.repeat(np.asarray(counts_b, dtype=np.int64), np.diff(offsets))
    w[(labels < 0) | (labels >= K_real)] = 0
    return np.repeat(np.arange(M), w)


def u2_ref(scores: np.ndarray, pos: np.ndarray):
    """(U2, n_pos, n_neg) in int64: U2 = sum over (i positive, j negative) of 2 [s_j < s_i] + [s_j == s_i]."""
    s = np.asarray(scores, dtype=np.float64)
    sp, sn = s[pos], np.sort(s[~pos])
    lt, le = np.searchsorted(sn, sp, "left").astype(np.int64), np.searchsorted(sn, sp, "right").astype(np.int64)
    return int((lt + le).sum()), int(pos.sum()), int((~pos).sum())


def stats_of_rows(probs, labels, u, idx):
    """dict(stats (6,) fp64, cm, u2, n_pos, n_neg) of the expanded row list ``idx``."""
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels)
    K = probs.shape[1]
    p, y = probs[idx], labels[idx]
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (y, p.argmax(1) if len(idx) else y), 1)  # numpy's argmax is the first largest
    acc, bal, f1 = sc.confusion_metrics(cm)
    u2, n_pos, n_neg = (np.zeros(K, dtype=np.int64) for _ in range(3))
    for k in range(K):
        u2[k], n_pos[k], n_neg[k] = u2_ref(p[:, k], y == k)
    if (n_pos > 0).all() and (n_neg > 0).all():
        auc = float((n_pos * (u2 / (2.0 * n_pos * n_neg))).sum() / n_pos.sum())
    else:
        auc = float("nan")  # the one deliberate difference from pasn_roc_auc_ovr: a lost class gives NaN, not 0.0
    aurc = ea = float("nan")
    if u is not None:
        uu = np.asarray(u, dtype=np.float32)[idx]
        aurc = sc.risk_coverage_ref(p, y, uu)["aurc"]  # np.repeat keeps the copies adjacent; equal u goes to the lower position
        ea = sc.error_auroc_ref(p, y, uu) if len(idx) else float("nan")
    return {"stats": np.array([acc, bal, f1, auc, aurc, ea]), "cm": cm, "u2": u2, "n_pos": n_pos, "n_neg": n_neg}


def stats_ref(probs, labels, u=None, groups=None, B: int = 1, seed: int = 0):
    """The B replicates and (row B) the point estimate: dict(stats (B + 1, 6), cm (B + 1, K, K), u2 / n_pos / n_neg (B + 1, K))."""
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels)
    K = probs.shape[1]
    G = labels.shape[0] if groups is None else len(groups[0]) - 1
    counts = np.concatenate([counts_ref(G, B, seed), np.ones((1, G), dtype=np.int32)])
    per = [stats_of_rows(probs, labels, u, replicate_rows(c, labels, K, groups)) for c in counts]
    return {k: np.stack([r[k] for r in per]) for k in per[0]}


def intervals_ref(stats: np.ndarray, confidence: float = 0.95):
    """{name: dict(point, lo, hi, se, n_finite)} from (B + 1, 6) replicate statistics, row B the point estimate."""
    out = {}
    for j, name in enumerate(STAT_NAMES):
        v = stats[:-1, j]
        v = v[np.isfinite(v)]
        if v.size >= 2:
            lo, hi = np.quantile(v, [(1 - confidence) / 2, (1 + confidence) / 2])
            se = float(np.std(v, ddof=1))
        else:
            lo = hi = se = float("nan")
        out[name] = {"point": float(stats[-1, j]), "lo": float(lo), "hi": float(hi), "se": se, "n_finite": int(v.size)}
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def metric_case(M: int, K: int, seed: int, kind: str = "ties"):
    """(probs (M, K) float32 quantised to eighths so that every class column is full of ties, balanced labels i % K, u (M,) float32
    quantised to eighths).  kind: "ties", "nan" (two rows with NaN u) or "pad" (about one padding row, label -1, in eight)."""
    rng = np.random.default_rng(seed)
    labels = (np.arange(M) % K).astype(np.int32)
    z = rng.standard_normal((M, K)) + 1.5 * np.eye(K)[labels]
    probs = (np.round(sc.softmax64(z) * 8) / 8).astype(np.float32)
    u = (rng.integers(0, 8, M) / 8.0).astype(np.float32)
    if kind == "nan":
        u[[1, M - 2]] = np.nan
    elif kind == "pad":
        labels[rng.random(M) < 0.125] = -1
        labels[:K] = np.arange(K)
    elif kind != "ties":
        raise ValueError(kind)
    return probs, labels, u


def random_groups(M: int, seed: int, lo: int = 1, hi: int = 9):
    """Keys of non-contiguous groups of lo .. hi rows over M rows (for ``selective.build_groups``)."""
    rng = np.random.default_rng(seed)
    keys = []
    while len(keys) < M:
        keys += [len(keys)] * int(rng.integers(lo, hi + 1))
    keys = np.array(keys[:M])
    return keys[rng.permutation(M)].tolist()
