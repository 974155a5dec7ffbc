"""Float64 / int64 numpy restatement of the calibration statistics and of temperature scaling (protoasnet_amd/calibration.py,
csrc/calibration.hip, include/protoasnet_amd.h) and the seeded case generators of their tests.  The reference has no code for any of
this: the restatement IS the specification the kernels are held to."""
import numpy as np

import bootstrap_cases as bc

STAT_NAMES = ("ece", "mce", "cw_ece", "brier", "nll", "conf_gap")
FLT_MIN = float(np.finfo(np.float32).tiny)
BETA_MIN, BETA_MAX, STEPS = 1.0 / 64.0, 64.0, 48
INT_KEYS = ("n", "hit", "qsum", "cn", "cpos", "cq", "skipped")


# ---- bins --------------------------------------------------------------------------------------------------------------------------------
def bin_of(c, n_bins: int) -> int:
    """The bin of one fp32 confidence in [0, 1]: min(n_bins - 1, (int)((double)c * n_bins))."""
    return min(n_bins - 1, int(float(np.float32(c)) * n_bins))


def q_of(c) -> int:
    """(uint64)((double)c * 2^32) of one fp32 confidence in [0, 1]."""
    return int(float(np.float32(c)) * 4294967296.0)


def row_units(M: int, groups=None) -> np.ndarray:
    """unit_i of every row: its group, -1 where no group lists it; without groups the row itself."""
    if groups is None:
        return np.arange(M, dtype=np.int64)
    unit = np.full(M, -1, dtype=np.int64)
    unit[np.asarray(groups[1])] = np.repeat(np.arange(len(groups[0]) - 1), np.diff(np.asarray(groups[0])))
    return unit


def _histogram(bins, w, q, n_bins: int, flag=None):
    """(sum w, sum w flag, sum w q) per bin as int64 / int64 / uint64.  bincount adds in float64: the counts stay below 2^53, and q goes in
    as two halves whose weighted sums do too (w sums to less than 2^31, a half is below 2^17), so every number is exact."""
    wf = w.astype(np.float64)
    n = np.bincount(bins, wf, n_bins).astype(np.int64)
    hit = np.bincount(bins, wf * flag, n_bins).astype(np.int64)
    hi = np.bincount(bins, wf * (q >> np.uint64(17)).astype(np.float64), n_bins).astype(np.uint64)
    lo = np.bincount(bins, wf * (q & np.uint64(0x1FFFF)).astype(np.float64), n_bins).astype(np.uint64)
    return n, hit, (hi << np.uint64(17)) + lo


def row_terms(probs, labels, n_bins: int, conf=None):
    """What every output row shares: per row the validity, the top-label (binned?, bin, q, hit), the same per class, and the fp64 Brier
    and NLL terms."""
    probs, labels = np.asarray(probs, dtype=np.float32), np.asarray(labels).astype(np.int64)
    M, K = probs.shape
    valid = (labels >= 0) & (labels < K)
    L = np.where(valid, labels, 0)
    c = probs.max(1) if conf is None else np.asarray(conf, dtype=np.float32)

    def words(c32):
        with np.errstate(invalid="ignore"):
            ok = (c32 >= 0) & (c32 <= 1)  # NaN fails both
        c64 = np.where(ok, c32, 0).astype(np.float64)
        return ok, np.minimum(n_bins - 1, (c64 * n_bins).astype(np.int64)), (c64 * 4294967296.0).astype(np.uint64)

    d = probs.astype(np.float64) - (np.arange(K)[None, :] == L[:, None])
    return {"K": K, "valid": valid, "top": words(c), "hit": probs.argmax(1) == L,  # numpy's argmax is the first largest
            "cls": [words(probs[:, k]) + (L == k,) for k in range(K)], "brier": (d * d).sum(1),
            "nll": -np.log(np.maximum(probs[np.arange(M), L].astype(np.float64), FLT_MIN))}


def bins_of_weights(probs, labels, w, n_bins: int, conf=None, terms=None):
    """One output row from per-row integer weights ``w`` (0 for a row that does not enter): dict of the integer arrays and ``stats``."""
    t = row_terms(probs, labels, n_bins, conf) if terms is None else terms
    K = t["K"]
    w = np.where(t["valid"], np.asarray(w, dtype=np.int64), 0)
    Wv = int(w.sum())
    ok, bins, q = t["top"]
    n, hit, qsum = _histogram(bins[ok], w[ok], q[ok], n_bins, t["hit"][ok])
    skipped = int(w[~ok].sum())
    per = [_histogram(b[o], w[o], qq[o], n_bins, pos[o]) for o, b, qq, pos in t["cls"]]
    cn, cpos, cq = (np.stack([p[j] for p in per]) for j in range(3))
    W = int(n.sum())
    gap = [float(np.float64(qj) * 2.0 ** -32) - float(hj) for qj, hj in zip(qsum, hit)]  # conf_j - hit_j
    stats = np.full(6, float("nan"))
    if W > 0:
        stats[0] = sum(abs(g) for g in gap) / W
        stats[1] = max(abs(g) / int(nj) for g, nj in zip(gap, n) if nj > 0)
        stats[5] = sum(gap) / W
    if Wv > 0:
        stats[2] = float(np.abs(cpos.astype(np.float64) - cq.astype(np.float64) * 2.0 ** -32).sum()) / Wv / K
        stats[3] = float((w * t["brier"]).sum()) / Wv
        stats[4] = float((w * t["nll"]).sum()) / Wv
    return {"n": n, "hit": hit, "qsum": qsum.view(np.int64), "cn": cn, "cpos": cpos, "cq": cq.view(np.int64), "skipped": np.int64(skipped),
            "stats": stats}


def reliability_ref(probs, labels, n_bins: int, conf=None, groups=None, B: int = 0, seed: int = 0):
    """The B replicates and (row B) the point estimate, stacked: the weights of replicate b are ``counts_ref(G, B, seed)[b][unit_i]``, the
    point estimate's are 1; a row no group lists has weight 0 in both."""
    M = np.asarray(labels).shape[0]
    unit = row_units(M, groups)
    G = M if groups is None else len(groups[0]) - 1
    listed = unit >= 0
    rows = [np.where(listed, c[np.maximum(unit, 0)], 0) for c in (bc.counts_ref(G, B, seed) if B else [])] + [listed.astype(np.int64)]
    terms = row_terms(probs, labels, n_bins, conf)
    per = [bins_of_weights(probs, labels, w, n_bins, conf, terms) for w in rows]
    return {k: np.stack([r[k] for r in per]) for k in per[0]}


def summary_ref(point: dict, n_bins: int):
    """What ``Reliability.summary()`` returns, from one output row of the restatement."""
    res = {name: float(v) for name, v in zip(STAT_NAMES, point["stats"])}
    res["skipped"] = int(point["skipped"])
    nan = float("nan")
    res["bins"] = []
    for j in range(n_bins):
        nj, conf = int(point["n"][j]), float(np.float64(np.uint64(point["qsum"][j])) * 2.0 ** -32)
        res["bins"].append({"lo": j / n_bins, "hi": (j + 1) / n_bins, "n": nj, "accuracy": float(point["hit"][j]) / nj if nj else nan,
                            "confidence": conf / nj if nj else nan})
    return res


# ---- temperature -------------------------------------------------------------------------------------------------------------------------
def _moments(z, y, beta):
    """(g, g', g'') at beta over the rows z (Mv, K) fp64 with labels y."""
    d = z - z.max(1, keepdims=True)
    e = np.exp(beta * d)
    S = e.sum(1)
    mean = (e * d).sum(1) / S
    var = (e * (d - mean[:, None]) ** 2).sum(1) / S
    dl = d[np.arange(len(y)), y]
    return float((np.log(S) - beta * dl).sum()), float((mean - dl).sum()), float(var.sum())


def temperature_ref(logits, labels, K_real: int):
    """[beta, g(1) / Mv, g(beta) / Mv, status] by the header's safeguarded Newton iteration, in float64."""
    labels = np.asarray(labels).astype(np.int64)
    ok = (labels >= 0) & (labels < K_real)
    z, y = np.asarray(logits, dtype=np.float32)[ok][:, :K_real].astype(np.float64), labels[ok]
    if len(y) == 0:
        return [1.0, float("nan"), float("nan"), 3]
    g1 = _moments(z, y, 1.0)[0] / len(y)
    if _moments(z, y, BETA_MIN)[1] >= 0.0:
        return [BETA_MIN, g1, _moments(z, y, BETA_MIN)[0] / len(y), 1]
    if _moments(z, y, BETA_MAX)[1] <= 0.0:
        return [BETA_MAX, g1, _moments(z, y, BETA_MAX)[0] / len(y), 2]
    lo, hi, beta = BETA_MIN, BETA_MAX, 1.0
    for _ in range(STEPS):
        _, d1, d2 = _moments(z, y, beta)
        if d1 > 0.0:
            hi = beta
        elif d1 < 0.0:
            lo = beta
        else:
            lo = hi = beta
        nt = beta - d1 / d2 if d2 > 0.0 else float("nan")
        beta = nt if d2 > 0.0 and lo < nt < hi else 0.5 * (lo + hi)
    return [beta, g1, _moments(z, y, beta)[0] / len(y), 0]


def scaled_probs_ref(logits, K_real: int, beta: float) -> np.ndarray:
    """softmax(beta z) over the first K_real columns in float64, rounded once to float32."""
    z = np.asarray(logits, dtype=np.float32)[:, :K_real].astype(np.float64)
    e = np.exp(beta * (z - z.max(1, keepdims=True)))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def prob_case(M: int, K: int, seed: int, pad: bool = False):
    """(probs (M, K) float32 from over-confident logits, labels (M,) int32 drawn from the true softmax): most confidences in the top
    bins, some rows wrong.  pad: about one row in eight is padding, label -1 or K alternately."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((M, K))
    p_true = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    labels = (p_true.cumsum(1) < rng.random((M, 1))).sum(1).clip(0, K - 1).astype(np.int32)
    e = np.exp(2.5 * (z - z.max(1, keepdims=True)))
    probs = (e / e.sum(1, keepdims=True)).astype(np.float32)
    if pad:
        bad = np.flatnonzero(rng.random(M) < 0.125)
        labels[bad] = np.where(np.arange(bad.size) % 2 == 0, -1, K)
    return probs, labels


def conf_case(M: int, seed: int, bad: bool = False) -> np.ndarray:
    """A confidence override (M,) float32 holding exact 0.0, 1.0 and the fp32 bin edges 0.3 / 0.7 (cycled over the first rows); bad: also
    NaN, 1.5 and -0.25."""
    rng = np.random.default_rng(seed)
    conf = rng.random(M).astype(np.float32)
    special = [0.0, 1.0, 0.3, 0.7] + ([np.nan, 1.5, -0.25] if bad else [])
    conf[: min(M, len(special))] = special[:M]
    if bad and M > 20:
        conf[rng.integers(7, M, M // 10)] = np.nan
    return conf


# (M, K_real, what the true logits were multiplied by): the interior cases of the fit -- the root lies near 1 / scale
FIT_CASES = [(8, 2, 3.0), (257, 4, 3.0), (5000, 3, 0.4), (5000, 16, 5.0), (70000, 4, 2.0)]


def logit_case(M: int, K: int, scale: float, seed: int = 0, extra: int = 0):
    """(logits (M, K + extra) float32 = scale x the true logits, labels drawn from the true softmax); ``extra`` more columns (the
    abstention logit) that no scaled probability may read."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((M, K))
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    labels = (p.cumsum(1) < rng.random((M, 1))).sum(1).clip(0, K - 1).astype(np.int32)
    logits = np.concatenate([scale * z, 9.0 * rng.standard_normal((M, extra))], 1).astype(np.float32)
    return logits, labels


def separable_case(M: int, K: int, seed: int = 0):
    """The label is the strict argmax of every row: g' < 0 on the whole bracket."""
    logits, _ = logit_case(M, K, 1.0, seed)
    return logits, logits.argmax(1).astype(np.int32)


def all_wrong_case(M: int, K: int, seed: int = 0):
    """The label is the strict argmin of every row: g' > 0 on the whole bracket."""
    logits, _ = logit_case(M, K, 1.0, seed)
    return logits, logits.argmin(1).astype(np.int32)
