"""Inputs and numpy restatements of the evaluation metrics (protoasnet_amd/metrics.py, csrc/eval_metrics.hip).

The recipes here are the ones tests/golden/make_golden_metrics.py fed to the reference's own code (SparsityMetric, sklearn's
roc_auc_score, BaseAgent.create_pred_log_df); the restatements are what the kernels are held to on inputs the fixture does not cover."""
import numpy as np
import torch

LEVEL = 0.8


# ---- sparsity: src/utils/metrics.py:16-25 ---------------------------------------------------------------------------------------------
def sparsity_batches():
    """{case: [batch (N, P) float32 in [0, 1]]}: P = 40 and P = 30, uniform and peaked, one all-zero row."""
    g = torch.Generator().manual_seed(9)
    out = {}
    for P in (40, 30):
        bs = [torch.rand(16, P, generator=g), torch.rand(16, P, generator=g) ** 6, torch.rand(8, P, generator=g) ** 12]
        bs[1][5] = 0.0  # an all-zero row: 0 / 0 = NaN everywhere, the reference's argmax of an all-false mask gives 0
        out[f"p{P}"] = [b.contiguous() for b in bs]
    return out


def sparsity_rows(sim: np.ndarray, level: float = LEVEL):
    """Per-row SparsityMetric index and the margin of the deciding prefix to ``level`` (inf for rows decided by NaN).  Row sum in fp64
    rounded once, IEEE fp32 division, descending sort, fp64 prefix sums each rounded to fp32 (torch's CPU cumsum), first prefix >= level
    (fp32), 0 when none."""
    sim = np.asarray(sim, dtype=np.float32)
    lv = np.float32(level)
    res, margin = [], []
    for row in sim:
        rs = np.float32(row.astype(np.float64).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            norm = row / rs
        if np.isnan(norm).any():
            res.append(0)
            margin.append(np.inf)
            continue
        srt = -np.sort(-norm)
        pre = np.cumsum(srt.astype(np.float64)).astype(np.float32)
        hit = np.nonzero(pre >= lv)[0]
        res.append(int(hit[0]) if hit.size else 0)
        margin.append(float(np.min(np.abs(pre.astype(np.float64) - float(lv)))))
    return np.array(res, dtype=np.int64), np.array(margin)


# ---- diversity: Video_XProtoNet_e2e.py:159-171 -----------------------------------------------------------------------------------------
def diversity_counts(sim: np.ndarray, P_cls: int, k_cls: int = 5, k_abs: int = 2) -> np.ndarray:
    sim = np.asarray(sim, dtype=np.float32)
    counts = np.zeros(sim.shape[1], dtype=np.int64)
    for lo, hi, k in ((0, P_cls, k_cls), (P_cls, sim.shape[1], k_abs)):
        if hi <= lo:
            continue
        order = np.argsort(-sim[:, lo:hi], axis=1, kind="stable")[:, : min(k, hi - lo)]  # ties: the lower index first
        np.add.at(counts, lo + order, 1)
    return counts


# ---- AUC: roc_auc_score(average="weighted", multi_class="ovr") as the exact Mann-Whitney statistic ------------------------------------
def _rankdata_avg(x: np.ndarray) -> np.ndarray:
    order = np.argsort(x, kind="stable")
    xs = x[order]
    ranks = np.empty(len(x), dtype=np.float64)
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and xs[j + 1] == xs[i]:
            j += 1
        ranks[order[i: j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return ranks


def auc_ovr_weighted(probs: np.ndarray, labels: np.ndarray, K: int):
    """(weighted AUC, per-class AUCs): average ranks per class over the rows with label >= 0; 0.0 (and NaN per class) where sklearn
    raises -- a class without positives or negatives, a label >= K, a NaN score."""
    probs = np.asarray(probs, dtype=np.float32)
    labels = np.asarray(labels)
    keep = labels >= 0
    p, y = probs[keep], labels[keep]
    if np.isnan(p).any() or (y >= K).any():
        return 0.0, np.full(K, np.nan)
    per, ok = np.full(K, np.nan), True
    npos_all = np.array([(y == k).sum() for k in range(K)], dtype=np.float64)
    for k in range(K):
        pos = y == k
        npos, nneg = int(pos.sum()), int((~pos).sum())
        if npos == 0 or nneg == 0:
            ok = False
            continue
        r = _rankdata_avg(p[:, k].astype(np.float64))
        u = r[pos].sum() - npos * (npos + 1) / 2.0
        per[k] = u / (float(npos) * float(nneg))
    if not ok:
        return 0.0, per
    return float((npos_all * per).sum() / npos_all.sum()), per


def auc_cases():
    """{case: (probs (M, 3) float32 rows summing to ~1, labels (M,) int64)}"""
    rng = np.random.default_rng(19)

    def softmax(z):
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)

    out = {}
    y = rng.integers(0, 3, 200)
    out["random"] = (softmax(rng.standard_normal((200, 3)) + 0.8 * np.eye(3)[y]), y)
    y = rng.integers(0, 3, 300)
    q = np.round(softmax(rng.standard_normal((300, 3)) + np.eye(3)[y]) * 8) / 8  # heavy ties
    q[:, 2] = 1.0 - q[:, 0] - q[:, 1]
    out["tied"] = (q.astype(np.float32), y)
    y = np.repeat(np.arange(3), 10)
    out["perfect"] = (np.eye(3, dtype=np.float32)[y] * np.float32(0.7) + np.float32(0.1), y)  # rows 0.8, 0.1, 0.1
    y = rng.integers(0, 2, 50)  # class 2 missing: sklearn raises, the reference logs and sets 0
    out["missing"] = (softmax(rng.standard_normal((50, 3))), y)
    return out


# ---- prediction log: base.py:195-211 ----------------------------------------------------------------------------------------------------
LOGIT_NAMES = ["No AS", "Early AS", "Significant AS", "abstain"]


def pred_log_batch(optional: bool = True):
    """A hand batch with every optional key (or none) and an abstain logit; logits exercise float32 formatting."""
    b = {"filename": ["a.mat", "b, c.mat", 'q"uote.mat'], "target_AS": torch.tensor([0, 2, 1])}
    if optional:
        b.update(interval_idx=torch.tensor([0, 3, 1]), window_start=torch.tensor([0, 12, 48]), window_end=torch.tensor([32, 44, 80]),
                 original_length=torch.tensor([90, 90, 120]))
    logits = torch.tensor([[0.1, -1.5, 2.25, 1e-8], [123456.79, -0.0, 3.0, float("nan")], [1e20, -7.1234567, 0.33333334, 5.5]],
                          dtype=torch.float32)
    return b, logits
