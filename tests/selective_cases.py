"""Float64 numpy restatements of the selective-prediction definitions (protoasnet_amd/selective.py, csrc/selective.hip,
include/protoasnet_amd.h) and the seeded case generators of their tests.  The reference has no code for any of this: the restatements ARE
the specification the kernels are held to."""
import numpy as np

from metric_cases import auc_ovr_weighted


# ---- uncertainty scores ----------------------------------------------------------------------------------------------------------------
def softmax64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def uncertainty_ref(logits: np.ndarray, K_real: int, mode: int) -> np.ndarray:
    """mode 0: 1 - max softmax(real classes); 1: the last column of the softmax over all columns; 2: sigmoid of the last column."""
    z = np.asarray(logits, dtype=np.float64)
    if mode == 0:
        return 1.0 - softmax64(z[:, :K_real]).max(1)
    if mode == 1:
        return softmax64(z)[:, -1]
    return 1.0 / (1.0 + np.exp(-z[:, -1]))


def score_logits(M: int, K: int, seed: int) -> np.ndarray:
    """(M, K) float32 logits, uniform in [-4, 4]."""
    return np.random.default_rng(seed).uniform(-4.0, 4.0, (M, K)).astype(np.float32)


# ---- confusion-matrix metrics (trainer.confusion_to_metrics) ----------------------------------------------------------------------------
def confusion_metrics(cm: np.ndarray):
    """(accuracy, balanced accuracy, mean F1) of a (K, K) confusion matrix [true][predicted]: trace / n; the mean over the classes with
    support > 0 of tp / support; the mean over ALL classes of 2 tp / (support + predicted), 0 for a zero denominator."""
    cm = np.asarray(cm, dtype=np.float64)
    tp, support, predicted = np.diag(cm), cm.sum(1), cm.sum(0)
    present = support > 0
    bal = float(np.mean(tp[present] / support[present])) if present.any() else 0.0
    denom = support + predicted
    f1 = np.where(denom > 0, 2.0 * tp / np.where(denom > 0, denom, 1.0), 0.0)
    return float(tp.sum() / cm.sum()) if cm.sum() > 0 else 0.0, bal, float(f1.mean())


# ---- risk-coverage -----------------------------------------------------------------------------------------------------------------------
def order_ref(u: np.ndarray, labels: np.ndarray, K_real: int) -> np.ndarray:
    """The valid rows (0 <= label < K_real) by ascending u; equal u: the lower index first; NaN last, by index."""
    u = np.asarray(u)
    idx = np.nonzero((labels >= 0) & (labels < K_real))[0]
    nan = np.isnan(u[idx])
    return idx[np.lexsort((idx, np.where(nan, 0.0, u[idx]), nan))]  # the last key is the primary one


def risk_coverage_ref(probs: np.ndarray, labels: np.ndarray, u: np.ndarray):
    """dict(order, acc, bal_acc, f1_mean, threshold, aurc, counts) over the Mv valid rows, from the SAME float32 arrays the kernel reads."""
    probs, u, labels = np.asarray(probs, dtype=np.float32), np.asarray(u, dtype=np.float32), np.asarray(labels)
    K = probs.shape[1]
    order = order_ref(u, labels, K)
    pred = probs.argmax(1)  # numpy's argmax is the first largest
    cm = np.zeros((K, K), dtype=np.int64)
    acc, bal, f1 = [], [], []
    for i in order:
        cm[labels[i], pred[i]] += 1
        a, b, f = confusion_metrics(cm)
        acc.append(a)
        bal.append(b)
        f1.append(f)
    acc = np.array(acc, dtype=np.float64)
    return {"order": order.astype(np.int32), "acc": acc, "bal_acc": np.array(bal), "f1_mean": np.array(f1), "threshold": u[order],
            "aurc": float(np.mean(1.0 - acc)) if order.size else float("nan"),
            "counts": np.array([order.size, int(np.isnan(u[order]).sum())], dtype=np.int64)}


def error_auroc_ref(probs: np.ndarray, labels: np.ndarray, u: np.ndarray) -> float:
    """AUROC of u as a detector of the wrong predictions (NaN when every valid row is right or every one is wrong)."""
    probs, u, labels = np.asarray(probs, dtype=np.float32), np.asarray(u, dtype=np.float32), np.asarray(labels)
    valid = (labels >= 0) & (labels < probs.shape[1])
    wrong = np.where(valid, (probs.argmax(1) != labels).astype(np.int64), -1)
    return float(auc_ovr_weighted(np.stack([np.float32(1.0) - u, u], 1), wrong, 2)[1][1])


def curve_case(M: int, K: int, seed: int, kind: str = "ties"):
    """(probs (M, K) float32, labels (M,) int32 with about one padding row (-1) in eight interleaved, u (M,) float32 quantised to 8
    levels so ties are everywhere).  kind: "ties", "equal" (all u equal) or "nan" (two valid rows with NaN u)."""
    rng = np.random.default_rng(seed)
    probs = softmax64(rng.uniform(-4.0, 4.0, (M, K))).astype(np.float32)
    labels = rng.integers(0, K, M).astype(np.int32)
    if M > 1:
        labels[rng.random(M) < 0.125] = -1
        labels[0] = 0  # (never all padding)
    u = (rng.integers(0, 8, M) / 8.0).astype(np.float32)
    if kind == "equal":
        u[:] = 0.25
    elif kind == "nan":
        valid = np.nonzero(labels >= 0)[0]
        u[valid[[1, -2]]] = np.nan
    elif kind != "ties":
        raise ValueError(kind)
    return probs, labels, u


# ---- one prediction per group ------------------------------------------------------------------------------------------------------------
def group_ref(probs: np.ndarray, u: np.ndarray, labels: np.ndarray, offsets: np.ndarray, rows: np.ndarray):
    """dict(p_mean, p_conf, u_mean, label, count, status): fp64 sums in the listed row order."""
    probs, u = np.asarray(probs, dtype=np.float32), np.asarray(u, dtype=np.float32)
    G, K = len(offsets) - 1, probs.shape[1]
    out = {"p_mean": np.zeros((G, K)), "p_conf": np.zeros((G, K)), "u_mean": np.zeros(G), "label": np.zeros(G, np.int32),
           "count": np.zeros(G, np.int32), "status": np.zeros(2, np.int32)}
    for g in range(G):
        mine = rows[offsets[g]: offsets[g + 1]]
        sp, spc, sw, su = np.zeros(K), np.zeros(K), np.float64(0.0), np.float64(0.0)
        for i in mine:
            w = np.float64(1.0) - np.float64(u[i])
            p = probs[i].astype(np.float64)
            sp, spc, sw, su = sp + p, spc + w * p, sw + w, su + np.float64(u[i])
            out["status"][1] += bool(np.isnan(u[i]) or np.isnan(probs[i]).any())
        n = len(mine)
        out["p_mean"][g] = sp / n
        out["p_conf"][g] = out["p_mean"][g] if sw == 0.0 else spc / sw
        out["u_mean"][g] = su / n
        out["label"][g], out["count"][g] = labels[mine[0]], n
        out["status"][0] += bool((labels[mine] != labels[mine[0]]).any())
    return out


def group_case(seed: int, K: int = 3):
    """Rows, keys and labels of the group tests: 50 groups of one row, a group of 700 rows scattered among the others, ordinary groups of
    2 .. 9 rows, and one group whose u are all exactly 1 (its confidence weights sum to 0).  Returns (probs, u, labels, keys)."""
    rng = np.random.default_rng(seed)
    keys = [f"one{g}" for g in range(50)] + ["big"] * 700 + ["sure"] * 5
    for g in range(40):
        keys += [f"cine{g}"] * int(rng.integers(2, 10))
    keys = [keys[i] for i in rng.permutation(len(keys))]
    names = sorted(set(keys))
    label_of = {k: int(rng.integers(0, K)) for k in names}
    M = len(keys)
    probs = softmax64(rng.uniform(-4.0, 4.0, (M, K))).astype(np.float32)
    u = rng.random(M).astype(np.float32)
    u[[i for i, k in enumerate(keys) if k == "sure"]] = 1.0
    labels = np.array([label_of[k] for k in keys], dtype=np.int32)
    return probs, u, labels, keys
