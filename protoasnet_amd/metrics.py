"""Evaluation metrics of the reference's epoch loop, accumulated on the device (``csrc/eval_metrics.hip``).

The reference ends every ``val`` / ``val_push`` / ``test`` epoch with the weighted one-vs-rest ROC AUC, the prototype sparsity
(``src/utils/metrics.py``), the prototype diversity counters and the per-prototype similarity sums, and writes a per-clip prediction CSV
(``Video_XProtoNet_e2e.py:154-173, 221-233, 240-319``; ``XProtoNet_Base.py:499-567``; ``base.py:195-211``).  There every batch costs
host round trips (``.cpu()``, numpy, sklearn).  Here:

* ``SparsityMetric``: drop-in for ``src.utils.metrics.SparsityMetric`` (same constructor, ``update`` / ``update_and_compute`` /
  ``compute`` / ``reset`` / ``__call__``), its state two int64 counters on the device, one ``pasn_eval_batch_stats`` launch per batch.
* ``EpochEvaluator``: everything an epoch needs, one launch per batch (``update``, no host synchronisation) into device epoch buffers
  (real-class probabilities, labels, optionally the logits) and counters; ``finish`` runs the AUC kernel (two launches) and reads the
  results once.
* ``roc_auc_ovr_weighted``: the AUC kernel on its own, for device tensors.
* ``write_prediction_log``: the reference's CSV (pandas' ``to_csv`` of ``create_pred_log_df``'s frame), in pure Python.

Numeric rules ("Evaluation metrics"): sparsity is the index -- not the count -- of the first sorted prefix >= ``level``, 0
when there is none; diversity ties go to the lower prototype index; AUC is the exact Mann-Whitney statistic (ties count 1/2), 0.0 when a
real class has no positive or no negative row or a probability is NaN (the reference's ``except ValueError: AUC = 0``).
"""
from __future__ import annotations

import csv
import math
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

CLASS_LABELS = ["No AS", "Early AS", "Significant AS"]  # src/data/as_dataloader.py: class_labels
OPTIONAL_LOG_KEYS = ("interval_idx", "window_start", "window_end", "original_length")  # base.py:203-206
MAX_PROTOTYPES = 4096  # pasn_eval_batch_stats: larger P is PASN_ERR_UNSUPPORTED
# csrc/eval_common.h: the limits selective.py, bootstrap.py and calibration.py share (a rank by counting; 4-bit class fields)
MAX_ROWS, MAX_K, MAX_REPLICATES = 1 << 20, 16, 65536


def _require_cuda(*ts) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("protoasnet_amd metrics run on the GPU only; there is no CPU fallback")


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def _batch_stats(logits, sim, target, K_real, P_cls, level, row_offset=0, capacity=0, probs=None, labels=None, logits_out=None,
                 sparsity=None, div_counts=None, sim_sums=None, k_cls=5, k_abs=2) -> None:
    N = sim.shape[0] if sim is not None else logits.shape[0]
    K = logits.shape[1] if logits is not None else max(K_real, 1)
    P = sim.shape[1] if sim is not None else 1
    _lib.check(_lib.lib().pasn_eval_batch_stats(
        _lib.ptr(logits), _lib.ptr(sim), _lib.ptr(target), N, K, K_real, P, P_cls, k_cls, k_abs, float(level), int(row_offset),
        int(capacity), _lib.ptr(probs), _lib.ptr(labels), _lib.ptr(logits_out), _lib.ptr(sparsity), _lib.ptr(div_counts),
        _lib.ptr(sim_sums), _lib.current_stream()))


class SparsityMetric:
    """``src/utils/metrics.py:8-44`` on the device: per row, the index of the first prefix of the descending-sorted normalised
    similarities that reaches ``level``; ``percentage_expl`` / ``total`` are device int64 counters, ``__call__`` /
    ``update_and_compute`` return the batch value as a 0-d device tensor (no host synchronisation)."""

    def __init__(self, dist_sync_on_step: bool = False, level: float = 0.9, device="cuda"):
        self.level = level
        self.device = torch.device(device)
        self._state = torch.zeros(2, dtype=torch.int64, device=self.device)

    @property
    def percentage_expl(self) -> torch.Tensor:
        return self._state[0]

    @property
    def total(self) -> torch.Tensor:
        return self._state[1]

    def reset(self) -> None:
        self._state.zero_()

    def update(self, prototype_activations: torch.Tensor) -> None:
        _require_cuda(prototype_activations, self._state)
        if prototype_activations.dim() != 2:
            raise ValueError("prototype_activations must be (N, P)")
        if prototype_activations.shape[0] == 0:
            return
        _batch_stats(None, _f32(prototype_activations), None, 1, 0, self.level, sparsity=self._state)

    def update_and_compute(self, prototype_activations: torch.Tensor) -> torch.Tensor:
        before = self._state.clone()
        self.update(prototype_activations)
        d = self._state - before
        return d[0].float() / d[1]

    __call__ = update_and_compute

    def compute(self) -> torch.Tensor:
        return self._state[0].float() / self._state[1]


def real_prototype_count(model, num_real_classes: int) -> int:
    """``P_cls``: the prototypes of the real classes, which must come first (the reference's literal ``[:30]`` / ``[30:]`` split holds
    on all of its configs).  Derived from ``prototype_class_identity``."""
    ident = model.prototype_class_identity.detach().cpu()
    cls = ident.argmax(dim=1)
    real = cls < num_real_classes
    P_cls = int(real.sum())
    if not bool(real[:P_cls].all()):
        raise ValueError("the prototypes of the real classes must precede the abstention prototypes")
    return P_cls


def roc_auc_ovr_weighted(probs: torch.Tensor, labels: torch.Tensor, num_classes: int, per_class: bool = False):
    """Weighted one-vs-rest ROC AUC of ``probs`` (M, num_classes) against ``labels`` (M,) -- sklearn's ``roc_auc_score(labels, probs,
    average="weighted", multi_class="ovr", labels=range(num_classes))``, 0.0 where the reference's ``except ValueError`` gives 0.  Labels
    < 0 are padding rows and are ignored.  Returns a 0-d fp64 device tensor (and the (num_classes,) per-class AUCs, NaN where undefined,
    with ``per_class=True``); no host synchronisation."""
    _require_cuda(probs, labels)
    if probs.dim() != 2 or probs.shape[1] != num_classes or labels.shape != probs.shape[:1]:
        raise ValueError("probs must be (M, num_classes) and labels (M,)")
    M = probs.shape[0]
    auc = torch.zeros(1, dtype=torch.float64, device=probs.device)
    auc_k = torch.full((num_classes,), float("nan"), dtype=torch.float64, device=probs.device)
    if M > 0:
        ws = _lib.workspace(_lib.lib().pasn_roc_auc_workspace_bytes(M, num_classes), probs.device)
        _lib.check(_lib.lib().pasn_roc_auc_ovr(_lib.ptr(_f32(probs)), _lib.ptr(labels.to(torch.int32).contiguous()), M, num_classes,
                                               _lib.ptr(auc), _lib.ptr(auc_k), _lib.ptr(ws), _lib.current_stream()))
    return (auc[0], auc_k) if per_class else auc[0]


class EpochEvaluator:
    """One epoch's evaluation statistics of ``model`` (XProtoNet / Video_XProtoNet / ProtoPNet surface: ``num_classes``,
    ``prototype_class_identity``, ``prototype_shape``).

    ``update(logits, sim, target)``: one ``pasn_eval_batch_stats`` launch, no host synchronisation.  ``finish(world_size)`` returns
    ``{auc, auc_per_class, sparsity, diversity, diversity_abstain, simscore_sum}``.  The diversity threshold (a prototype counts when it
    is among a clip's top 5 -- top 2 of the abstention prototypes -- in more than ``threshold * clips`` clips) defaults to the reference's
    0.05 for video models (5-D prototype shape, 6-D occurrence map: Video_XProtoNet_e2e.py:274) and 0.3 for image models
    (XProtoNet_Base.py:533).  Epoch buffers hold ``capacity`` rows (``len(loader) * batch`` when the trainer knows it) and double when
    full.  ``keep_logits=True`` also keeps every row's logits for the prediction CSV."""

    def __init__(self, model, level: float = 0.8, diversity_threshold: Optional[float] = None, keep_logits: bool = False,
                 abstain_class: bool = False, capacity: int = 0):
        self.K = int(model.num_classes)
        self.K_real = self.K - 1 if abstain_class else self.K
        self.P = int(model.num_prototypes) if hasattr(model, "num_prototypes") else int(model.prototype_shape[0])
        if self.P > MAX_PROTOTYPES:
            raise NotImplementedError(f"{self.P} prototypes: the evaluation kernel supports at most {MAX_PROTOTYPES}")
        self.P_cls = real_prototype_count(model, self.K_real)
        self.abstain = abstain_class
        self.level = level
        video = len(tuple(model.prototype_shape)) == 5
        self.diversity_threshold = (0.05 if video else 0.3) if diversity_threshold is None else diversity_threshold
        self.keep_logits = keep_logits
        self.device = next(model.parameters()).device
        _require_cuda(torch.empty(0, device=self.device))
        self.reset(capacity)

    def reset(self, capacity: int = 0) -> None:
        dev = self.device
        self.rows = 0
        self.capacity = max(int(capacity), 1)
        self.probs = torch.empty(self.capacity, self.K_real, dtype=torch.float32, device=dev)
        self.labels = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.logits = torch.empty(self.capacity, self.K, dtype=torch.float32, device=dev) if self.keep_logits else None
        self.sparsity = torch.zeros(2, dtype=torch.int64, device=dev)
        self.div_counts = torch.zeros(self.P, dtype=torch.int64, device=dev)
        self.sim_sums = torch.zeros(self.P, dtype=torch.float64, device=dev)

    def _grow(self, need: int) -> None:
        cap = self.capacity
        while cap < need:
            cap *= 2
        for name in ("probs", "labels", "logits"):
            old = getattr(self, name)
            if old is not None:
                new = old.new_empty((cap,) + tuple(old.shape[1:]))
                new[: self.rows] = old[: self.rows]
                setattr(self, name, new)
        self.capacity = cap

    def update(self, logits: torch.Tensor, sim: torch.Tensor, target: torch.Tensor) -> None:
        _require_cuda(logits, sim, target)
        N = logits.shape[0]
        if logits.shape != (N, self.K) or sim.shape != (N, self.P) or target.shape != (N,):
            raise ValueError(f"expected logits (N, {self.K}), sim (N, {self.P}), target (N,); got {tuple(logits.shape)}, "
                             f"{tuple(sim.shape)}, {tuple(target.shape)}")
        if N == 0:
            return
        if self.rows + N > self.capacity:
            self._grow(self.rows + N)
        _batch_stats(_f32(logits), _f32(sim), target.detach().to(torch.int64).contiguous(), self.K_real, self.P_cls, self.level,
                     self.rows, self.capacity, self.probs, self.labels, self.logits, self.sparsity, self.div_counts, self.sim_sums)
        self.rows += N

    # ---- the pieces the data-parallel trainer exchanges -------------------------------------------------------------------------
    def additive_stats(self) -> torch.Tensor:
        """fp64 device vector [sparsity sum, sparsity count, diversity counts (P), similarity sums (P)]: summed over ranks as it is."""
        return torch.cat([self.sparsity.double(), self.div_counts.double(), self.sim_sums])

    def summarize(self, additive: torch.Tensor, auc: torch.Tensor, auc_k: torch.Tensor, clips: int) -> Dict[str, object]:
        """Host dict from the (reduced) additive vector and the AUC tensors: ONE device-to-host copy."""
        host = torch.cat([additive, auc.reshape(1).double(), auc_k.double()]).cpu()
        P = self.P
        sp_sum, sp_cnt = host[0].item(), host[1].item()
        counts = host[2: 2 + P]
        sims = host[2 + P: 2 + 2 * P]
        thr = self.diversity_threshold * clips
        return {
            "auc": float(host[2 + 2 * P]),
            "auc_per_class": host[3 + 2 * P:].tolist(),
            "sparsity": sp_sum / sp_cnt if sp_cnt > 0 else float("nan"),
            "diversity": int((counts[: self.P_cls] > thr).sum()),
            "diversity_abstain": int((counts[self.P_cls:] > thr).sum()) if self.abstain else None,
            "simscore_sum": sims.tolist(),
        }

    def finish(self, world_size: int = 1) -> Dict[str, object]:
        """The epoch's metrics.  ``world_size > 1`` (an initialised process group): counters summed over the ranks, the AUC over every
        rank's rows -- the same result on every rank."""
        return self.finish_with(world_size)[0]

    def finish_with(self, world_size: int = 1, carry: Optional[torch.Tensor] = None):
        """``finish``, plus a caller's own vector ``carry`` summed over the ranks in the SAME all-reduce (``DPTrainer`` sends its confusion
        matrix and loss sums along): returns (metrics, reduced carry as fp64, or None).  Collectives with ``world_size > 1``: one
        all-reduce (carry, additive counters, one row count per rank) and one ``all_gather`` of the padded (probs, label) rows."""
        additive = self.additive_stats()
        probs, labels, clips = self.probs[: self.rows], self.labels[: self.rows], self.rows
        nc = 0 if carry is None else carry.numel()
        if world_size > 1:
            import torch.distributed as dist

            vec = torch.cat([torch.zeros(0, dtype=torch.float64, device=self.device) if carry is None else carry.double().to(self.device),
                             additive, torch.zeros(world_size, dtype=torch.float64, device=self.device)])
            vec[nc + additive.numel() + dist.get_rank()] = float(self.rows)
            vec = _all_reduce(vec)
            carry, additive = vec[:nc] if nc else None, vec[nc: nc + additive.numel()]
            counts = [int(c) for c in vec[nc + additive.numel():].cpu()]
            probs, labels = gather_rows(probs, labels, counts)
            clips = sum(counts)
        elif carry is not None:
            carry = carry.double()
        auc, auc_k = roc_auc_ovr_weighted(probs, labels, self.K_real, per_class=True)
        return self.summarize(additive, auc, auc_k, clips), carry


def _all_reduce(t: torch.Tensor) -> torch.Tensor:
    import torch.distributed as dist

    from .push import _for_collective

    buf = _for_collective(t)
    dist.all_reduce(buf)
    return buf.to(t.device)


def gather_rows(probs: torch.Tensor, labels: torch.Tensor, counts: Sequence[int]):
    """Every rank's (probs, label) rows on every rank: ONE ``all_gather`` of the rows padded to the largest count, padding label -1
    (ignored by the AUC kernel).  ``counts[r]`` is rank r's row count (every rank passes the same list).  Rank-major order."""
    import torch.distributed as dist

    from .push import _for_collective

    K_real = probs.shape[1]
    m = max(max(counts), 1)
    pad = torch.full((m, K_real + 1), -1.0, dtype=torch.float32, device=probs.device)
    pad[: probs.shape[0], :K_real] = probs
    pad[: probs.shape[0], K_real] = labels.float()  # labels are small integers: exact in fp32
    pad = _for_collective(pad)
    bufs = [torch.empty_like(pad) for _ in counts]
    dist.all_gather(bufs, pad)
    allrows = torch.cat(bufs).to(probs.device)
    return allrows[:, :K_real].contiguous(), allrows[:, K_real].to(torch.int32).contiguous()


# ---- prediction CSV (base.py:195-211, Video_XProtoNet_e2e.py:221-233, :313-319) -------------------------------------------------------
def logit_names(num_real_classes: int, abstain_class: bool, class_labels: Optional[Sequence[str]] = None) -> List[str]:
    labels = list(class_labels) if class_labels is not None else (CLASS_LABELS if num_real_classes == 3 else [str(k) for k in range(num_real_classes)])
    if len(labels) != num_real_classes:
        raise ValueError(f"{len(labels)} class labels for {num_real_classes} real classes")
    return labels + ["abstain"] if abstain_class else labels


def batch_log_meta(sample: dict) -> dict:
    """The host-side columns of one batch: filename, target_AS and whichever of interval_idx / window_start / window_end /
    original_length it carries, as Python lists (the loader's tensors are host tensors: no device synchronisation)."""
    def ints(v):
        return torch.as_tensor(v).int().tolist()

    meta = {"filename": list(sample["filename"]), "target_AS": ints(sample["target_AS"])}
    for k in OPTIONAL_LOG_KEYS:
        if k in sample:
            meta[k] = ints(sample[k])
    return meta


def prediction_rows(metas: Iterable[dict], logits: np.ndarray, names: Sequence[str]) -> List[dict]:
    """One dict per clip, columns in the reference's order; ``logits`` holds the clips' rows in the order of ``metas``."""
    rows, r = [], 0
    for meta in metas:
        for i in range(len(meta["filename"])):
            row = {k: v[i] for k, v in meta.items()}
            row.update({f"logit_{n}": logits[r, j] for j, n in enumerate(names)})
            rows.append(row)
            r += 1
    if r != logits.shape[0]:
        raise ValueError(f"{r} clips in the batch columns, {logits.shape[0]} logit rows")
    return rows


def _fmt(v) -> str:
    if isinstance(v, (float, np.floating)):
        f = np.float32(v)
        return "" if math.isnan(f) else str(f)  # pandas writes a float32 column with numpy's shortest float32 repr, NaN as ""
    return str(v)


def write_prediction_log(path: str, rows: Sequence[dict]) -> None:
    """``df.reset_index(drop=True).to_csv(path)`` of the reference's prediction frame, byte for byte: an unnamed index column, then the
    rows' columns in order (every row has the same keys); logits are float32 columns."""
    cols = list(rows[0].keys()) if rows else ["filename", "target_AS"]
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        w.writerow([""] + cols)
        for i, row in enumerate(rows):
            if list(row.keys()) != cols:
                raise ValueError(f"row {i} has columns {list(row.keys())}, expected {cols}")
            w.writerow([str(i)] + [_fmt(row[c]) for c in cols])
