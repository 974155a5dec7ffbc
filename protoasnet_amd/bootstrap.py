"""Bootstrap confidence intervals for the evaluation metrics, on the device (``csrc/bootstrap.hip``).

Every number ``metrics.py`` and ``selective.py`` report for a split is a point estimate; this module puts an interval around it.  The
clips of one cine are strongly correlated, so the resampling unit is a GROUP of rows -- the cine, or the patient, whatever key the
caller grouped by (``selective.build_groups``) --, not the row.  The reference has no code for this: the definitions in
``include/protoasnet_amd.h`` ("Bootstrap confidence intervals") are the specification, ``tests/bootstrap_cases.py`` their
float64 / int64 restatement.

* ``draw_counts(G, B, seed)``: the resamples alone -- ``(B, G)`` int32, how often each of the G units was drawn in each replicate
  (Philox4x32-10, counter ``(d >> 2, b, 0, 0)``, unit ``(r * G) >> 32``).  A replicate depends on ``(seed, b, G)`` only.
* ``replicates(probs, labels, u, groups, B, seed)``: accuracy, balanced accuracy, mean F1, weighted one-vs-rest AUC and -- with an
  uncertainty ``u`` -- the risk-coverage area and the error-detection AUROC of every replicate and (last row) of the sample itself, with
  the integers they come from.  Device tensors, no host synchronisation, a fixed number of launches whatever ``B`` is.
* ``intervals(rep, confidence)``: percentile interval, standard error and the number of finite replicates per statistic: host work on
  the ``(B + 1, 6)`` array after ONE synchronising read.

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .metrics import MAX_K, MAX_REPLICATES, MAX_ROWS, _f32, _require_cuda
from .selective import check_groups

STAT_NAMES = ("acc", "bal_acc", "f1_mean", "auc", "aurc", "error_auroc")  # the columns of ``stats``


def lds_max_groups() -> int:
    """The largest G whose counts a block keeps in LDS (``PASN_BOOTSTRAP_LDS_MAX_G``); above it they live in global memory."""
    return int(_lib.lib().pasn_bootstrap_lds_max_groups())


def _check_B_seed(B, seed, min_B: int = 1) -> None:
    """``min_B=0``: ``calibration.reliability``, where no replicates is a call of its own."""
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not min_B <= B <= MAX_REPLICATES:
        raise ValueError(f"B must be an integer in [{min_B}, {MAX_REPLICATES}], got {B!r}")
    if not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")


def draw_counts(G: int, B: int, seed: int = 0, device="cuda", b0: int = 0) -> torch.Tensor:
    """``(B, G)`` int32: ``counts[b][g]`` = how often unit ``g`` was drawn in replicate ``b0 + b``; every row sums to ``G``."""
    _check_B_seed(B, seed)
    if not isinstance(G, (int, np.integer)) or not 1 <= G <= MAX_ROWS:
        raise ValueError(f"G must be an integer in [1, {MAX_ROWS}], got {G!r}")
    if not isinstance(b0, (int, np.integer)) or not 0 <= b0 <= (1 << 31) - 1 - B:
        raise ValueError(f"b0 must not be negative and b0 + B must fit an int32, got {b0!r}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("protoasnet_amd metrics run on the GPU only; there is no CPU fallback")
    with torch.cuda.device(device):
        counts = torch.empty(int(B), int(G), dtype=torch.int32, device=device)
        _lib.check(_lib.lib().pasn_bootstrap_counts(_lib.ptr(counts), int(G), int(B), int(seed), int(b0), _lib.current_stream()))
    return counts


class Replicates:
    """Device results of ``replicates``; row ``b < B`` is replicate ``b``, row ``B`` the point estimate: ``stats`` (B + 1, 6) fp64 in the
    order of ``STAT_NAMES``, ``cm`` (B + 1, K, K), ``u2`` / ``n_pos`` / ``n_neg`` (B + 1, K) int64.  ``point`` is ``stats[B]``."""

    def __init__(self, stats, cm, u2, n_pos, n_neg, B, G, seed):
        self.stats, self.cm, self.u2, self.n_pos, self.n_neg = stats, cm, u2, n_pos, n_neg
        self.B, self.G, self.seed = B, G, seed

    @property
    def point(self) -> torch.Tensor:
        return self.stats[self.B]


def replicates(probs: torch.Tensor, labels: torch.Tensor, u: Optional[torch.Tensor] = None, groups=None, B: int = 1000,
               seed: int = 0) -> Replicates:
    """``B`` grouped bootstrap replicates of the metrics of ``probs`` (M, K_real) fp32, ``labels`` (M,) (< 0 or >= K_real: a padding
    row, never drawn) and, optionally, the uncertainty ``u`` (M,) fp32.  ``groups`` is ``selective.build_groups``' tuple (or its first
    two arrays): the resampling units; ``None``: every row is its own unit.  No host synchronisation."""
    _require_cuda(probs, labels, u)
    _check_B_seed(B, seed)
    if probs.dim() != 2 or labels.shape != probs.shape[:1] or (u is not None and u.shape != probs.shape[:1]):
        raise ValueError("probs must be (M, K_real), labels and u (M,)")
    M, K = probs.shape
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"replicates takes 1 .. {MAX_ROWS} rows, got {M}")
    if not 2 <= K <= MAX_K:
        raise ValueError(f"replicates takes 2 .. {MAX_K} classes, got {K}")
    dev = probs.device
    d_off = d_rows = None
    G = M
    if groups is not None:
        offsets, rows, G = check_groups(groups, M, exclusive=True)
        d_off, d_rows = torch.from_numpy(offsets).to(dev), torch.from_numpy(rows).to(dev)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        probs, labels = _f32(probs), labels.to(torch.int32).contiguous()
        u = None if u is None else _f32(u)
        stats = torch.empty(B + 1, 6, dtype=torch.float64, device=dev)
        cm = torch.empty(B + 1, K, K, dtype=torch.int64, device=dev)
        u2, n_pos, n_neg = (torch.empty(B + 1, K, dtype=torch.int64, device=dev) for _ in range(3))
        ws = _lib.workspace(lib.pasn_bootstrap_workspace_bytes(M, G, K, B), dev)
        _lib.check(lib.pasn_bootstrap_metrics(_lib.ptr(probs), _lib.ptr(labels), _lib.ptr(u), _lib.ptr(d_off), _lib.ptr(d_rows), M, G, K, int(B),
                                              int(seed), _lib.ptr(stats), _lib.ptr(cm), _lib.ptr(u2), _lib.ptr(n_pos), _lib.ptr(n_neg),
                                              _lib.ptr(ws), _lib.current_stream()))
    return Replicates(stats, cm, u2, n_pos, n_neg, int(B), G, int(seed))


def check_confidence(confidence) -> float:
    c = float(confidence)
    if not 0.0 < c < 1.0:
        raise ValueError(f"confidence must lie in (0, 1), got {confidence!r}")
    return c


def intervals_of(stats, confidence: float = 0.95, names=STAT_NAMES) -> Dict[str, Dict[str, float]]:
    """``intervals`` on a host array / tensor ``(B + 1, 6)`` (row B the point estimate): no device work.  ``names``: the columns' names
    (``calibration.STAT_NAMES`` for the calibration statistics: the same arithmetic)."""
    c = check_confidence(confidence)
    s = np.asarray(stats, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] < 2 or s.shape[1] != len(names):
        raise ValueError(f"stats must be (B + 1, {len(names)})")
    out = {}
    nan = float("nan")
    for j, name in enumerate(names):
        v = s[:-1, j]
        v = v[np.isfinite(v)]
        lo, hi, se = nan, nan, nan
        if v.size >= 2:  # fewer finite replicates carry no interval
            lo, hi = (float(x) for x in np.quantile(v, [(1.0 - c) / 2.0, (1.0 + c) / 2.0]))  # numpy's default: linear interpolation
            se = float(np.std(v, ddof=1))
        out[name] = {"point": float(s[-1, j]), "lo": lo, "hi": hi, "se": se, "n_finite": int(v.size)}
    return out


def intervals(rep: Replicates, confidence: float = 0.95) -> Dict[str, Dict[str, float]]:
    """``{name: {"point", "lo", "hi", "se", "n_finite"}}`` for the six statistics: ``lo`` / ``hi`` the ``(1 - c) / 2`` and ``(1 + c) / 2``
    quantiles (linear interpolation) and ``se`` the ``ddof=1`` standard deviation of the FINITE replicate values, ``n_finite`` their
    number (a replicate that lost a class has no AUC); fewer than two give NaN bounds.  ONE synchronising read."""
    check_confidence(confidence)
    return intervals_of(rep.stats.cpu().numpy(), confidence)
