"""Calibration: are the model's numbers probabilities?  (``csrc/calibration.hip``)

Every other evaluation statistic of the project judges the RANKING of the outputs; this module asks whether "0.9" means that about 90 %
of such calls are right, and repairs it with one scalar fitted on a split.  The reference has no code for this: the definitions in
``include/protoasnet_amd.h`` ("Calibration") are the specification, ``tests/calibration_cases.py`` their float64 / int64
restatement.

* ``reliability(probs, labels, n_bins, conf, groups, B, seed)``: the reliability bins (``n``, ``hit``, ``qsum`` per bin; ``cn``, ``cpos``,
  ``cq`` per class and bin) and ``ece``, ``mce``, ``cw_ece``, ``brier``, ``nll``, ``conf_gap`` of the sample (last row) and of ``B``
  grouped-bootstrap replicates -- the resamples of ``bootstrap.draw_counts``, so the same ones ``bootstrap.replicates`` scores for the
  same seed and units.  ``conf`` overrides the top-label confidence: ``1 - u`` asks whether an uncertainty is an honest probability of
  error.  Device tensors, no host synchronisation.
* ``fit_temperature(logits, labels, num_real_classes)``: ``beta = 1 / T`` minimising the NLL of ``softmax(beta z)``, a fixed number of
  launches; ``scaled_probs(logits, num_real_classes, temperature)`` applies it.  ``T`` is ONE number: it is not refitted inside a
  bootstrap replicate.
* ``intervals(rel, confidence)``: ``bootstrap.intervals_of`` on the six statistics after ONE synchronising read.

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Union

import numpy as np
import torch

from . import _lib, bootstrap
from .metrics import MAX_K, MAX_REPLICATES, MAX_ROWS, _f32, _require_cuda
from .selective import check_groups

STAT_NAMES = ("ece", "mce", "cw_ece", "brier", "nll", "conf_gap")  # the columns of ``stats``
STATUS_NAMES = ("ok", "lower_bound", "upper_bound", "empty")  # fit[3]
MAX_BINS = 64
BETA_MIN, BETA_MAX = 1.0 / 64.0, 64.0
CHUNK_BYTES = 64 << 20  # of bootstrap counts drawn at a time


def _check_K(K) -> int:
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 2 <= K <= MAX_K:
        raise ValueError(f"num_real_classes must be an integer in [2, {MAX_K}], got {K!r}")
    return int(K)


def _check_logits(logits: torch.Tensor, K_real: int) -> None:
    if logits.dim() != 2 or not K_real <= logits.shape[1] <= MAX_K + 1:
        raise ValueError(f"logits must be (M, K) with {K_real} <= K <= {MAX_K + 1}")
    if not 1 <= logits.shape[0] <= MAX_ROWS:
        raise ValueError(f"1 .. {MAX_ROWS} rows, got {logits.shape[0]}")


# ---- temperature scaling ---------------------------------------------------------------------------------------------------------------
class TemperatureFit:
    """Device result of ``fit_temperature``: ``info`` (4,) fp64 = {beta, NLL at T = 1, NLL at the fitted T, status}; ``beta`` its first
    element as a (1,) view (what ``scaled_probs`` reads, without a host round trip)."""

    def __init__(self, info: torch.Tensor):
        self.info = info
        self.beta = info[:1]

    def read(self) -> Dict[str, object]:
        """ONE synchronisation: ``{temperature, beta, nll_before, nll_after, status}``, ``status`` one of ``STATUS_NAMES``."""
        beta, before, after, status = self.info.cpu().tolist()
        return {"temperature": 1.0 / beta, "beta": beta, "nll_before": before, "nll_after": after, "status": STATUS_NAMES[int(status)]}


def fit_temperature(logits: torch.Tensor, labels: torch.Tensor, num_real_classes: int) -> TemperatureFit:
    """The temperature of ``logits`` (M, K) fp32 -- the first ``num_real_classes`` columns are scored -- against ``labels`` (M,) (< 0 or
    >= num_real_classes: a padding row).  No host synchronisation."""
    K_real = _check_K(num_real_classes)
    _require_cuda(logits, labels)
    _check_logits(logits, K_real)
    if labels.shape != logits.shape[:1]:
        raise ValueError("labels must be (M,)")
    M, K = logits.shape
    lib = _lib.lib()
    with torch.cuda.device(logits.device):
        info = torch.empty(4, dtype=torch.float64, device=logits.device)
        ws = _lib.workspace(lib.pasn_temperature_workspace_bytes(M, K_real), logits.device)
        _lib.check(lib.pasn_temperature_fit(_lib.ptr(_f32(logits)), _lib.ptr(labels.to(torch.int32).contiguous()), M, K, K_real, _lib.ptr(info),
                                            _lib.ptr(ws), _lib.current_stream()))
    return TemperatureFit(info)


def _check_temperature(temperature) -> None:
    if isinstance(temperature, TemperatureFit):
        return
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)):
        raise ValueError(f"temperature must be a TemperatureFit or a number > 0, got {temperature!r}")
    if not (float(temperature) > 0.0 and np.isfinite(float(temperature))):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")


def scaled_probs(logits: torch.Tensor, num_real_classes: int, temperature: Union[TemperatureFit, float], with_u: bool = False):
    """``softmax(logits[:, :num_real_classes] / T)`` (M, num_real_classes) fp32, computed in fp64 and rounded once; ``with_u=True``
    returns ``(probs, u)`` with ``u`` bitwise ``1.0f - `` the row's largest probability.  No host synchronisation."""
    K_real = _check_K(num_real_classes)
    _check_temperature(temperature)
    _require_cuda(logits)
    _check_logits(logits, K_real)
    M, K = logits.shape
    with torch.cuda.device(logits.device):
        beta = temperature.beta if isinstance(temperature, TemperatureFit) else torch.tensor([1.0 / float(temperature)], dtype=torch.float64,
                                                                                             device=logits.device)
        probs = torch.empty(M, K_real, dtype=torch.float32, device=logits.device)
        u = torch.empty(M, dtype=torch.float32, device=logits.device) if with_u else None
        _lib.check(_lib.lib().pasn_temperature_probs(_lib.ptr(_f32(logits)), M, K, K_real, _lib.ptr(beta), _lib.ptr(probs), _lib.ptr(u),
                                                     _lib.current_stream()))
    return (probs, u) if with_u else probs


# ---- reliability -----------------------------------------------------------------------------------------------------------------------
def check_bins(n_bins) -> int:
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins must be an integer in [1, {MAX_BINS}], got {n_bins!r}")
    return int(n_bins)


class Reliability:
    """Device results of ``reliability``; row ``b < B`` is replicate ``b``, row ``B`` the point estimate: ``n`` / ``hit`` / ``qsum``
    (B + 1, n_bins), ``cn`` / ``cpos`` / ``cq`` (B + 1, K, n_bins), ``skipped`` (B + 1,) -- int64; ``qsum`` and ``cq`` hold the uint64 sums
    of ``q = c * 2^32`` (below 2^63, so the bits are the same) --, ``stats`` (B + 1, 6) fp64 in the order of ``STAT_NAMES``."""

    def __init__(self, stats, n, hit, qsum, cn, cpos, cq, skipped, B, G, n_bins, seed):
        self.stats, self.n, self.hit, self.qsum, self.cn, self.cpos, self.cq, self.skipped = stats, n, hit, qsum, cn, cpos, cq, skipped
        self.B, self.G, self.n_bins, self.seed = B, G, n_bins, seed

    @property
    def point(self) -> torch.Tensor:
        return self.stats[self.B]

    def packed(self) -> torch.Tensor:
        """fp64 device vector [the six statistics, skipped, n, hit, conf (n_bins each)] of the point estimate: what ``summary`` reads."""
        B = self.B
        return torch.cat([self.stats[B], self.skipped[B: B + 1].double(), self.n[B].double(), self.hit[B].double(),
                          self.qsum[B].double() * 2.0 ** -32])

    @staticmethod
    def unpack(host: torch.Tensor, n_bins: int) -> Dict[str, object]:
        v = host.tolist()
        res = dict(zip(STAT_NAMES, v[:6]))
        res["skipped"] = int(v[6])
        n, hit, conf = (v[7 + j * n_bins: 7 + (j + 1) * n_bins] for j in range(3))
        nan = float("nan")
        res["bins"] = [{"lo": j / n_bins, "hi": (j + 1) / n_bins, "n": int(n[j]), "accuracy": hit[j] / n[j] if n[j] else nan,
                        "confidence": conf[j] / n[j] if n[j] else nan} for j in range(n_bins)]
        return res

    def summary(self) -> Dict[str, object]:
        """ONE read: the six statistics, ``skipped`` and ``bins``: one ``{lo, hi, n, accuracy, confidence}`` per bin (NaN where empty)."""
        return self.unpack(self.packed().cpu(), self.n_bins)


def _row_units(groups, M: int):
    """``(row_unit int32 (M,), G)`` of ``selective.build_groups``' tuple, with ``bootstrap.replicates``' checks."""
    offsets, rows, G = check_groups(groups, M, exclusive=True)
    unit = np.full(M, -1, dtype=np.int32)
    unit[rows] = np.repeat(np.arange(G, dtype=np.int32), np.diff(offsets))
    return unit, G


def reliability(probs: torch.Tensor, labels: torch.Tensor, n_bins: int = 15, conf: Optional[torch.Tensor] = None, groups=None, B: int = 0,
                seed: int = 0) -> Reliability:
    """Reliability bins and calibration statistics of ``probs`` (M, K_real) fp32 against ``labels`` (M,) (< 0 or >= K_real: a padding
    row), with ``B >= 0`` grouped-bootstrap replicates.  ``conf`` (M,) fp32 replaces the largest probability as the top-label
    confidence.  ``groups`` is ``selective.build_groups``' tuple (or its first two arrays): the resampling units; ``None``: every row is
    its own unit.  The replicates are drawn in chunks of at most ``CHUNK_BYTES`` of counts; the result does not depend on the chunking.
    No host synchronisation."""
    n_bins = check_bins(n_bins)
    bootstrap._check_B_seed(B, seed, min_B=0)
    _require_cuda(probs, labels, conf)
    if probs.dim() != 2 or labels.shape != probs.shape[:1] or (conf is not None and conf.shape != probs.shape[:1]):
        raise ValueError("probs must be (M, K_real), labels and conf (M,)")
    M, K = probs.shape
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"reliability takes 1 .. {MAX_ROWS} rows, got {M}")
    if not 2 <= K <= MAX_K:
        raise ValueError(f"reliability takes 2 .. {MAX_K} classes, got {K}")
    B, dev, G, d_unit = int(B), probs.device, M, None
    if groups is not None:
        unit, G = _row_units(groups, M)
        d_unit = torch.from_numpy(unit).to(dev)
    lib = _lib.lib()
    with torch.cuda.device(dev):
        probs, labels = _f32(probs), labels.to(torch.int32).contiguous()
        conf = None if conf is None else _f32(conf)
        stats = torch.empty(B + 1, 6, dtype=torch.float64, device=dev)
        n, hit, qsum = (torch.empty(B + 1, n_bins, dtype=torch.int64, device=dev) for _ in range(3))
        cn, cpos, cq = (torch.empty(B + 1, K, n_bins, dtype=torch.int64, device=dev) for _ in range(3))
        skipped = torch.empty(B + 1, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.pasn_calibration_workspace_bytes(M, G, K, n_bins, B), dev)
        outs = (n, hit, qsum, cn, cpos, cq, skipped, stats)
        step = max(1, min(B, CHUNK_BYTES // (4 * G))) if B else 1
        # a chunk writes its replicates at rows b0 .. and the point estimate behind them, where the next chunk's first replicate lands
        for b0 in range(0, max(B, 1), step):
            Bc = min(step, B - b0)
            counts = bootstrap.draw_counts(G, Bc, seed, dev, b0=b0) if Bc else None
            _lib.check(lib.pasn_calibration_bins(_lib.ptr(probs), _lib.ptr(labels), _lib.ptr(conf), _lib.ptr(d_unit), _lib.ptr(counts), M, G, K,
                                                 n_bins, Bc, *(_lib.ptr(t[b0:]) for t in outs), _lib.ptr(ws), _lib.current_stream()))
    return Reliability(stats, n, hit, qsum, cn, cpos, cq, skipped, B, G, n_bins, int(seed))


def intervals(rel: Reliability, confidence: float = 0.95) -> Dict[str, Dict[str, float]]:
    """``bootstrap.intervals`` for the six calibration statistics of ``rel`` (``B >= 1``).  ONE synchronising read."""
    bootstrap.check_confidence(confidence)
    return bootstrap.intervals_of(rel.stats.cpu().numpy(), confidence, names=STAT_NAMES)
