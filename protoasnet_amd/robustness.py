"""Robustness: echo-style clip corruptions and the stability of a prediction and of its explanation under them (``csrc/corrupt.hip``).

``metrics.py`` to ``faithfulness.py`` ask how good the prediction and its maps are on the clips as recorded.  This module asks what
happens to both when the acquisition changes a little: gain and time-gain compensation differ between operators, speckle and electronic
noise between probes, frames get dropped, focus is soft.  A prototype explanation is worth showing only if it survives the perturbations
the class prediction survives.  The reference has no code for this: the definitions in ``include/protoasnet_amd.h`` (INTEGRATION.md,
"Robustness") are the specification, ``tests/robustness_cases.py`` their numpy restatement.

* ``CORRUPTIONS``: name -> (the parameter at severities 1 - 5, the descriptor builder).  The values are part of the definition.
* ``describe(name, severity, shape, seed)``: the ``Corruption`` descriptor of a named corruption for clips of ``shape``.
* ``corrupt(x, name_or_descriptor, severity, seed)``: the corrupted clips (``pasn_clip_corrupt``, one launch).
* ``stability(model, x, x_corrupted, ...)``: both ``push_forward``s and ``pasn_stability_stats``; device tensors, nothing is read back.
* ``RobustnessAccumulator``: the sums of a sweep per (corruption, severity) cell in fp64 device accumulators, read once
  (``DPTrainer.evaluate_robustness``).

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .data import ECHO_MEAN, ECHO_STD
from .explain import _check_model, _dimensions, _int_select, _select_count

MAX_RADIUS = 8   # taps: 2 R + 1 <= 17
MAX_MAP = 4096   # voxels of an occurrence map pasn_stability_stats ranks in LDS
SEVERITIES = (1, 2, 3, 4, 5)


@dataclass
class Corruption:
    """The optional stages of ``pasn_clip_corrupt``; ``None`` / 0 is off.  Host arrays (or device tensors) of the shapes below."""

    src_t: Optional[object] = None   # (N, T) int32: output frame t shows input frame src_t[n, t]
    taps: Optional[object] = None    # (2 R + 1,) fp32: the separable blur
    row_a: Optional[object] = None   # (H,) fp32: v = row_a[h] * v + row_b[h] in the pixel domain
    row_b: Optional[object] = None   # (H,) fp32
    sigma_add: float = 0.0           # v += sigma_add * z
    sigma_mul: float = 0.0           # v += (sigma_mul * z) * v


def gaussian_taps(sigma: float) -> np.ndarray:
    """``R = min(8, ceil(2.5 sigma))``; ``exp(-i^2 / (2 sigma^2))`` for ``i = -R .. R`` in float64, normalised, then rounded to fp32."""
    R = min(MAX_RADIUS, int(math.ceil(2.5 * float(sigma))))
    i = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return (w / w.sum()).astype(np.float32)


def attenuation_rows(alpha: float, H: int) -> np.ndarray:
    """``exp(-alpha h / (H - 1))`` per image row in float64, rounded once to fp32 (one row: no attenuation)."""
    h = np.arange(H, dtype=np.float64)
    return np.exp(-float(alpha) * h / float(max(H - 1, 1))).astype(np.float32)


def frame_hold_table(p: float, N: int, T: int, seed: int) -> np.ndarray:
    """(N, T) int32: every frame ``t > 0`` is dropped with probability ``p`` (``numpy.random.default_rng(seed)``, one draw per (n, t > 0)
    in that order); a dropped frame shows the last kept one.  Frame 0 is never dropped."""
    if T < 2:
        raise ValueError("frame_hold needs a clip with more than one frame (T = 1)")
    drop = np.random.default_rng(int(seed)).random((N, T - 1)) < float(p)
    src = np.zeros((N, T), np.int32)
    for t in range(1, T):
        src[:, t] = np.where(drop[:, t - 1], src[:, t - 1], t)
    return src


def _geometry(shape) -> Tuple[int, int, int, int, int]:
    shape = tuple(int(v) for v in shape)
    if len(shape) == 5:
        return shape
    if len(shape) == 4:
        return shape[0], shape[1], 1, shape[2], shape[3]
    raise ValueError(f"the clip must be (N, C, T, H, W) or (N, C, H, W), got {shape}")


def _rows(H: int, value: float) -> np.ndarray:
    return np.full(H, value, np.float32)


# name -> (the parameter at severities 1 .. 5, builder(parameter, (N, C, T, H, W), seed) -> Corruption)
CORRUPTIONS = {
    "gain_down": ((.8, .65, .5, .35, .2), lambda a, g, seed: Corruption(row_a=_rows(g[3], a))),
    "gain_up": ((1.25, 1.5, 1.75, 2., 2.5), lambda a, g, seed: Corruption(row_a=_rows(g[3], a))),
    "contrast": ((.8, .65, .5, .35, .2), lambda c, g, seed: Corruption(row_a=_rows(g[3], c), row_b=_rows(g[3], .5 * (1. - c)))),
    "attenuation": ((.5, 1., 1.5, 2., 3.), lambda al, g, seed: Corruption(row_a=attenuation_rows(al, g[3]))),
    "noise": ((.02, .04, .08, .12, .16), lambda s, g, seed: Corruption(sigma_add=s)),
    "speckle": ((.1, .2, .3, .45, .6), lambda s, g, seed: Corruption(sigma_mul=s)),
    "blur": ((.5, .75, 1., 1.5, 2.), lambda s, g, seed: Corruption(taps=gaussian_taps(s))),
    "frame_hold": ((.1, .2, .3, .4, .5), lambda p, g, seed: Corruption(src_t=frame_hold_table(p, g[0], g[2], seed))),
}


def describe(name: str, severity: int, shape, seed: int = 0) -> Corruption:
    """The descriptor of the named corruption at ``severity`` (1 - 5) for clips of ``shape`` (N, C, [T,] H, W)."""
    if name not in CORRUPTIONS:
        raise ValueError(f"unknown corruption {name!r}; known: {', '.join(CORRUPTIONS)}")
    if isinstance(severity, bool) or not isinstance(severity, (int, np.integer)) or severity not in SEVERITIES:
        raise ValueError(f"severity must be an integer in [1, 5], got {severity!r}")
    values, build = CORRUPTIONS[name]
    return build(values[int(severity) - 1], _geometry(shape), int(seed))


def _table(v, dtype, shape, what: str, device) -> Optional[torch.Tensor]:
    if v is None:
        return None
    t = torch.as_tensor(v).to(device=device, dtype=dtype).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t


def corrupt(x: torch.Tensor, corruption: Union[str, Corruption], severity: Optional[int] = None, seed: int = 0, mean: float = ECHO_MEAN,
            std: float = ECHO_STD) -> torch.Tensor:
    """The corrupted copy of the normalised clips ``x`` (N, C, [T,] H, W), C = 1 or 3, fp32 / bf16 on the GPU: the same shape and dtype.
    ``corruption``: a name of ``CORRUPTIONS`` with its ``severity``, or a ``Corruption`` of the caller's.  ``seed``: the noise stream
    (and the generator of ``frame_hold``'s table).  One launch on the current stream; bit for bit the definition of
    ``pasn_clip_corrupt``."""
    if not x.is_cuda:
        raise RuntimeError(f"protoasnet_amd models run on the GPU only; there is no CPU fallback (x is on {x.device})")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"the clip must be fp32 or bf16, got {x.dtype}")
    N, C, T, H, W = _geometry(x.shape)
    if C not in (1, 3):
        raise ValueError(f"the clip must have 1 or 3 channels, got {C}")
    d = describe(corruption, severity, x.shape, seed) if isinstance(corruption, str) else corruption
    if not isinstance(d, Corruption):
        raise TypeError(f"corruption must be a name or a Corruption, got {type(corruption).__name__}")
    dev = x.device
    taps = None if d.taps is None else torch.as_tensor(d.taps).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    R = 0 if taps is None else (int(taps.numel()) - 1) // 2
    if taps is not None and (taps.numel() % 2 == 0 or R > MAX_RADIUS):
        raise ValueError(f"taps must hold 2 R + 1 entries, 0 <= R <= {MAX_RADIUS}, got {taps.numel()}")
    src_t = _table(d.src_t, torch.int32, (N, T), "src_t", dev)
    row_a = _table(d.row_a, torch.float32, (H,), "row_a", dev)
    row_b = _table(d.row_b, torch.float32, (H,), "row_b", dev)
    desc = _lib.CorruptDesc(src_t=_lib.ptr(src_t) or None, taps=(_lib.ptr(taps) if R else 0) or None, row_a=_lib.ptr(row_a) or None,
                            row_b=_lib.ptr(row_b) or None, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, R=R, sigma_add=float(d.sigma_add),
                            sigma_mul=float(d.sigma_mul), mean=float(mean), stdv=float(std))
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().pasn_clip_corrupt(x.data_ptr(), y.data_ptr(), N, C, T, H, W, _lib.dtype_code(x.dtype), ctypes.byref(desc),
                                            _lib.current_stream()))
    return y


@dataclass
class Stability:
    """Device tensors of one batch: the clean forward (a) against the corrupted one (b).  k selected prototypes per clip."""

    flip: torch.Tensor        # (N,) fp64: 1 where the predicted class changed
    tv: torch.Tensor          # (N,) fp64: total variation between the two softmax vectors over the real classes
    prob_drop: torch.Tensor   # (N,) fp64: p_a[pred_a] - p_b[pred_a]
    overlap: torch.Tensor     # (N,) fp64: |top-k prototypes clean and corrupted| / k, inside the clean prediction's class block
    correct: Optional[torch.Tensor]  # (N, 2) int32 (clean, corrupted) when labels were given
    selected: torch.Tensor    # (N, k) int32: the clean clip's top-k prototypes of its predicted class
    dsim: torch.Tensor        # (N, k) fp64: similarity corrupted - clean
    corr: torch.Tensor        # (N, k) fp64: Pearson correlation of the two occurrence maps
    iou: torch.Tensor         # (N, k) fp64: intersection over union of their top-m voxel sets
    shift: torch.Tensor       # (N, k) fp64: distance between their argmax voxels over the grid's diagonal
    m: int                    # voxels in a top set


def accumulator_size(k: int) -> int:
    """fp64 entries of the ``acc`` vector of ``pasn_stability_stats``: 4 clip statistics, 2 correct counts, (k, 4) pair statistics, N."""
    return 6 + 4 * k + 1


def _forward(model, x: torch.Tensor):
    """(logits (N, K), sim (N, P), occ (N, P, S), (Ti, Hi, Wi)) of ``push_forward``, fp32 and contiguous."""
    with torch.no_grad():
        _, dist, occ, logits = model.push_forward(x)
        N, P = int(occ.shape[0]), int(occ.shape[1])
        grid = tuple(int(v) for v in occ.shape[3:])
        grid = grid if len(grid) == 3 else (1,) + grid
        return logits.float().contiguous(), (1 - dist).float().contiguous(), occ.float().reshape(N, P, -1).contiguous(), grid


def top_count(top_fraction: float, S: int) -> int:
    """``m = max(1, ceil(top_fraction S))`` voxels (at most S)."""
    if not 0.0 < float(top_fraction) <= 1.0:
        raise ValueError(f"top_fraction must lie in (0, 1], got {top_fraction}")
    return min(S, max(1, int(math.ceil(float(top_fraction) * S))))


def stability(model, x: torch.Tensor, x_corrupted: torch.Tensor, select: int = 1, top_fraction: float = 0.1, labels=None,
              abstain_class: bool = True, _clean=None, _acc: Optional[torch.Tensor] = None) -> Stability:
    """Compare the model on the clips ``x`` and on ``x_corrupted`` (the same clips, corrupted): two ``push_forward``s and one
    ``pasn_stability_stats``.  ``select``: the k best prototypes of the clean prediction's class; ``top_fraction``: the share of an
    occurrence map's voxels in its top set; ``labels`` (N,) for the two correctness columns."""
    _check_model(model, x, "robustness")
    if x_corrupted.shape != x.shape or x_corrupted.device != x.device:
        raise ValueError(f"the corrupted clips {tuple(x_corrupted.shape)} do not belong to the clips {tuple(x.shape)}")
    k = _int_select(select, "prototypes per clip")
    P, K, G, K_real = _dimensions(model, abstain_class)
    _select_count(select, G, P)  # k lies in [1, G]
    la, sa, oa, grid = _clean if _clean is not None else _forward(model, x)
    lb, sb, ob, grid_b = _forward(model, x_corrupted)
    S = grid[0] * grid[1] * grid[2]
    m = top_count(top_fraction, S)
    N, dev = int(x.shape[0]), x.device
    lab = None if labels is None else torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    if lab is not None and tuple(lab.shape) != (N,):
        raise ValueError(f"labels must have shape ({N},), got {tuple(lab.shape)}")
    clip = torch.empty((N, 4), dtype=torch.float64, device=dev)
    correct = torch.empty((N, 2), dtype=torch.int32, device=dev) if lab is not None else None
    sel = torch.empty((N, k), dtype=torch.int32, device=dev)
    pair = torch.empty((N, k, 4), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().pasn_stability_stats(la.data_ptr(), lb.data_ptr(), sa.data_ptr(), sb.data_ptr(), oa.data_ptr(), ob.data_ptr(),
                                               _lib.ptr(lab), N, K, K_real, P, grid[0], grid[1], grid[2], k, m, clip.data_ptr(),
                                               _lib.ptr(correct), sel.data_ptr(), pair.data_ptr(), _lib.ptr(_acc), _lib.current_stream()))
    return Stability(flip=clip[:, 0], tv=clip[:, 1], prob_drop=clip[:, 2], overlap=clip[:, 3], correct=correct, selected=sel,
                     dsim=pair[..., 0], corr=pair[..., 1], iou=pair[..., 2], shift=pair[..., 3], m=m)


def robustness(model, x: torch.Tensor, corruption: Union[str, Corruption], severity: Optional[int] = None, seed: int = 0, select: int = 1,
               top_fraction: float = 0.1, labels=None, abstain_class: bool = True, mean: float = ECHO_MEAN,
               std: float = ECHO_STD) -> Stability:
    """``stability`` of the clips ``x`` against ``corrupt(x, corruption, severity, seed)`` (also ``model.robustness(x, ...)``)."""
    _check_model(model, x, "robustness")
    return stability(model, x, corrupt(x, corruption, severity, seed, mean, std), select=select, top_fraction=top_fraction, labels=labels,
                     abstain_class=abstain_class)


class RobustnessAccumulator:
    """The sums of a sweep per (corruption, severity) cell: per batch one clean ``push_forward`` and one corrupted one per cell (batch
    ``b`` corrupts with ``seed + b``), added on the device onto fp64 accumulators (clips in ascending order); ``result()`` is the ONE
    synchronising read."""

    def __init__(self, model, corruptions: Optional[Sequence[str]] = None, severities: Sequence[int] = (1, 3, 5), select: int = 1,
                 top_fraction: float = 0.1, seed: int = 0, abstain_class: bool = True, mean: float = ECHO_MEAN, std: float = ECHO_STD):
        self.model, self.select, self.top_fraction, self.seed = model, int(select), float(top_fraction), int(seed)
        self.abstain_class, self.mean, self.std = abstain_class, mean, std
        self.corruptions = tuple(CORRUPTIONS) if corruptions is None else tuple(corruptions)
        self.severities = tuple(int(s) for s in severities)
        for name in self.corruptions:
            for s in self.severities:
                describe(name, s, (1, 1, 2, 2, 2))  # unknown names and severities fail here, not in the middle of a sweep
        if not self.corruptions or not self.severities:
            raise ValueError("at least one corruption and one severity")
        self.batches = 0
        self.labelled = True  # every batch so far came with labels
        self.acc = None       # (corruptions, severities, accumulator_size) fp64, on the first batch's device

    def update(self, x: torch.Tensor, labels=None) -> None:
        _check_model(self.model, x, "robustness")
        if self.acc is None:
            self.acc = torch.zeros((len(self.corruptions), len(self.severities), accumulator_size(self.select)), dtype=torch.float64,
                                   device=x.device)
        self.labelled = self.labelled and labels is not None
        clean = _forward(self.model, x)
        for i, name in enumerate(self.corruptions):
            for j, sev in enumerate(self.severities):
                xc = corrupt(x, name, sev, self.seed + self.batches, self.mean, self.std)
                stability(self.model, x, xc, select=self.select, top_fraction=self.top_fraction, labels=labels,
                          abstain_class=self.abstain_class, _clean=clean, _acc=self.acc[i, j])
        self.batches += 1

    def result(self) -> Dict[str, object]:
        """``{clips, cells}``; ``cells[name][severity]`` holds the means over the clips: ``acc_clean`` / ``acc_corrupted`` (NaN unless
        every batch came with labels), ``flip_rate``, ``tv``, ``prob_drop``, ``overlap``, and per rank j of the selected prototypes
        ``dsim``, ``corr``, ``iou``, ``shift`` (k,), numpy float64."""
        if self.acc is None:
            raise ValueError("no clips: update() was never called")
        host = self.acc.cpu().numpy()  # the one read
        k = self.select
        cells: Dict[str, Dict[int, Dict[str, object]]] = {}
        for i, name in enumerate(self.corruptions):
            for j, sev in enumerate(self.severities):
                v = host[i, j]
                n = v[-1]
                pair = v[6:6 + 4 * k].reshape(k, 4) / n
                nan = float("nan")
                cells.setdefault(name, {})[sev] = {
                    "acc_clean": float(v[4] / n) if self.labelled else nan, "acc_corrupted": float(v[5] / n) if self.labelled else nan,
                    "flip_rate": float(v[0] / n), "tv": float(v[1] / n), "prob_drop": float(v[2] / n), "overlap": float(v[3] / n),
                    "dsim": pair[:, 0].copy(), "corr": pair[:, 1].copy(), "iou": pair[:, 2].copy(), "shift": pair[:, 3].copy()}
        return {"clips": int(host[0, 0, -1]), "cells": cells}
