"""Black-box saliency: RISE (Petsiuk, Das, Saenko, BMVC 2018) on the device (``csrc/rise.hip``), the baseline ``faithfulness.py``
compares the occurrence maps with.

Beating a random map is a low bar.  RISE never looks inside the model: it runs it on many randomly masked copies of the clip and averages
the masks, weighted by the score (the similarity to a prototype, or the probability of a class).  If the model's own occurrence maps are
not more faithful than that, they explain little.

The masks are never stored.  A mask is a function of ``(seed, clip id, mask index)`` through Philox -- a coarse lattice of 0 / 1 points,
shifted and interpolated trilinearly -- and is regenerated wherever it is needed; the sums run with the mask index ascending in fp64.  A
map is therefore reproducible bit for bit and does not depend on which batch its clip arrived in.  The reference has no code for this:
the definitions in ``include/protoasnet_amd.h`` ("Black-box saliency") are the specification,
``tests/saliency_cases.py`` their numpy restatement.

* ``keep_threshold(p)``: the uint32 a lattice word is compared with.
* ``masked_clips(x, grid, p, seed, clip0, m0, Mc, baseline, fill)``: the masked copies for a chunk of masks (``pasn_rise_apply``).
* ``mask_scores(...)`` / ``saliency_maps(...)``: ``pasn_rise_scores`` / ``pasn_rise_maps`` on the caller's tensors.
* ``rise(model, x, ...)`` (also ``model.rise(x, ...)``): one ``explain_batch``, the model's forward on chunks of masked clips, one scores
  call, one maps call; device tensors, nothing is read back.

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .explain import _check_model, _clip_geometry, _dimensions, _int_select, explain_batch

TARGETS = ("prototype", "class")   # target 0, target 1 of pasn_rise_scores
NORMS = ("coverage", "expected")   # norm 0, norm 1 of pasn_rise_maps
GRID_VIDEO, GRID_IMAGE = (4, 7, 7), (1, 7, 7)
MAX_MASKS, MAX_MAPS, MAX_LATTICE, MAX_CHANNELS = 65535, 65535, 8192, 64


def keep_threshold(p: float) -> int:
    """``min(2^32 - 1, floor(p 2^32))`` for a keep probability ``0 < p < 1``: a lattice point is 1 iff its Philox word is below it."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"p must lie in (0, 1), got {p!r}")
    keep = min(2 ** 32 - 1, int(math.floor(p * 4294967296.0)))  # (a power-of-two scale: the product is exact)
    if keep < 1:
        raise ValueError(f"p = {p!r} keeps nothing (floor(p 2^32) = 0)")
    return keep


def _int_in(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def check_grid(grid: Optional[Sequence[int]], shape: Tuple[int, int, int], video: bool) -> Tuple[int, int, int]:
    """The coarse grid ``(gt, gh, gw)`` of a clip of ``shape = (T, H, W)`` (images: a pair is read as ``(1, gh, gw)``), within the
    kernels' limits.  ``None``: ``(4, 7, 7)`` for video, ``(1, 7, 7)`` for images."""
    if grid is None:
        grid = GRID_VIDEO if video else GRID_IMAGE
    g = tuple(grid)
    if len(g) == 2 and not video:
        g = (1,) + g
    if len(g) != 3:
        raise ValueError(f"grid must be (gt, gh, gw), got {grid!r}")
    gt, gh, gw = _int_in(g[0], 1, 16, "gt"), _int_in(g[1], 1, 32, "gh"), _int_in(g[2], 1, 32, "gw")
    if (gt + 2) * (gh + 2) * (gw + 2) > MAX_LATTICE:
        raise ValueError(f"grid {g} has {(gt + 2) * (gh + 2) * (gw + 2)} lattice points, more than {MAX_LATTICE}")
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f"a clip of {shape} has 2^31 voxels or more")
    return gt, gh, gw


def _seed_clip(seed, clip0, N: int) -> Tuple[int, int]:
    seed, clip0 = _int_in(seed, 0, 2 ** 64 - 1, "seed"), _int_in(clip0, 0, 2 ** 32 - 1, "clip0")
    if clip0 + N > 2 ** 32:
        raise ValueError(f"clip ids {clip0} .. {clip0 + N - 1} leave 32 bits")
    return seed, clip0


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"protoasnet_amd models run on the GPU only; there is no CPU fallback ({what} is on {t.device})")


def masked_clips(x: torch.Tensor, grid, p: float, seed: int, clip0: int, m0: int, Mc: int, baseline: Optional[torch.Tensor] = None,
                 fill: float = 0.0) -> torch.Tensor:
    """The copies of the clips ``x`` (N, C, [T,] H, W) fp32 / bf16 under the masks ``m0 .. m0 + Mc - 1``: (N, Mc, C, [T,] H, W),
    ``b + (x - b) * mask`` in fp32, rounded to the dtype once.  Clip ``n`` is clip ``clip0 + n`` of the caller's numbering: its masks are
    the same in any batch.  ``baseline``: a tensor like ``x`` or None for the scalar ``fill``.  One launch."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"the clip must be fp32 or bf16, got {x.dtype}")
    video, shape = _clip_geometry(x)
    gt, gh, gw = check_grid(grid, shape, video)
    keep = keep_threshold(p)
    N, C = int(x.shape[0]), int(x.shape[1])
    _int_in(N, 1, 65535, "clips per call")
    _int_in(C, 1, MAX_CHANNELS, "channels")
    seed, clip0 = _seed_clip(seed, clip0, N)
    m0, Mc = _int_in(m0, 0, MAX_MASKS - 1, "m0"), _int_in(Mc, 1, MAX_MASKS, "Mc")
    if m0 + Mc > MAX_MASKS:
        raise ValueError(f"masks {m0} .. {m0 + Mc - 1} exceed {MAX_MASKS}")
    if baseline is not None and (baseline.shape != x.shape or baseline.dtype != x.dtype or baseline.device != x.device):
        raise ValueError("baseline must have the shape, dtype and device of x")
    _require_cuda(x, "x")
    x = x.contiguous()
    baseline = None if baseline is None else baseline.contiguous()
    out = torch.empty((N, Mc) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().pasn_rise_apply(x.data_ptr(), _lib.ptr(baseline), float(fill), N, C, shape[0], shape[1], shape[2], gt, gh, gw, keep,
                                          seed, clip0, m0, Mc, _lib.dtype_code(x.dtype), out.data_ptr(), _lib.current_stream()))
    return out


def _code(value, names, what: str) -> int:
    if value not in names:
        raise ValueError(f"{what} must be one of {names}, got {value!r}")
    return names.index(value)


def mask_scores(sim: Optional[torch.Tensor], logits: Optional[torch.Tensor], sel: Optional[torch.Tensor], cls: Optional[torch.Tensor],
                target: str = "prototype", K_real: Optional[int] = None) -> torch.Tensor:
    """The scores (N, M, k) fp32 of the masked copies.  "prototype": ``sim`` (N, M, P) read at ``sel`` (N, k) int32, a copy; "class":
    the softmax of ``logits`` (N, M, K) over the first ``K_real`` classes read at ``cls`` (N,) int32, k = 1.  An index out of range
    gives NaN.  One launch."""
    code = _code(target, TARGETS, "target")
    src, idx = (sim, sel) if code == 0 else (logits, cls)
    if src is None or idx is None or src.dim() != 3 or src.dtype != torch.float32 or idx.dtype != torch.int32:
        raise ValueError(f"target {target!r} needs fp32 (N, M, .) {'sim' if code == 0 else 'logits'} and int32 {'sel' if code == 0 else 'cls'}")
    N, M, width = (int(v) for v in src.shape)
    k = int(idx.shape[1]) if code == 0 else 1
    if idx.shape != ((N, k) if code == 0 else (N,)):
        raise ValueError(f"the index tensor {tuple(idx.shape)} does not belong to {N} clips")
    _int_in(M, 1, MAX_MASKS, "masks")
    _int_in(N * k, 1, MAX_MAPS, "maps per call")
    P, K = (width, 0) if code == 0 else (0, width)
    K_real = 0 if code == 0 else _int_in(K if K_real is None else K_real, 1, min(K, 16), "K_real")
    _require_cuda(src, "the model's output")
    _require_cuda(idx, "the index tensor")
    src, idx = src.contiguous(), idx.contiguous()
    scores = torch.empty((N, M, k), dtype=torch.float32, device=src.device)
    a = (src.data_ptr(), 0, idx.data_ptr(), 0) if code == 0 else (0, src.data_ptr(), 0, idx.data_ptr())
    _lib.check(_lib.lib().pasn_rise_scores(*a, N, M, k, P, K, K_real, code, scores.data_ptr(), _lib.current_stream()))
    return scores


def stage_masks(grid: Sequence[int]) -> int:
    """The masks a block of the maps kernel stages in LDS at once for this grid (``pasn_rise_stage_masks``)."""
    return int(_lib.lib().pasn_rise_stage_masks(int(grid[0]), int(grid[1]), int(grid[2])))


def saliency_maps(scores: torch.Tensor, shape: Sequence[int], grid, p: float, seed: int = 0, clip0: int = 0, norm: str = "coverage",
                  maps: bool = True, saliency: bool = True, cov: bool = False):
    """``scores`` (N, M, k) fp32 on the GPU, ``shape`` the clip's ``([T,] H, W)``: ``(saliency, maps, cov)`` -- (N, k, [T,] H, W) fp32,
    the same as uint8 by ``pasn_explain_maps``' rule, the coverage (N, [T,] H, W) fp64; None where not asked.  ``norm``: "coverage"
    (S / Cov, 0 where Cov == 0) or "expected" (S / (M keep / 2^32))."""
    code = _code(norm, NORMS, "norm")
    if scores.dim() != 3 or scores.dtype != torch.float32:
        raise ValueError(f"scores must be fp32 (N, M, k), got {scores.dtype} {tuple(scores.shape)}")
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError(f"shape must be ([T,] H, W), got {shape!r}")
    video = len(shape) == 3
    thw = shape if video else (1,) + shape
    gt, gh, gw = check_grid(grid, thw, video)
    keep = keep_threshold(p)
    N, M, k = (int(v) for v in scores.shape)
    _int_in(M, 1, MAX_MASKS, "masks")
    _int_in(N * k, 1, MAX_MAPS, "maps per call")
    seed, clip0 = _seed_clip(seed, clip0, N)
    if not (maps or saliency or cov):
        raise ValueError("nothing to compute: maps, saliency and cov are all off")
    _require_cuda(scores, "scores")
    dev = scores.device
    scores = scores.contiguous()
    lib = _lib.lib()
    sal = torch.empty((N, k) + shape, dtype=torch.float32, device=dev) if saliency else None
    u8 = torch.empty((N, k) + shape, dtype=torch.uint8, device=dev) if maps else None
    cv = torch.empty((N,) + shape, dtype=torch.float64, device=dev) if cov else None
    ws = _lib.workspace(lib.pasn_rise_maps_workspace_bytes(N, k, M, thw[0], thw[1], thw[2], gt, gh, gw), dev)
    _lib.check(lib.pasn_rise_maps(scores.data_ptr(), N, k, M, thw[0], thw[1], thw[2], gt, gh, gw, keep, seed, clip0, code, _lib.ptr(sal),
                                  _lib.ptr(u8), _lib.ptr(cv), ws.data_ptr(), _lib.current_stream()))
    return sal, u8, cv


@dataclass
class Rise:
    """Device tensors of one batch.  k maps per clip, M masks."""

    maps: Optional[torch.Tensor]  # (N, k, [T,] H, W) uint8, on the scale of explain_batch(maps="uint8"); None with maps=None
    saliency: torch.Tensor        # (N, k, [T,] H, W) fp32
    scores: torch.Tensor          # (N, M, k) fp32: the score of every masked copy
    selected: torch.Tensor        # (N, k) int32: the prototypes the maps belong to (explain_batch's)
    pred: torch.Tensor            # (N,) int32: the class predicted for the untouched clip


def rise(model, x: torch.Tensor, select: int = 1, masks: int = 2048, grid=None, p: float = 0.5, target: str = "prototype",
         norm: str = "coverage", maps: Optional[str] = "uint8", seed: int = 0, clip0: int = 0, max_batch: int = 64,
         baseline: Optional[torch.Tensor] = None, fill: float = 0.0, abstain_class: bool = True) -> Rise:
    """RISE saliency of the clips ``x`` (the model's input, on the GPU) without looking inside the model: ``masks`` masked copies per
    clip go through ``model.forward``, and the masks are averaged, weighted by the score.  ``target``: "prototype" -- the similarity to
    each of the ``select`` best prototypes of the predicted class, one map each -- or "class" -- the probability of the predicted class,
    one map (``select`` must be 1).  ``grid``: the coarse lattice, None = (4, 7, 7) for video and (1, 7, 7) for images; ``p``: the
    probability that a lattice point keeps the clip.  ``norm``: "coverage" or "expected" (``saliency_maps``).  ``maps``: "uint8" or
    None (the fp32 ``saliency`` always comes).  Clip ``n`` is clip ``clip0 + n``: a sweep that passes the clips seen so far gets the
    maps one big batch would give.  The masked copies go through the model ``max_batch`` at a time at most, every forward with the
    same batch size (the last chunk repeats its last mask), so that one plan is compiled."""
    _check_model(model, x, "saliency")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"the clip must be fp32 or bf16, got {x.dtype}")
    k = _int_select(select, "maps per clip")
    code = _code(target, TARGETS, "target")
    _code(norm, NORMS, "norm")
    if maps not in ("uint8", None):
        raise ValueError(f"maps must be 'uint8' or None, got {maps!r}")
    if code == 1 and k != 1:
        raise ValueError(f"target 'class' gives one map per clip: select must be 1, got {k}")
    M = _int_in(masks, 1, MAX_MASKS, "masks")
    max_batch = _int_in(max_batch, 1, 2 ** 31 - 1, "max_batch")
    video, shape = _clip_geometry(x)
    grid = check_grid(grid, shape, video)
    keep_threshold(p)
    N = int(x.shape[0])
    _int_in(N * k, 1, MAX_MAPS, "maps per call")
    seed, clip0 = _seed_clip(seed, clip0, N)
    K_real = _dimensions(model, abstain_class)[3]
    P, K = int(model.num_prototypes), int(model.num_classes)
    x = x.contiguous()
    dev = x.device
    with torch.no_grad():
        ex = explain_batch(model, x, select=k, maps=None, abstain_class=abstain_class)
        selected, pred = ex.selected.contiguous(), ex.pred.contiguous()
        sim_all = torch.empty((N, M, P), dtype=torch.float32, device=dev)
        logits_all = torch.empty((N, M, K), dtype=torch.float32, device=dev)
        chunk = min(M, max_batch)                         # masks per forward: FIXED, the last chunk repeats its last mask
        n_clips = max(1, min(N, max_batch // chunk))      # clips per forward (more than one only when all M masks fit)
        for n0 in range(0, N, n_clips):
            n1 = min(N, n0 + n_clips)
            bs = None if baseline is None else baseline[n0:n1]
            for m0 in range(0, M, chunk):
                live = min(chunk, M - m0)
                clips = masked_clips(x[n0:n1], grid, p, seed, clip0 + n0, m0, live, bs, fill)
                if live < chunk:
                    clips = torch.cat([clips, clips[:, -1:].expand((-1, chunk - live) + tuple(clips.shape[2:]))], 1)
                logits, sim, _ = model(clips.reshape((-1,) + tuple(clips.shape[2:])))
                sim_all[n0:n1, m0:m0 + live] = sim.float().reshape(n1 - n0, chunk, P)[:, :live]
                logits_all[n0:n1, m0:m0 + live] = logits.float().reshape(n1 - n0, chunk, K)[:, :live]
        scores = mask_scores(sim_all, logits_all, selected, pred, target, K_real)
        sal, u8, _ = saliency_maps(scores, tuple(x.shape[2:]), grid, p, seed, clip0, norm, maps=maps == "uint8")
    return Rise(maps=u8, saliency=sal, scores=scores, selected=selected, pred=pred)
