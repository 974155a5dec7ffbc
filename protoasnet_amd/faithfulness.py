"""Explanation faithfulness: deletion and insertion curves of the head-B models' occurrence maps (``csrc/perturb.hip``).

``explain.py`` says where a prototype looks; this module asks whether the similarity and the class probability rest on those voxels.  The
clip's voxels are ordered by the map (level descending, flat index ascending), and for step ``s`` the first ``counts[s]`` of them are

* **deletion**: replaced by the baseline -- a faithful map makes the score fall early (a SMALL area under the curve);
* **insertion**: the only ones taken from the clip, the rest is baseline -- a faithful map makes the score rise early (a LARGE area).

Both are compared with the same curves under a random map (``saliency="random"``) and, on request, under a RISE map obtained without
looking inside the model (``saliency="rise"``, ``saliency.py``).  The reference has no code for this: the definitions
in ``include/protoasnet_amd.h`` ("Explanation faithfulness") are the specification, ``tests/faithfulness_cases.py`` their
numpy restatement.

* ``step_counts(V, steps)`` / ``step_counts(V, fractions=[...])``: the voxel counts of the steps, Python integers.
* ``removal_steps(maps_u8, counts)``: per voxel the first step that touches it (``pasn_perturb_steps``).
* ``perturb(x, steps, step_ids, mode, baseline, fill)``: the perturbed clips of a chunk of steps (``pasn_perturb_apply``).
* ``perturbation_curves(model, x, ...)`` (also ``model.faithfulness(x, ...)``): one ``explain_batch``, one ``removal_steps``, the model's
  forward on chunks of perturbed clips, one ``pasn_perturb_curves``; device tensors, nothing is read back.
* ``FaithfulnessAccumulator``: the sums of a sweep in fp64 device accumulators, read once (``DPTrainer.evaluate_faithfulness``).

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .explain import _check_model, _clip_geometry, _dimensions, _int_select, explain_batch

MAX_STEPS = 64                      # S1 = steps + 1 entries of counts at most
MODES = ("deletion", "insertion")   # mode 0, mode 1 of pasn_perturb_apply


def step_counts(V: int, steps: int = 10, fractions: Optional[Sequence[float]] = None) -> List[int]:
    """The number of voxels touched at each step.  ``steps``: ``counts[s] = (2 s V + steps) // (2 steps)`` for ``s = 0 .. steps`` (``s V /
    steps`` rounded half up, in integers: 0 first, V last).  ``fractions``: ``floor(f V + 0.5)`` per entry, which must be non-decreasing
    in [0, 1]."""
    V = int(V)
    if V < 1:
        raise ValueError(f"V must be positive, got {V}")
    if fractions is not None:
        fr = [float(f) for f in fractions]
        if not fr or len(fr) > MAX_STEPS or any(not 0.0 <= f <= 1.0 for f in fr) or any(b < a for a, b in zip(fr, fr[1:])):
            raise ValueError(f"fractions must be 1 .. {MAX_STEPS} non-decreasing values in [0, 1]")
        return [min(V, int(np.floor(f * V + 0.5))) for f in fr]
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps < MAX_STEPS:
        raise ValueError(f"steps must be an integer in [1, {MAX_STEPS - 1}], got {steps!r}")
    steps = int(steps)
    return [(2 * s * V + steps) // (2 * steps) for s in range(steps + 1)]


def _mode_code(mode) -> int:
    if mode in (0, 1) and not isinstance(mode, bool):
        return int(mode)
    if mode in MODES:
        return MODES.index(mode)
    raise ValueError(f"mode must be 'deletion' (0) or 'insertion' (1), got {mode!r}")


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"protoasnet_amd models run on the GPU only; there is no CPU fallback ({what} is on {t.device})")


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _counts_tensor(counts, V: int, device) -> torch.Tensor:
    if isinstance(counts, torch.Tensor):
        if counts.dim() != 1 or not 1 <= counts.numel() <= MAX_STEPS:
            raise ValueError(f"counts must hold 1 .. {MAX_STEPS} entries")
        return counts.to(device=device, dtype=torch.int32).contiguous()
    c = [int(v) for v in counts]
    if not 1 <= len(c) <= MAX_STEPS:
        raise ValueError(f"counts must hold 1 .. {MAX_STEPS} entries, got {len(c)}")
    if any(not 0 <= v <= V for v in c) or any(b < a for a, b in zip(c, c[1:])):
        raise ValueError(f"counts must be non-decreasing in [0, {V}]")
    return torch.tensor(c, dtype=torch.int32, device=device)


def removal_steps(maps_u8: torch.Tensor, counts) -> torch.Tensor:
    """``maps_u8`` (N, k, [To,] Ho, Wo) uint8 on the GPU, ``counts`` non-decreasing in [0, V] (a sequence, or an int32 device tensor that
    is then not checked): the uint8 volume ``steps`` of the same shape, ``steps[v]`` = the number of ``s`` with ``counts[s] <= pos(v)``,
    ``pos`` the voxel's position in the map's (level descending, index ascending) order.  Exact; three launches, no synchronisation."""
    if maps_u8.dtype != torch.uint8 or maps_u8.dim() < 3:
        raise TypeError(f"maps must be a uint8 tensor (N, k, [To,] Ho, Wo), got {maps_u8.dtype} {tuple(maps_u8.shape)}")
    _require_cuda(maps_u8, "maps")
    N, k = int(maps_u8.shape[0]), int(maps_u8.shape[1])
    V = int(np.prod(maps_u8.shape[2:]))
    maps_u8 = _aligned(maps_u8)
    dev = maps_u8.device
    cnt = _counts_tensor(counts, V, dev)
    S1 = int(cnt.numel())
    lib = _lib.lib()
    steps = torch.empty_like(maps_u8)
    ws = _lib.workspace(lib.pasn_perturb_steps_workspace_bytes(N * k, V, S1), dev)
    _lib.check(lib.pasn_perturb_steps(maps_u8.data_ptr(), cnt.data_ptr(), N * k, V, S1, steps.data_ptr(), ws.data_ptr(), _lib.current_stream()))
    return steps


def perturb(x: torch.Tensor, steps: torch.Tensor, step_ids, mode, baseline: Optional[torch.Tensor] = None, fill: float = 0.0) -> torch.Tensor:
    """The perturbed copies of the clips ``x`` (N, C, [T,] H, W) fp32 / bf16 at the steps ``step_ids`` (ints, or an int32 device tensor):
    (N, k, Sc, C, [T,] H, W), a bitwise copy of ``x`` or of the baseline per voxel.  ``steps`` (N, k, [T,] H, W) is ``removal_steps``'
    volume.  Deletion: voxels with ``steps <= s`` come from ``baseline`` (same shape and dtype as ``x``; ``None``: the scalar ``fill``);
    insertion: only those come from ``x``.  One launch."""
    code = _mode_code(mode)
    _require_cuda(x, "x")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"the clip must be fp32 or bf16, got {x.dtype}")
    if steps.dtype != torch.uint8 or steps.dim() != x.dim() or steps.shape[0] != x.shape[0] or steps.shape[2:] != x.shape[2:]:
        raise ValueError(f"steps {tuple(steps.shape)} {steps.dtype} does not belong to clips {tuple(x.shape)}")
    if baseline is not None and (baseline.shape != x.shape or baseline.dtype != x.dtype or baseline.device != x.device):
        raise ValueError("baseline must have the shape, dtype and device of x")
    dev = x.device
    ids = step_ids.to(device=dev, dtype=torch.int32).contiguous() if isinstance(step_ids, torch.Tensor) else \
        torch.tensor([int(s) for s in step_ids], dtype=torch.int32, device=dev)
    if ids.dim() != 1 or ids.numel() < 1:
        raise ValueError("step_ids must hold at least one step")
    N, C, k, Sc = int(x.shape[0]), int(x.shape[1]), int(steps.shape[1]), int(ids.numel())
    V = int(np.prod(x.shape[2:]))
    x, steps = x.contiguous(), steps.contiguous()
    baseline = None if baseline is None else baseline.contiguous()
    out = torch.empty((N, k, Sc, C) + tuple(x.shape[2:]), dtype=x.dtype, device=dev)
    _lib.check(_lib.lib().pasn_perturb_apply(x.data_ptr(), steps.data_ptr(), ids.data_ptr(), _lib.ptr(baseline), float(fill), N, C, k, V, Sc,
                                             code, _lib.dtype_code(x.dtype), out.data_ptr(), _lib.current_stream()))
    return out


@dataclass
class Curves:
    """Device tensors of one batch and one mode.  k maps per clip, S1 steps."""

    mode: str
    fractions: torch.Tensor       # (S1,) fp64: counts / V, the curves' abscissa
    similarity: torch.Tensor      # (N, k, S1) fp32: the similarity to prototype selected[n, j] on the perturbed clip
    prob: torch.Tensor            # (N, k, S1) fp32: the probability of class pred[n] (softmax over the non-abstain logits)
    auc_similarity: torch.Tensor  # (N, k) fp64: trapezoid areas over fractions
    auc_prob: torch.Tensor        # (N, k) fp64
    selected: torch.Tensor        # (N, k) int32: the prototypes the maps belong to
    pred: torch.Tensor            # (N,) int32: the class predicted for the untouched clip
    steps: torch.Tensor           # (N, k, [To,] Ho, Wo) uint8: removal_steps of the maps


@dataclass
class CurvePair:
    """``perturbation_curves(mode="both")``."""

    deletion: Curves
    insertion: Curves


def accumulator_size(k: int, S1: int) -> int:
    """fp64 entries of the ``acc`` vector of ``pasn_perturb_curves``: similarity curves (k, S1), probability curves (k, S1), the areas
    (k, 2), the clip count."""
    return 2 * k * S1 + 2 * k + 1


def random_saliency(x: torch.Tensor, k: int, seed: int = 0) -> torch.Tensor:
    """The control: a uniform uint8 map (N, k, [T,] H, W) from a device generator seeded with ``seed``."""
    g = torch.Generator(device=x.device)
    g.manual_seed(int(seed))
    return torch.randint(0, 256, (int(x.shape[0]), int(k)) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device, generator=g)


def _run_mode(model, x, steps_vol, counts_dev, fractions, code: int, selected, pred, baseline, fill, max_batch: int, K_real: int, V: int,
              acc: Optional[torch.Tensor]) -> Curves:
    N, k, S1 = int(x.shape[0]), int(steps_vol.shape[1]), int(counts_dev.numel())
    P, K = int(model.num_prototypes), int(model.num_classes)
    dev = x.device
    sim_all = torch.empty((N, k, S1, P), dtype=torch.float32, device=dev)
    logits_all = torch.empty((N, k, S1, K), dtype=torch.float32, device=dev)
    n_clips = max(1, min(N, max_batch // k))                  # clips per forward
    chunk = max(1, min(S1, max_batch // (n_clips * k)))       # steps per forward: FIXED, the last chunk repeats its last step
    ids_all = torch.arange(-(-S1 // chunk) * chunk, dtype=torch.int32, device=dev).clamp_(max=S1 - 1)
    for n0 in range(0, N, n_clips):
        n1 = min(N, n0 + n_clips)
        xs, ss = x[n0:n1], steps_vol[n0:n1]
        bs = None if baseline is None else baseline[n0:n1]
        for s0 in range(0, S1, chunk):
            live = min(chunk, S1 - s0)
            clips = perturb(xs, ss, ids_all[s0:s0 + chunk], code, bs, fill)
            logits, sim, _ = model(clips.reshape((-1,) + tuple(clips.shape[3:])))
            sim_all[n0:n1, :, s0:s0 + live] = sim.float().reshape(n1 - n0, k, chunk, P)[:, :, :live]
            logits_all[n0:n1, :, s0:s0 + live] = logits.float().reshape(n1 - n0, k, chunk, K)[:, :, :live]
    curve_sim = torch.empty((N, k, S1), dtype=torch.float32, device=dev)
    curve_prob = torch.empty((N, k, S1), dtype=torch.float32, device=dev)
    auc = torch.empty((N, k, 2), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().pasn_perturb_curves(sim_all.data_ptr(), logits_all.data_ptr(), selected.data_ptr(), pred.data_ptr(),
                                              counts_dev.data_ptr(), N, k, S1, P, K, K_real, V, curve_sim.data_ptr(), curve_prob.data_ptr(),
                                              auc.data_ptr(), _lib.ptr(acc), _lib.current_stream()))
    return Curves(mode=MODES[code], fractions=fractions, similarity=curve_sim, prob=curve_prob,
                  auc_similarity=auc[..., 0], auc_prob=auc[..., 1], selected=selected, pred=pred, steps=steps_vol)


def perturbation_curves(model, x: torch.Tensor, select: int = 1, steps: Union[int, Sequence[float]] = 10, mode: str = "both",
                        saliency=None, baseline: Optional[torch.Tensor] = None, fill: float = 0.0, max_batch: int = 64,
                        abstain_class: bool = True, seed: int = 0, _acc: Optional[Dict[str, torch.Tensor]] = None,
                        rise: Optional[Dict[str, object]] = None):
    """Deletion / insertion curves of the clips ``x`` (the model's input, on the GPU) for the ``select`` best prototypes of the predicted
    class.  ``steps``: an int (``step_counts(V, steps)``) or a sequence of fractions.  ``mode``: "deletion", "insertion" (a ``Curves``) or
    "both" (a ``CurvePair``).  ``saliency``: None = the model's own uint8 occurrence maps (``explain_batch(maps="uint8")``), a uint8 tensor
    (N, select, [To,] Ho, Wo) of the caller's, "random" (``random_saliency(x, select, seed)``, the control) or "rise" (the uint8 maps of
    ``saliency.rise(model, x, select=select, abstain_class=abstain_class, **rise)``, the black-box baseline; ``rise`` holds its other
    arguments: masks, grid, p, target, norm, seed, clip0, max_batch, baseline, fill).  ``baseline``: a tensor like
    ``x`` (a blurred clip, say) or None for the scalar ``fill`` (0 = the mean grey of a normalised clip).  The perturbed clips go through
    ``model.forward`` at most ``max_batch`` at a time, every chunk of steps with the same batch size, so that one plan is compiled (a last,
    smaller group of clips compiles a second one).  Step 0 of the default counts is the untouched clip under deletion and the baseline
    under insertion; the last step the reverse."""
    _check_model(model, x, "faithfulness")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"the clip must be fp32 or bf16, got {x.dtype}")
    if mode not in MODES + ("both",):
        raise ValueError(f"mode must be 'deletion', 'insertion' or 'both', got {mode!r}")
    k = _int_select(select, "maps per clip")
    if rise is not None and saliency != "rise":
        raise ValueError("rise holds the arguments of saliency='rise' and goes with nothing else")
    if isinstance(max_batch, bool) or not isinstance(max_batch, (int, np.integer)) or max_batch < 1:
        raise ValueError(f"max_batch must be a positive integer, got {max_batch!r}")
    _, grid = _clip_geometry(x)
    V = grid[0] * grid[1] * grid[2]
    counts = step_counts(V, steps) if isinstance(steps, (int, np.integer)) else step_counts(V, fractions=steps)
    K_real = _dimensions(model, abstain_class)[3]
    x = x.contiguous()
    with torch.no_grad():
        own = saliency is None
        ex = explain_batch(model, x, select=k, maps="uint8" if own else None, abstain_class=abstain_class)
        if own:
            maps = ex.maps
        elif isinstance(saliency, str):
            if saliency == "rise":
                from .saliency import rise as rise_maps

                maps = rise_maps(model, x, **{**dict(rise or {}), "select": k, "maps": "uint8", "abstain_class": abstain_class}).maps
            elif saliency == "random":
                maps = random_saliency(x, k, seed)
            else:
                raise ValueError(f"saliency must be None, 'random', 'rise' or a uint8 tensor, got {saliency!r}")
        else:
            maps = saliency
            if not isinstance(maps, torch.Tensor) or maps.dtype != torch.uint8 or maps.numel() != x.shape[0] * k * V or maps.shape[:2] != (x.shape[0], k):
                raise ValueError(f"saliency must be a uint8 tensor ({x.shape[0]}, {k}, ...) of {V} voxels per map")
            _require_cuda(maps, "saliency")
        maps = maps.reshape((int(x.shape[0]), k) + tuple(x.shape[2:]))
        counts_dev = _counts_tensor(counts, V, x.device)
        steps_vol = removal_steps(maps, counts_dev)
        fractions = torch.tensor([c / V for c in counts], dtype=torch.float64, device=x.device)  # (the kernel's own quotient, IEEE)
        res = {}
        for name in MODES if mode == "both" else (mode,):
            res[name] = _run_mode(model, x, steps_vol, counts_dev, fractions, MODES.index(name), ex.selected.contiguous(), ex.pred, baseline, fill,
                                  int(max_batch), K_real, V, None if _acc is None else _acc[name])
    return CurvePair(**res) if mode == "both" else res[mode]


class FaithfulnessAccumulator:
    """The sums of a sweep: per batch the curves of the model's maps and of the random control (batch ``b`` draws it with ``seed + b``),
    both modes, added on the device onto fp64 accumulators (clips in ascending order); ``result()`` is the ONE synchronising read.
    ``kinds``: which maps are swept, "model" first; "rise" adds the black-box baseline (``saliency.rise`` with the arguments ``rise``,
    ``seed`` unless it names its own, and ``clip0`` = its own plus the clips seen so far: a clip's masks do not depend on the batching)."""

    KINDS = ("model", "random")
    ALL_KINDS = ("model", "random", "rise")

    def __init__(self, model, select: int = 1, steps=10, fill: float = 0.0, max_batch: int = 64, abstain_class: bool = True, seed: int = 0,
                 kinds: Sequence[str] = KINDS, rise: Optional[Dict[str, object]] = None):
        kinds = tuple(kinds)
        if not kinds or kinds[0] != "model" or len(set(kinds)) != len(kinds) or any(kd not in self.ALL_KINDS for kd in kinds):
            raise ValueError(f"kinds must start with 'model' and add any of 'random', 'rise' once, got {kinds!r}")
        if rise is not None and "rise" not in kinds:
            raise ValueError("rise holds the arguments of the 'rise' kind, which is not swept")
        self.kinds, self.rise, self.clips = kinds, dict(rise or {}), 0
        self.model, self.select, self.steps, self.fill, self.max_batch = model, int(select), steps, fill, max_batch
        self.abstain_class, self.seed = abstain_class, int(seed)
        self.S1 = (int(steps) + 1) if isinstance(steps, (int, np.integer)) else len(steps)
        self.batches = 0
        self.acc = None       # (kinds, 2 modes, accumulator_size) fp64, on the first batch's device
        self.fractions = None

    def update(self, x: torch.Tensor) -> None:
        if self.acc is None:
            self.acc = torch.zeros((len(self.kinds), 2, accumulator_size(self.select, self.S1)), dtype=torch.float64, device=x.device)
        for i, kind in enumerate(self.kinds):
            args = None
            if kind == "rise":
                args = {"seed": self.seed, **self.rise, "clip0": int(self.rise.get("clip0", 0)) + self.clips}
            pair = perturbation_curves(self.model, x, select=self.select, steps=self.steps, mode="both",
                                       saliency=None if kind == "model" else kind, fill=self.fill, max_batch=self.max_batch,
                                       abstain_class=self.abstain_class, seed=self.seed + self.batches,
                                       _acc={m: self.acc[i, j] for j, m in enumerate(MODES)}, rise=args)
        self.fractions = pair.deletion.fractions
        self.batches += 1
        self.clips += int(x.shape[0])

    def result(self) -> Dict[str, object]:
        """``{clips, fractions, deletion, insertion, random: {deletion, insertion}, difference: {deletion, insertion}}``: per mode the mean
        curves ``similarity`` / ``prob`` (k, S1) and the mean areas ``auc_similarity`` / ``auc_prob`` (k,), numpy float64; ``difference`` is
        model minus random for the areas (faithful maps: negative under deletion, positive under insertion).  ``random`` and ``difference``
        come with the "random" kind; the "rise" kind adds ``rise`` and ``difference_rise`` (model minus RISE) of the same layout."""
        if self.acc is None:
            raise ValueError("no clips: update() was never called")
        k, S1 = self.select, self.S1
        host = self.acc.cpu().numpy()  # the one read
        fractions = self.fractions.cpu().numpy()

        def unpack(v):
            n = v[-1]
            return {"similarity": v[:k * S1].reshape(k, S1) / n, "prob": v[k * S1:2 * k * S1].reshape(k, S1) / n,
                    "auc_similarity": v[2 * k * S1:-1].reshape(k, 2)[:, 0] / n, "auc_prob": v[2 * k * S1:-1].reshape(k, 2)[:, 1] / n}

        res = {"clips": int(host[0, 0, -1]), "fractions": fractions}
        res.update({m: unpack(host[0, j]) for j, m in enumerate(MODES)})
        for i, kind in enumerate(self.kinds[1:], 1):
            res[kind] = {m: unpack(host[i, j]) for j, m in enumerate(MODES)}
            res["difference" if kind == "random" else f"difference_{kind}"] = \
                {m: {a: res[m][a] - res[kind][m][a] for a in ("auc_similarity", "auc_prob")} for m in MODES}
        return res
