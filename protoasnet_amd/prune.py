"""Prototype pruning: what does the prediction lose when a prototype goes, and which prototypes can go?  (``csrc/prune.hip``)

The other split-level evaluators audit a trained model; this one acts on what they show about the prototypes.  The last layer is linear
without a bias, so the logits of "the model without prototype p" follow from the similarities of ONE forward sweep: an M x P x K problem,
not M forwards.  The reference has a ``prune_prototypes`` for head A only and no criterion; the definitions in
``include/protoasnet_amd.h`` ("Prototype pruning") are the specification, ``tests/prune_cases.py`` their float64 / int64
restatement.

* ``importance(sim, fc_w, labels, K_real, proto_class) -> PruneTable``: per prototype the change in errors (also per true class), the
  predictions that flip and the change of the summed margin when it alone is ablated.
* ``eliminate(..., budget, keep_per_class, min_per_class, max_extra_errors, margin_fraction) -> PruneResult``: greedy backward
  elimination, one round per removal, every round on the device (no read inside the loop); ``read()`` is ONE read.
* ``apply(model, remove)``: the surgery on ``PPNet``, ``XProtoNet`` and ``Video_XProtoNet`` (``model.prune_prototypes``); ``state`` /
  ``restore``: the removed indices relative to the model as built, which is what a checkpoint stores.

The kernels run on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_P, MAX_K, MAX_ROWS = 256, 16, 1 << 24  # PASN_PRUNE_MAX_P, the evaluators' class limit, PASN_PRUNE_MAX_ROWS


def chunk() -> int:
    """The rows of one chunk of the margin sums' fixed order (``pasn_prune_chunk``)."""
    return int(_lib.lib().pasn_prune_chunk())


# ---- the model side: class of a prototype, balance, surgery -----------------------------------------------------------------------------
def proto_classes(model) -> torch.Tensor:
    """(P,) int64 on the host: the class of every prototype (``prototype_class_identity``)."""
    return model.prototype_class_identity.detach().cpu().argmax(dim=1)


def class_counts(model) -> List[int]:
    return torch.bincount(proto_classes(model), minlength=int(model.num_classes)).tolist()


def is_balanced(model) -> bool:
    """Every class owns the same number of prototypes, laid out class-major (a model whose class identity is not a tensor of one row per
    prototype is taken as built)."""
    ident = getattr(model, "prototype_class_identity", None)
    if not isinstance(ident, torch.Tensor) or ident.dim() != 2:
        return True
    cls = proto_classes(model)
    counts = torch.bincount(cls, minlength=int(model.num_classes)).tolist()
    return len(set(counts)) == 1 and bool((cls[1:] >= cls[:-1]).all())


def require_balanced(model, what: str) -> None:
    """Raise the named ``ValueError`` when the classes do not all own the same number of prototypes, laid out class-major: ``what``
    reshapes (N, P) to (N, K, P / K) and would mis-index."""
    if not is_balanced(model):
        counts = class_counts(model)
        raise ValueError(f"unbalanced prototype blocks: the classes own {counts} prototypes, and {what} needs the same number for every "
                         "class, laid out class-major (prune with keep_per_class to keep equal blocks)")


def check_class_blocks(P: int, num_classes: int, what: str) -> None:
    """The same refusal where only the shapes are known (the loss classes)."""
    if P % num_classes:
        raise ValueError(f"unbalanced prototype blocks: {P} prototypes do not split into {num_classes} equal class blocks, which {what} "
                         "needs (prune with keep_per_class to keep equal blocks)")


def track(model, keep: Sequence[int], before: int) -> None:
    """Keep ``model._proto_origin`` -- the index every current prototype had in the model as built -- through a removal that left the
    prototypes ``keep`` of ``before`` (``prune_prototypes`` calls it)."""
    origin = model.__dict__.get("_proto_origin")
    if origin is None:
        origin, model._built_prototypes = list(range(before)), before
    model._proto_origin = [origin[i] for i in keep]


def _check_remove(model, remove) -> List[int]:
    P = int(model.num_prototypes)
    rm = [int(i) for i in (remove.tolist() if isinstance(remove, (torch.Tensor, np.ndarray)) else remove)]
    if any(not 0 <= i < P for i in rm) or len(set(rm)) != len(rm):
        raise ValueError(f"remove must hold distinct prototype indices in [0, {P}), got {rm}")
    if len(rm) >= P:
        raise ValueError("at least one prototype must remain")
    return rm


def slice_occurrence(model, keep: Sequence[int]) -> None:
    """Head B: the occurrence module's last conv has one output channel per prototype."""
    conv = model.occurrence_module.convs()[-1]
    conv.weight = torch.nn.Parameter(conv.weight.data[list(keep)].contiguous(), requires_grad=conv.weight.requires_grad)
    if conv.bias is not None:
        conv.bias = torch.nn.Parameter(conv.bias.data[list(keep)].contiguous(), requires_grad=conv.bias.requires_grad)
    conv.out_channels = len(keep)


def apply(model, remove) -> List[int]:
    """Remove the prototypes ``remove`` (indices into the model as it stands) from a ``PPNet``, ``XProtoNet`` or ``Video_XProtoNet``:
    ``prototype_vectors``, ``ones``, the last layer's columns, ``prototype_class_identity`` and, for head B, the rows of the occurrence
    module's last conv.  The packed-weight, plan and training-runner caches key on the tensors' signatures and rebuild on their own.
    Returns the kept indices.  An optimizer built on the old parameters must be rebuilt (``DPTrainer.prune_prototypes`` does)."""
    from .nets import PPNet

    if not isinstance(model, PPNet):
        raise NotImplementedError(f"prune.apply covers PPNet, XProtoNet and Video_XProtoNet, not {type(model).__name__}")
    rm = _check_remove(model, remove)
    keep = sorted(set(range(int(model.num_prototypes))) - set(rm))
    if rm:
        model.prune_prototypes(rm)
    return keep


def state(model) -> List[int]:
    """The removed prototypes as indices into the model as BUILT, ascending: what a checkpoint stores next to the ``state_dict``."""
    origin = model.__dict__.get("_proto_origin")
    if origin is None:
        return []
    return sorted(set(range(int(model._built_prototypes))) - set(origin))


def restore(model, removed) -> None:
    """Bring a freshly built model to the shape of a pruned one (before ``load_state_dict``)."""
    removed = [int(i) for i in removed]
    if not removed:
        return
    if state(model):
        raise ValueError("prune.restore takes the model as built; this one has been pruned already")
    apply(model, removed)


# ---- the kernels' side ----------------------------------------------------------------------------------------------------------------
def _check_inputs(sim, fc_w, labels, K_real, proto_class):
    for t in (sim, fc_w, labels, proto_class):
        if not isinstance(t, torch.Tensor):
            raise ValueError("sim, fc_w, labels and proto_class must be tensors")
        if not t.is_cuda:
            raise RuntimeError("protoasnet_amd pruning runs on the GPU only; there is no CPU fallback")
    if sim.dim() != 2 or fc_w.dim() != 2 or fc_w.shape[1] != sim.shape[1] or labels.shape != sim.shape[:1] or proto_class.shape != sim.shape[1:]:
        raise ValueError("sim must be (M, P), fc_w (K, P), labels (M,) and proto_class (P,)")
    M, P = sim.shape
    K = fc_w.shape[0]
    if isinstance(K_real, bool) or not isinstance(K_real, (int, np.integer)) or not 2 <= K_real <= K <= MAX_K:
        raise ValueError(f"2 <= K_real <= K <= {MAX_K} is required, got K_real={K_real!r}, K={K}")
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"pruning takes 1 .. {MAX_ROWS} rows, got {M}")
    if not 1 <= P <= MAX_P:
        raise ValueError(f"pruning takes 1 .. {MAX_P} prototypes, got {P}")
    return M, P, K, int(K_real)


def _nonneg_int(v, name, lo=0):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


class PruneTable:
    """Device result of round 0: ``table_i`` (P + 1, 2 + K_real) int64 -- per prototype ``wrong``, ``flips``, ``wrong`` per true class of
    the model without it; row P: the model itself -- and ``table_m`` (P + 1,) fp64, the margin sums."""

    def __init__(self, table_i: torch.Tensor, table_m: torch.Tensor, K_real: int):
        self.table_i, self.table_m, self.K_real = table_i, table_m, K_real
        self.P = table_i.shape[0] - 1

    def packed(self) -> torch.Tensor:
        return torch.cat([self.table_i.double().flatten(), self.table_m])  # counts are below 2^53: exact in fp64

    @staticmethod
    def unpack(host, P: int, K_real: int) -> Dict[str, object]:
        W = 2 + K_real
        h = np.asarray(host, dtype=np.float64)
        ti = h[: (P + 1) * W].reshape(P + 1, W).astype(np.int64)
        tm = h[(P + 1) * W: (P + 1) * W + P + 1]
        return {"wrong_0": int(ti[P, 0]), "wrong_per_class_0": ti[P, 2:].copy(), "margin_sum_0": float(tm[P]),
                "wrong": ti[:P, 0].copy(), "flips": ti[:P, 1].copy(), "wrong_per_class": ti[:P, 2:].copy(), "margin_sum": tm[:P].copy(),
                "d_wrong": ti[:P, 0] - ti[P, 0], "d_wrong_per_class": ti[:P, 2:] - ti[P, 2:], "d_margin": tm[:P] - tm[P]}

    def read(self) -> Dict[str, object]:
        """ONE synchronising copy: ``{wrong_0, wrong_per_class_0, margin_sum_0, wrong, flips, wrong_per_class, margin_sum, d_wrong,
        d_wrong_per_class, d_margin}`` (numpy; the ``d_`` entries are the differences to the model itself)."""
        return self.unpack(self.packed().cpu().numpy(), self.P, self.K_real)


class PruneResult:
    """Device results of ``eliminate``: ``table`` (the round-0 ``PruneTable``), ``removed`` (R,) int32 -- the prototype each round removed,
    -1 from the round that stopped on --, ``trace_i`` (R, 1 + K_real) int64 and ``trace_m`` (R,) fp64 -- ``wrong``, ``wrong`` per class and
    the margin sum of the model AFTER each round --, ``kept`` (P,) int32 and ``z`` (M, K_real) fp64, the logits of the model at the end."""

    def __init__(self, table: PruneTable, removed, trace_i, trace_m, kept, z, rounds: int):
        self.table, self.removed, self.trace_i, self.trace_m, self.kept, self.z, self.rounds = table, removed, trace_i, trace_m, kept, z, rounds

    def read(self) -> Dict[str, object]:
        """ONE synchronising copy: ``{order, removed, kept, kept_mask, stopped, trace: [{removed, wrong, wrong_per_class, margin_sum}],
        table}`` -- ``order`` the removed prototypes in order, ``kept`` the remaining indices, ``table`` as ``PruneTable.read``."""
        P, Kr, R = self.table.P, self.table.K_real, self.rounds
        parts = [self.table.packed(), self.kept.double()]
        if R:
            parts += [self.removed.double(), self.trace_i.double().flatten(), self.trace_m]
        h = torch.cat(parts).cpu().numpy()
        nt = (P + 1) * (2 + Kr) + P + 1
        table = PruneTable.unpack(h[:nt], P, Kr)
        mask = h[nt: nt + P].astype(np.int64)
        o = nt + P
        removed = h[o: o + R].astype(np.int64)
        ti = h[o + R: o + R + R * (1 + Kr)].reshape(R, 1 + Kr).astype(np.int64)
        tm = h[o + R + R * (1 + Kr): o + 2 * R + R * (1 + Kr)]
        trace = [{"removed": int(removed[r]), "wrong": int(ti[r, 0]), "wrong_per_class": ti[r, 1:].tolist(), "margin_sum": float(tm[r])}
                 for r in range(R)]
        return {"order": [int(p) for p in removed if p >= 0], "removed": removed.tolist(), "kept": np.flatnonzero(mask).tolist(),
                "kept_mask": mask, "stopped": bool(R and removed[-1] < 0), "trace": trace, "trace_wrong": ti, "trace_margin": tm, "table": table}


def _run(sim, fc_w, labels, K_real, proto_class, rounds, floors, accept, max_extra, margin_fraction) -> PruneResult:
    M, P, K, Kr = _check_inputs(sim, fc_w, labels, K_real, proto_class)
    dev, lib = sim.device, _lib.lib()
    with torch.cuda.device(dev):
        sim = sim.detach().float().contiguous()
        fc_w = fc_w.detach().float().contiguous()
        labels = labels.to(torch.int32).contiguous()
        proto_class = proto_class.to(torch.int32).contiguous()
        fl = None if floors is None else torch.tensor(floors, dtype=torch.int32).to(dev, non_blocking=True)
        z = torch.empty(M, Kr, dtype=torch.float64, device=dev)
        table_i = torch.empty(P + 1, 2 + Kr, dtype=torch.int64, device=dev)
        table_m = torch.empty(P + 1, dtype=torch.float64, device=dev)
        kept = torch.empty(P, dtype=torch.int32, device=dev)
        removed = torch.empty(rounds, dtype=torch.int32, device=dev) if rounds else None
        trace_i = torch.empty(rounds, 1 + Kr, dtype=torch.int64, device=dev) if rounds else None
        trace_m = torch.empty(rounds, dtype=torch.float64, device=dev) if rounds else None
        ws = _lib.workspace(lib.pasn_prune_workspace_bytes(M, P, Kr), dev)
        _lib.check(lib.pasn_prune_eliminate(_lib.ptr(sim), _lib.ptr(fc_w), _lib.ptr(labels), _lib.ptr(proto_class), _lib.ptr(fl), M, P, K, Kr,
                                            rounds, int(accept), int(max_extra), int(margin_fraction is not None),
                                            0.0 if margin_fraction is None else float(margin_fraction), _lib.ptr(z), _lib.ptr(table_i),
                                            _lib.ptr(table_m), _lib.ptr(removed), _lib.ptr(trace_i), _lib.ptr(trace_m), _lib.ptr(kept),
                                            _lib.ptr(ws), _lib.current_stream()))
    return PruneResult(PruneTable(table_i, table_m, Kr), removed, trace_i, trace_m, kept, z, rounds)


def importance(sim: torch.Tensor, fc_w: torch.Tensor, labels: torch.Tensor, K_real: int, proto_class: torch.Tensor) -> PruneTable:
    """The round-0 table of ``sim`` (M, P) fp32 under the last layer ``fc_w`` (K, P) against ``labels`` (M,) (< 0 or >= K_real: the row
    is skipped): per prototype what the model without it gets wrong (also per true class), how many predictions flip and its margin sum.
    The building launch and the launch that adds the chunk sums; no host synchronisation."""
    return _run(sim, fc_w, labels, K_real, proto_class, 0, None, False, 0, None).table


def plan_rounds(class_of, K_real: int, budget=None, keep_per_class=None, min_per_class: int = 1):
    """``(rounds, floors, accept)`` of an elimination over prototypes of the classes ``class_of`` (host integers)."""
    counts = np.bincount(np.asarray([c for c in class_of if 0 <= c < K_real], dtype=np.int64), minlength=K_real)
    if keep_per_class is not None:
        g = _nonneg_int(keep_per_class, "keep_per_class", 1)
        if budget is not None:
            raise ValueError("keep_per_class fixes the number of rounds; budget can not be given with it")
        if (counts < g).any():
            raise ValueError(f"keep_per_class={g}, but the real classes own {counts.tolist()} prototypes")
        return int((counts - g).sum()), [g] * K_real, False
    m = _nonneg_int(min_per_class, "min_per_class")
    most = int(np.maximum(counts - m, 0).sum())
    rounds = most if budget is None else min(_nonneg_int(budget, "budget"), most)
    return rounds, [m] * K_real, True


def eliminate(sim: torch.Tensor, fc_w: torch.Tensor, labels: torch.Tensor, K_real: int, proto_class: torch.Tensor,
              budget: Optional[int] = None, keep_per_class: Optional[int] = None, min_per_class: int = 1, max_extra_errors: int = 0,
              margin_fraction: Optional[float] = None) -> PruneResult:
    """Greedy backward elimination: every round removes, among the kept prototypes of the real classes that stand above their class's
    floor, the one whose removal leaves the fewest errors (then the largest margin sum, then the lowest index).

    ``keep_per_class=g``: the floors are ``g``, the loop runs exactly ``P_real - K_real * g`` rounds and accepts every one: equal blocks
    per class remain.  Otherwise the floors are ``min_per_class``, at most ``budget`` rounds run, and a removal is accepted only while
    ``wrong <= wrong_0 + max_extra_errors`` and (``margin_fraction`` given) ``margin_sum >= margin_fraction * margin_sum_0``; the first
    refusal stops the loop on the device and the later rounds record -1.  ``proto_class`` is read on the host once, to size the loop."""
    if keep_per_class is not None and (max_extra_errors != 0 or margin_fraction is not None):
        raise ValueError("keep_per_class runs with the acceptance test off; max_extra_errors and margin_fraction can not be given with it")
    _check_inputs(sim, fc_w, labels, K_real, proto_class)
    max_extra = _nonneg_int(max_extra_errors, "max_extra_errors")
    if margin_fraction is not None and (isinstance(margin_fraction, bool) or not np.isfinite(float(margin_fraction))):
        raise ValueError(f"margin_fraction must be a finite number or None, got {margin_fraction!r}")
    rounds, floors, accept = plan_rounds(proto_class.tolist(), int(K_real), budget, keep_per_class, min_per_class)
    return _run(sim, fc_w, labels, K_real, proto_class, rounds, floors, accept, max_extra, margin_fraction if accept else None)
