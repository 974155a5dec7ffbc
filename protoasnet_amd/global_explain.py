"""Global explanations of the head-B models (``XProtoNet``, ``Video_XProtoNet``): per prototype, the k nearest clips of a split.

The reference's ``explain.py --explain_globally`` ends in a stub (``XProtoNet_Base.explain_global`` calls nothing); the only global piece
it ships is ``get_sim_scores`` / ``load_sim_scores`` (``src/agents/XProtoNet_Base.py:613-667``), which save the whole (clips, P)
similarity matrix and the targets "for ranking prototypes".  This module answers the question those files are for without pulling
every batch to the host: which clips of a split lie nearest to each prototype, are they of its class, what do their occurrence maps
look like, and how well does each prototype separate its class.

* ``nearest_clips(dataloader, model, k)``: one sweep in the manner of the push (``push.push_prototypes``).  Per batch one
  ``push_forward``, then ``pasn_topk_xproto_update`` (the running k winners per prototype, on the device), ``pasn_topk_gather`` once per
  payload kind (occurrence maps, logits, labels follow the winners into a slot store) and ``pasn_proto_class_stats`` (fp64 per-class
  similarity sums).  No host synchronisation inside the sweep.
* ``merge_topk(states)``: the pure merge of several shards' rows (also on CPU tensors), used for ``world_size > 1``.
* ``nearest_maps(result, ...)``: normalised, upsampled maps and overlays of the winners through ``pasn_explain_maps``.

Order of a row: ascending (distance, global clip index): equal distances keep the LOWER index first, however the split was batched or
sharded.  (The push keeps the later clip on a tie, push_abs_revision.py:299; the rules differ by design -- INTEGRATION.md.)
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import push as push_mod
from .data import ECHO_MEAN, ECHO_STD
from .sweep import WinnerStore, filenames_at, gather_ranks, sweep_batches

K_MAX = 64      # one row entry per lane of a wave
_I64_MAX = torch.iinfo(torch.int64).max
_SIGNED = (torch.int8, torch.int16, torch.int32, torch.int64)  # payloads whose empty entries read -1 (0 for every other dtype)


@dataclass
class GlobalExplanation:
    """P prototypes, k winners each, K classes.  Rows are in rank order (nearest first); entries past the eligible clips hold
    ``dist = +inf``, ``index = -1``, ``labels = -1`` and zero payloads."""

    dist: torch.Tensor                   # (P, k) fp32, ascending
    similarity: torch.Tensor             # (P, k): 1 - dist (-inf where empty)
    index: torch.Tensor                  # (P, k) int64 global clip index in loader order
    labels: torch.Tensor                 # (P, k) int64
    logits: torch.Tensor                 # (P, k, K)
    occurrence_maps: torch.Tensor        # (P, k, 1, [T,] H, W)
    filenames: List[List[Optional[str]]]
    class_mean_similarity: torch.Tensor  # (P, K) fp64: mean similarity to the clips of each ground-truth class (0 for a class without clips)
    class_count: torch.Tensor            # (K,) int64 clips per ground-truth class
    purity: torch.Tensor                 # (P,) fp64
    margin: torch.Tensor                 # (P,) fp64
    ranking: torch.Tensor                # (P,) int64: prototypes by descending margin, the lower index first on ties
    prototype_class: torch.Tensor        # (P,) int64
    sim_scores: Optional[torch.Tensor] = None  # (N_total, P) fp32, with keep_sim_scores
    targets: Optional[torch.Tensor] = None     # (N_total,) int64

    FIELDS = ("dist", "similarity", "index", "labels", "logits", "occurrence_maps", "filenames", "class_mean_similarity", "class_count",
              "purity", "margin", "ranking", "prototype_class")

    def to_numpy(self) -> dict:
        """The fields as numpy arrays (``filenames`` as an object array) -- what ``DPTrainer.explain_global`` pickles."""
        out = {}
        for name in self.FIELDS:
            v = getattr(self, name)
            out[name] = np.array(v, dtype=object) if name == "filenames" else v.detach().cpu().numpy()
        return out


# ------------------------------------------------------------------------------------------------- device state
class TopKState:
    """The caller's side of ``pasn_topk_xproto_update`` / ``pasn_topk_gather``: rows, slot ids and one slot store per payload kind."""

    def __init__(self, P: int, k: int, device):
        if not 1 <= int(k) <= K_MAX:
            raise ValueError(f"k={k} must lie in [1, {K_MAX}] (one row entry per lane; there is no slow path)")
        self.P, self.k, self.device = int(P), int(k), device
        self.dist = torch.full((P, k), float("inf"), dtype=torch.float32, device=device)
        self.index = torch.full((P, k), -1, dtype=torch.int64, device=device)
        self.slot = torch.arange(k, dtype=torch.int32, device=device).repeat(P, 1).contiguous()
        self.store = WinnerStore(P, k, device)

    @property
    def stores(self) -> dict:
        return self.store.stores

    def update(self, proto_dist, labels, proto_class, class_mask, index_base: int) -> None:
        B, P = (int(v) for v in proto_dist.shape)
        _lib.check(_lib.lib().pasn_topk_xproto_update(
            proto_dist.data_ptr(), labels.data_ptr(), proto_class.data_ptr(), class_mask.data_ptr(), self.dist.data_ptr(),
            self.index.data_ptr(), self.slot.data_ptr(), B, P, self.k, int(index_base), _lib.current_stream()))

    def gather(self, name: str, payload: torch.Tensor, per_proto: bool, index_base: int, fill=0) -> None:
        """``payload`` (B, P, ...) with ``per_proto`` else (B, ...): its rows follow this batch's winners into ``stores[name]``."""
        self.store.gather(name, payload, per_proto, self.index, self.slot, index_base, fill)

    def resolved(self, name: str) -> torch.Tensor:
        """``stores[name]`` in row order (slot indirection resolved); empty entries keep the store's fill value."""
        return self.store.resolved(name, self.index, self.slot)


# ------------------------------------------------------------------------------------------------- pure host-side pieces
def merge_topk(states: Sequence[Sequence[torch.Tensor]]):
    """Merge shards' rows under the (distance, index) order.  ``states``: per shard ``(dist (P, k_s), index (P, k_s), *payloads
    (P, k_s, ...))`` in row order; returns the same tuple with k = the first shard's k.  Entries with ``index < 0`` are empty and sort
    last; a union smaller than k leaves the tail at (+inf, -1) with zero payloads (-1 for integer payloads).  Works on CPU tensors."""
    k = int(states[0][0].shape[1])
    cat = [torch.cat([s[i] for s in states], dim=1) for i in range(len(states[0]))]
    dist, index = cat[0], cat[1]
    P, n = dist.shape
    if n < k:
        pad = k - n
        dist = torch.cat([dist, dist.new_full((P, pad), float("inf"))], dim=1)
        index = torch.cat([index, index.new_full((P, pad), -1)], dim=1)
        cat[2:] = [torch.cat([t, t.new_zeros((P, pad) + tuple(t.shape[2:]))], dim=1) for t in cat[2:]]
    empty = index < 0
    dist = torch.where(empty, dist.new_full((), float("inf")), dist)
    key = torch.where(empty, index.new_full((), _I64_MAX), index)
    by_index = torch.sort(key, dim=1, stable=True).indices  # secondary key first, then a stable sort on the primary one
    order = by_index.gather(1, torch.sort(dist.gather(1, by_index), dim=1, stable=True).indices)[:, :k]
    out = [dist.gather(1, order), index.gather(1, order)]
    valid = out[1] >= 0
    for t in cat[2:]:
        rows = t[torch.arange(P, device=t.device)[:, None], order]
        fill = t.new_full((), -1 if t.dtype in _SIGNED else 0)
        out.append(torch.where(valid.view((P, k) + (1,) * (t.dim() - 2)), rows, fill))
    return tuple(out)


def ranking_stats(class_sim_sum: torch.Tensor, class_count: torch.Tensor, proto_class: torch.Tensor, labels: torch.Tensor,
                  index: torch.Tensor, num_real_classes: int):
    """``(class_mean_similarity (P, K), purity (P,), margin (P,), ranking (P,))`` from the sweep's sums (fp64 throughout).

    * mean: sum / count; a class without clips has mean 0 (no division by zero).
    * purity: the share of a prototype's valid entries (index >= 0) whose label is the prototype's class; 0 without a valid entry.
    * margin: the mean on the prototype's own class minus the largest mean on ANOTHER real class that has clips (0 when no other
      real class has one).  An own class without clips -- the abstention prototypes, whose class no clip carries -- counts as mean 0.
    * ranking: prototype indices by descending margin; equal margins keep the lower index first."""
    s = class_sim_sum.to(torch.float64)
    cnt = class_count.to(torch.int64)
    P, K = s.shape
    has = cnt > 0
    mean = torch.where(has[None, :], s / cnt.clamp(min=1).to(torch.float64)[None, :], torch.zeros_like(s))
    pc = proto_class.to(torch.int64)
    valid = index >= 0
    own = (labels == pc[:, None]) & valid
    purity = own.sum(1).to(torch.float64) / valid.sum(1).clamp(min=1).to(torch.float64)
    cls = torch.arange(K, device=s.device)
    other = has[None, :] & (cls[None, :] < int(num_real_classes)) & (cls[None, :] != pc[:, None])
    best_other = torch.where(other, mean, mean.new_full((), float("-inf"))).amax(dim=1)
    best_other = torch.where(other.any(dim=1), best_other, torch.zeros_like(best_other))
    margin = mean.gather(1, pc[:, None])[:, 0] - best_other
    ranking = torch.sort(-margin, stable=True).indices
    return mean, purity, margin, ranking


_filenames = filenames_at


# ------------------------------------------------------------------------------------------------- the sweep
def nearest_clips(dataloader, model, k: int = 10, class_specific: bool = False, abstain_class: bool = True,
                  preprocess_input_function=None, rank: int = 0, world_size: int = 1, keep_sim_scores: bool = False,
                  log=print) -> GlobalExplanation:
    """The k nearest clips of ``dataloader`` per prototype (``class_specific``: among the clips of the prototype's class, with the
    push's exemption of the abstention prototypes), their labels, logits and occurrence maps, and the per-class similarity statistics.
    Batches are ``{"cine", "target_AS"[, "filename"]}`` as for the push; ``world_size > 1`` shards the loader by contiguous batches
    (a sequential sampler is required, as for the sharded push) and merges with all_gathers."""
    from .explain import _is_xproto

    if not _is_xproto(model):
        raise NotImplementedError("global explanations cover XProtoNet and Video_XProtoNet; the reference has none for PPNet")
    push_mod._require_group(world_size)
    was_training = model.training
    model.eval()
    P, K = model.num_prototypes, model.num_classes
    device = model.prototype_vectors.device
    state = TopKState(P, k, device)
    proto_class = push_mod._proto_classes(model).to(device)
    mask = push_mod.xproto_class_mask(P, K, class_specific, abstain_class).to(device)
    class_sum = torch.zeros((P, K), dtype=torch.float64, device=device)
    class_count = torch.zeros((K,), dtype=torch.int64, device=device)
    lib = _lib.lib()
    names, sims, targets = {}, [], []
    for _, base, sample, xdev, labels in sweep_batches(dataloader, device, rank, world_size, preprocess_input_function):
        with torch.no_grad():
            _, proto_dist, occ, logits = model.push_forward(xdev)
        proto_dist = proto_dist.contiguous()
        B = int(proto_dist.shape[0])
        state.update(proto_dist, labels, proto_class, mask, base)
        state.gather("occ", occ, True, base)
        state.gather("logits", logits, False, base)
        state.gather("labels", labels, False, base, fill=-1)
        _lib.check(lib.pasn_proto_class_stats(proto_dist.data_ptr(), labels.data_ptr(), B, P, K, class_sum.data_ptr(),
                                              class_count.data_ptr(), _lib.current_stream()))
        files = sample.get("filename")
        names[base] = [None] * B if files is None else list(files)
        if keep_sim_scores:
            sims.append(1 - proto_dist)
            targets.append(labels)
    if not state.store.agree(world_size):
        raise ValueError("nearest_clips: the loader holds no batch")
    rows = (state.dist, state.index, state.resolved("labels"), state.resolved("logits"), state.resolved("occ"))
    sim_scores = torch.cat(sims) if sims else None
    tgt = torch.cat(targets) if targets else None
    if world_size > 1:
        import torch.distributed as dist

        rows = merge_topk(gather_ranks(rows, device))
        for t in (class_sum, class_count):
            buf = push_mod._for_collective(t)
            dist.all_reduce(buf)
            t.copy_(buf.to(device))
        every = [None] * world_size
        dist.all_gather_object(every, (names, None if sim_scores is None else sim_scores.cpu(), None if tgt is None else tgt.cpu()))
        names = {b: n for part in every for b, n in part[0].items()}
        if keep_sim_scores:  # shards are contiguous and rank-ordered: rank-major concatenation is loader order
            sim_scores = torch.cat([p[1] for p in every if p[1] is not None]).to(device)
            tgt = torch.cat([p[2] for p in every if p[2] is not None]).to(device)
    dist_rows, index, labels_rows, logit_rows, occ_rows = rows
    K_real = K - 1 if abstain_class else K
    mean, purity, margin, ranking = ranking_stats(class_sum, class_count, proto_class, labels_rows, index, K_real)
    model.train(was_training)
    log(f"\tglobal explanation: {int(class_count.sum())} labelled clips, k = {k}, best margin {float(margin.max()):.4f} "
        f"(prototype {int(ranking[0])})")
    return GlobalExplanation(dist=dist_rows, similarity=1 - dist_rows, index=index, labels=labels_rows, logits=logit_rows,
                             occurrence_maps=occ_rows, filenames=_filenames(names, index), class_mean_similarity=mean,
                             class_count=class_count, purity=purity, margin=margin, ranking=ranking,
                             prototype_class=proto_class.to(torch.int64), sim_scores=sim_scores, targets=tgt)


# ------------------------------------------------------------------------------------------------- maps of the winners
def nearest_maps(result: GlobalExplanation, clips=None, dataset=None, maps: Optional[str] = "float", lut=None, prototypes=None,
                 alpha: float = 0.3, mean: float = ECHO_MEAN, std: float = ECHO_STD):
    """Normalised, upsampled occurrence maps (and, with ``lut``, overlays) of the winners: ``{"maps": (p, k, [To,] Ho, Wo), "overlays":
    (p, k, [To,] Ho, Wo, 3) or None, "prototypes": (p,)}`` on the result's device, through ``pasn_explain_maps`` with one selected map
    per clip (``explain.prototype_maps`` does the same for the pushed prototypes).

    The winners' source clips are NOT kept during the sweep (P * k video clips are gigabytes): hand them in as ``clips``
    (p, k, C, [To,] Ho, Wo) -- the normalised model input, rows matching ``prototypes`` -- or name the ``dataset`` whose
    ``dataset[index]["cine"]`` is that clip; one prototype's k clips are on the device at a time.  ``prototypes``: the prototype indices
    to render (default all P).  An empty entry (index -1) gives an all-zero map over a zero clip."""
    from .explain import MAPS, _check_lut, _check_src, _maps_launch

    if maps not in MAPS:
        raise ValueError(f"maps must be one of {MAPS}, got {maps!r}")
    if maps is None and lut is None:
        raise ValueError("nothing to compute: pass maps='float' / 'uint8' and / or a lut")
    if (clips is None) == (dataset is None):
        raise ValueError("pass the winners' clips or the dataset to fetch them from (exactly one of the two)")
    occ = result.occurrence_maps
    device = occ.device
    if not occ.is_cuda:
        raise RuntimeError("protoasnet_amd kernels run on the GPU only; there is no CPU fallback")
    P, k = int(occ.shape[0]), int(occ.shape[1])
    video = occ.dim() == 6
    sel = list(range(P)) if prototypes is None else [int(p) for p in prototypes]
    if clips is not None and (clips.shape[0] != len(sel) or clips.shape[1] != k):
        raise ValueError(f"clips {tuple(clips.shape)} do not hold k = {k} clips for each of the {len(sel)} prototypes")
    lut = _check_lut(lut, device)
    index = result.index.cpu()
    out_m, out_o = [], []
    for row, j in enumerate(sel):
        if clips is not None:
            src = clips[row]
        else:
            fetched = [None if int(g) < 0 else torch.as_tensor(dataset[int(g)]["cine"]) for g in index[j]]
            like = next((c for c in fetched if c is not None), None)
            if like is None:
                raise ValueError(f"prototype {j} has no winner to render")
            src = torch.stack([torch.zeros_like(like) if c is None else c for c in fetched])
        src = src.to(device).contiguous()
        if src.dim() != (5 if video else 4):
            raise ValueError(f"the clips must be (k, C, {'To, ' if video else ''}Ho, Wo), got {tuple(src.shape)}")
        out_shape = tuple(int(v) for v in src.shape[2:]) if video else (1, int(src.shape[2]), int(src.shape[3]))
        if lut is not None:
            _check_src(src)
        occ5 = (occ[j] if video else occ[j].unsqueeze(2)).to(torch.float32).contiguous()  # (k, 1, Ti, Hi, Wi): k clips of one map
        with torch.no_grad():
            m, ov = _maps_launch(occ5, None, 1, out_shape, maps, lut, src if lut is not None else None, alpha, mean, std)
        out_m.append(None if m is None else m.reshape((k,) + tuple(m.shape[2:] if video else m.shape[3:])))
        out_o.append(None if ov is None else ov.reshape((k,) + tuple(ov.shape[2:] if video else ov.shape[3:])))
    return {"maps": None if maps is None else torch.stack(out_m), "overlays": None if lut is None else torch.stack(out_o),
            "prototypes": torch.tensor(sel, dtype=torch.int64)}
