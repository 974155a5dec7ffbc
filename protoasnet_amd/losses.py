"""``TransformLoss`` of the reference (src/loss/loss.py:257-320) on the HIP path.

The reference warps the input clip and the occurrence maps with ``torchvision.transforms.functional.affine`` (rotation
in [-20, 20] degrees, scale in [0.6, 1.5], bilinear, fill 0), runs ``model.compute_occurence_map`` on the warped clip and takes
the L1 distance between the two sets of maps.  Here the warp is ``pasn_affine_warp_fwd`` / ``_bwd`` (csrc/warp.hip) under a small
``autograd.Function``; the second trunk pass is the compiled training pass of ``compute_occurence_map``; the L1 reduction over
the (N, P, T', H', W') maps is a plain torch op on a tiny tensor.  Same constructor arguments and ``compute`` signature as the
reference class, so an agent swaps the import only.  No torchvision is needed (it is absent from this image)."""
from __future__ import annotations

import ctypes
import random

import torch

from . import _lib


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, angle, scale):
        if not x.is_cuda:
            raise RuntimeError("protoasnet_amd.losses run on the GPU only; there is no CPU fallback")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        h, w = x.shape[-2], x.shape[-1]
        planes = x.numel() // (h * w)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().pasn_affine_warp_fwd(x.data_ptr(), y.data_ptr(), planes, h, w, float(angle), float(scale), _lib.dtype_code(x.dtype),
                                                   _lib.current_stream()))
        ctx.geom = (planes, h, w, float(angle), float(scale), x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        planes, h, w, angle, scale, dtype = ctx.geom
        dyf = dy.contiguous().float()
        dx = torch.zeros_like(dyf)
        _lib.check(_lib.lib().pasn_affine_warp_bwd(dyf.data_ptr(), dx.data_ptr(), planes, h, w, angle, scale, _lib.current_stream()))
        return dx.to(dtype), None, None


def affine_warp(x: torch.Tensor, angle: float, scale: float) -> torch.Tensor:
    """Every trailing (H, W) plane of ``x`` rotated by ``angle`` degrees about its centre and scaled by ``scale`` (torchvision
    ``affine`` with translate = (0, 0), shear = 0, bilinear interpolation, fill = 0)."""
    return _AffineWarp.apply(x, angle, scale)


def get_affine_config() -> dict:
    """The reference's sampler (loss.py:257-269): the keys that vary."""
    return {"angle": random.uniform(-20, 20), "scale": random.uniform(0.6, 1.5)}


class TransformLoss(object):
    """reference src/loss/loss.py:272-320 -- same arguments, same ``compute(x, occurrence_map, model)``."""

    def __init__(self, loss_weight=1e-4, reduction="sum"):
        self.loss_weight = loss_weight
        self.reduction = reduction

    def compute(self, x, occurrence_map, model, config=None):
        if self.loss_weight == 0:
            return torch.tensor(0, device=x.device)
        cfg = config or get_affine_config()
        transformed_x = affine_warp(x, cfg["angle"], cfg["scale"])  # per-frame 2-D warp of (N,3,[T,]H,W)
        return self.compute_from_maps(occurrence_map, model.compute_occurence_map(transformed_x), cfg)

    def paired_forward(self, x, model, config=None):
        """The model's forward AND this term from ONE trunk pass over [x, warp(x)] (``model.forward_pair``): returns
        ``((logits, similarity, occurrence_map), loss_term)``.  The affine parameters are drawn here, i.e. BEFORE the forward where
        ``compute`` draws them after it; nothing in between consumes random numbers, so a seeded run sees the same transforms."""
        if self.loss_weight == 0 or not hasattr(model, "forward_pair"):
            out = model(x)
            return out, (torch.zeros((), device=x.device) if self.loss_weight == 0 else self.compute(x, out[2], model, config))
        cfg = config or get_affine_config()
        out, occ_t = model.forward_pair(x, affine_warp(x, cfg["angle"], cfg["scale"]))
        return out, self.compute_from_maps(out[2], occ_t, cfg)

    def compute_from_maps(self, occurrence_map, occurrence_map_transformed, config):
        """loss.py:302-320 once both sets of maps exist: ``occurrence_map_transformed`` = the model's maps of the warped clip (the
        caller may have produced them in the same pass as the originals: eval mode uses running statistics, so a 2N-clip batch of
        [clips, warped clips] gives each clip exactly what two N-clip passes give)."""
        occ_t = occurrence_map_transformed.squeeze(2)  # (N, P, [T',] H', W')
        warped = affine_warp(occurrence_map.squeeze(2), config["angle"], config["scale"])
        loss = (occ_t - warped).abs().sum()
        if self.reduction == "mean":
            loss = loss / (occ_t.shape[0] * occ_t.shape[1])
        return self.loss_weight * loss


# --------------------------------------------------------------------------------------------------------------------------
# The rest of the reference's loss stack (src/loss/loss.py): small reductions over (N, K) / (N, P) / (P, D) tensors, i.e. host
# plumbing in plain torch -- provided so a training step needs nothing from the reference's loss module (whose import drags in
# torchvision).  Same class names, constructor arguments and ``compute`` signatures; pinned against the reference's outputs and
# gradients by tests/golden/g6_losses.npz.
# --------------------------------------------------------------------------------------------------------------------------
def _zero(t):
    return torch.tensor(0, device=t.device)


def _per_class_extreme(scores, num_classes, largest, proto_class=None):
    """(N, P) scores -> (N, classes): best prototype score of every class.  ``proto_class`` None: the prototypes are laid out class-major
    in equal blocks (the model as built).  Else (P,) the class of every prototype -- a pruned model whose classes own different numbers
    of prototypes --: the extreme over each class's own prototypes; a class that owns none contributes 0."""
    if proto_class is not None:
        own = _class_mask(proto_class, num_classes, scores.device)  # (classes, P)
        fill = float("-inf") if largest else float("inf")
        spread = scores[:, None, :].masked_fill(~own[None], fill)
        best = spread.amax(dim=2) if largest else spread.amin(dim=2)
        return torch.where(own.any(dim=1)[None], best, torch.zeros_like(best))
    if scores.shape[1] % num_classes:
        from .prune import check_class_blocks

        check_class_blocks(scores.shape[1], num_classes, "the cluster / separation cost")
    grouped = scores.reshape(scores.shape[0], num_classes, -1)
    return grouped.max(dim=2)[0] if largest else grouped.min(dim=2)[0]


def _class_mask(proto_class, num_classes, device):
    if proto_class.shape[0] == 0 or int(proto_class.max()) >= num_classes or int(proto_class.min()) < 0:
        raise ValueError(f"proto_class must hold classes in [0, {num_classes})")
    return proto_class.to(device)[None, :] == torch.arange(num_classes, device=device)[:, None]


def _class_index(loss, P):
    """``loss.proto_class`` (None: equal class-major blocks), checked against the P prototypes the cost is handed."""
    pc = loss.proto_class
    if pc is not None and pc.shape[0] != P:
        raise ValueError(f"unbalanced prototype blocks: the criterion groups {pc.shape[0]} prototypes by class, the model has {P} "
                         "(rebuild the criterion after pruning)")
    return pc


def _batch_reduce(per_class, reduction):
    """(N, classes) -> scalar: 'sum' over everything, 'mean' = batch mean then class sum (the reference's convention)."""
    return per_class.mean(dim=0).sum() if reduction == "mean" else per_class.sum()


class CeLoss(object):
    """loss.py:23-34"""

    def __init__(self, loss_weight=1, reduction="mean"):
        self.loss_weight, self.reduction = loss_weight, reduction

    def compute(self, logits, target):
        if self.loss_weight == 0:
            return _zero(target)
        return self.loss_weight * torch.nn.functional.cross_entropy(logits, target, reduction=self.reduction)


class ClusterPatch(object):
    proto_class = None  # (P,) class of every prototype when the blocks are unequal (DPTrainer.get_criterion sets it)

    """loss.py:37-65 -- ProtoPNet cluster cost on min_distances (N, P)."""

    def __init__(self, loss_weight, num_classes=4, reduction="mean"):
        self.loss_weight, self.num_classes, self.reduction = loss_weight, num_classes, reduction

    def compute(self, min_distances, target):
        if self.loss_weight == 0:
            return _zero(target)
        own = torch.nn.functional.one_hot(target, num_classes=self.num_classes)
        return self.loss_weight * _batch_reduce(_per_class_extreme(min_distances, self.num_classes, False, _class_index(self, min_distances.shape[1])) * own, self.reduction)


class SeparationPatch(object):
    proto_class = None  # (P,) class of every prototype when the blocks are unequal (DPTrainer.get_criterion sets it)

    """loss.py:68-95 -- ProtoPNet separation cost."""

    def __init__(self, loss_weight, num_classes=4, reduction="mean"):
        self.loss_weight, self.num_classes, self.reduction = loss_weight, num_classes, reduction

    def compute(self, min_distances, target):
        if self.loss_weight == 0:
            return _zero(target)
        other = 1 - torch.nn.functional.one_hot(target, num_classes=self.num_classes)
        return -self.loss_weight * _batch_reduce(_per_class_extreme(min_distances, self.num_classes, False, _class_index(self, min_distances.shape[1])) * other, self.reduction)


class ClusterRoiFeat(object):
    proto_class = None  # (P,) class of every prototype when the blocks are unequal (DPTrainer.get_criterion sets it)

    """loss.py:98-138 -- XProtoNet cluster cost on similarities (N, P)."""

    def __init__(self, loss_weight, num_classes=4, reduction="sum"):
        self.loss_weight, self.num_classes, self.reduction = loss_weight, num_classes, reduction

    def compute(self, similarities, target):
        if self.loss_weight == 0:
            return _zero(target)
        own = torch.nn.functional.one_hot(target, num_classes=self.num_classes)
        return -self.loss_weight * _batch_reduce(_per_class_extreme(similarities, self.num_classes, True, _class_index(self, similarities.shape[1])) * own, self.reduction)


class SeparationRoiFeat(object):
    proto_class = None  # (P,) class of every prototype when the blocks are unequal (DPTrainer.get_criterion sets it)

    """loss.py:141-183 -- XProtoNet separation cost; the abstain class (last) is never penalised when ``abstain_class``."""

    def __init__(self, loss_weight, num_classes=4, reduction="sum", abstain_class=True):
        self.loss_weight, self.num_classes, self.reduction, self.abstain_class = loss_weight, num_classes, reduction, abstain_class

    def compute(self, similarities, target):
        if self.loss_weight == 0:
            return _zero(target)
        own = torch.nn.functional.one_hot(target, num_classes=self.num_classes)
        if self.abstain_class:
            own = own.clone()
            own[:, -1] = 1
        return self.loss_weight * _batch_reduce(_per_class_extreme(similarities, self.num_classes, True, _class_index(self, similarities.shape[1])) * (1 - own), self.reduction)


class OrthogonalityLoss(object):
    proto_class = None  # as in the cluster / separation costs

    """loss.py:186-229 -- sum of the pairwise cosine similarities of the prototypes (upper triangle), per class or over all."""

    def __init__(self, loss_weight, num_classes=4, mode="per_class"):
        if mode not in ("per_class", "all"):
            raise ValueError("mode must be 'per_class' or 'all'")
        self.loss_weight, self.num_classes, self.mode = loss_weight, num_classes, mode

    def compute(self, prototype_vectors):
        if self.loss_weight == 0:
            return _zero(prototype_vectors)
        p = prototype_vectors.reshape(prototype_vectors.shape[0], prototype_vectors.shape[1])
        if self.mode == "per_class" and self.proto_class is not None:  # unequal blocks: the pairs of a class, picked by a mask
            c = _class_index(self, p.shape[0]).to(p.device)
            sim = torch.nn.functional.cosine_similarity(p.unsqueeze(1), p.unsqueeze(0), dim=2)
            return self.loss_weight * (torch.triu(sim, diagonal=1) * (c[:, None] == c[None, :])).sum()
        if self.mode == "per_class":
            if p.shape[0] % self.num_classes:
                from .prune import check_class_blocks

                check_class_blocks(p.shape[0], self.num_classes, "the per-class orthogonality loss")
            p = p.reshape(self.num_classes, -1, p.shape[1])
            sim = torch.nn.functional.cosine_similarity(p.unsqueeze(1), p.unsqueeze(2), dim=3)
        else:
            sim = torch.nn.functional.cosine_similarity(p.unsqueeze(1), p.unsqueeze(0), dim=2)
        return self.loss_weight * torch.triu(sim, diagonal=1).sum()


class L_norm(object):  # noqa: N801 -- reference class name
    """loss.py:232-254 -- p-norm of a tensor (the occurrence maps), optionally masked."""

    def __init__(self, mask=None, p=1, loss_weight=1e-4, reduction="sum"):
        self.mask, self.p, self.loss_weight, self.reduction = mask, p, loss_weight, reduction

    def compute(self, tensor, dim=None):
        if self.loss_weight == 0:
            return _zero(tensor)
        t = tensor if self.mask is None else self.mask.to(tensor.device) * tensor
        loss = t.norm(p=self.p, dim=dim)
        if self.reduction == "mean":
            loss = loss.mean(dim=0).sum()
        elif self.reduction == "sum":
            loss = loss.sum()
        return self.loss_weight * loss


class CeLossAbstain(object):
    """loss.py:323-371 -- cross entropy with a learned abstention output (the K+1-th logit)."""

    def __init__(self, loss_weight=1, ab_weight=0.3, reduction="sum", ab_logitpath="joined"):
        if ab_logitpath not in ("joined", "separate"):
            raise AssertionError("ab_logitpath must be 'joined' or 'separate'")
        self.loss_weight, self.ab_weight, self.reduction, self.ab_logitpath = loss_weight, ab_weight, reduction, ab_logitpath

    def to(self, device):
        return None

    def compute(self, logits, target):
        if self.loss_weight == 0:
            return _zero(target)
        k = logits.shape[1] - 1
        assert k >= 2, "CeLossAbstain input must have >= 2 classes not including abstention"
        abstain = (logits.softmax(dim=1) if self.ab_logitpath == "joined" else logits.sigmoid())[:, k: k + 1]
        virtual = (1 - abstain) * logits[:, :k].softmax(dim=1) + abstain * torch.nn.functional.one_hot(target, num_classes=k)
        loss_pred = torch.nn.functional.nll_loss(torch.log(virtual), target, reduction=self.reduction)
        loss_abs = -torch.log(1 - abstain).squeeze()
        loss_abs = loss_abs.mean() if self.reduction == "mean" else loss_abs.sum() if self.reduction == "sum" else loss_abs
        return self.loss_weight * (loss_pred + self.ab_weight * loss_abs)


# --------------------------------------------------------------------------------------------------------------------------
# The same recipe in the library: ``pasn_proto_loss_fwd`` / ``_bwd`` (csrc/proto_loss.hip) compute the seven terms of a training
# step (XProtoNet_Base.py:54-81 as Video_XProtoNet_e2e.py:86-110 applies them), their sum and the epoch statistics in at most two
# launches each way, where the classes above cost a few dozen eager launches forward and again under autograd.
# --------------------------------------------------------------------------------------------------------------------------
def _reduction_code(reduction):
    if reduction not in ("mean", "sum"):
        raise ValueError(f"{reduction} is not a valid value for reduction")  # what torch's criteria say (loss.py:25,336)
    return 0 if reduction == "mean" else 1


def _norm_p(loss, what):
    if loss.loss_weight != 0 and loss.p not in (1, 2):
        raise ValueError(f"L_norm of {what}: p must be 1 or 2, not {loss.p!r}")
    return int(loss.p) if loss.p in (1, 2) else 1


class _FusedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, crit, target, stats, logit, scores, occ, protos, fc_w, transform_term):
        d, mask = crit._describe(logit, scores, occ, protos, fc_w)
        dev = logit.device
        logit, scores, target = logit.contiguous(), scores.contiguous(), target.contiguous()
        occ = None if occ is None or d.w_map == 0 else occ.contiguous()
        protos = None if protos is None else protos.contiguous()
        fc_w = None if fc_w is None else fc_w.contiguous()
        tt = None if transform_term is None else transform_term.detach().float().reshape(1)
        out = torch.empty(8, dtype=torch.float32, device=dev)  # the seven terms, then their sum
        ws = torch.empty(d.N * d.P + d.P, dtype=torch.float32, device=dev) if (d.w_map != 0 or d.w_ortho != 0) else None
        cm, loss_sum = stats if stats is not None else (None, None)
        _lib.check(_lib.lib().pasn_proto_loss_fwd(logit.data_ptr(), scores.data_ptr(), target.data_ptr(), _lib.ptr(protos), _lib.ptr(occ),
                                                  _lib.ptr(fc_w), _lib.ptr(mask), _lib.ptr(tt), out.data_ptr(), out[7:].data_ptr(), _lib.ptr(ws),
                                                  _lib.ptr(cm), _lib.ptr(loss_sum), ctypes.byref(d), _lib.current_stream()))
        ctx.desc = d
        ctx.save_for_backward(logit, scores, target, protos, occ, fc_w, mask, ws)
        terms = out[:7]
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for the terms
        return out[7], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        if grad_loss is None:
            return (None,) * 9
        d = ctx.desc
        logit, scores, target, protos, occ, fc_w, mask, ws = ctx.saved_tensors
        need = ctx.needs_input_grad[3:]
        g = grad_loss.detach().float().contiguous().reshape(1)  # stays on the device
        d_logit = torch.empty_like(logit) if need[0] else None
        d_scores = torch.empty_like(scores) if need[1] else None
        d_occ = torch.empty_like(occ) if need[2] and occ is not None else None  # weight 0: no gradient (None is autograd's zero)
        d_protos = torch.empty_like(protos) if need[3] and protos is not None and d.w_ortho != 0 else None
        d_fc = torch.empty_like(fc_w) if need[4] and fc_w is not None and d.w_fc != 0 else None
        if any(t is not None for t in (d_logit, d_scores, d_occ, d_protos, d_fc)):
            _lib.check(_lib.lib().pasn_proto_loss_bwd(g.data_ptr(), logit.data_ptr(), scores.data_ptr(), target.data_ptr(), _lib.ptr(protos),
                                                      _lib.ptr(occ), _lib.ptr(fc_w), _lib.ptr(mask), _lib.ptr(ws), _lib.ptr(d_logit),
                                                      _lib.ptr(d_scores), _lib.ptr(d_protos), _lib.ptr(d_occ), _lib.ptr(d_fc), ctypes.byref(d),
                                                      _lib.current_stream()))
        return None, None, None, d_logit, d_scores, d_occ, d_protos, d_fc, (grad_loss if need[5] else None)


class FusedCriterion(object):
    """The seven loss objects of a trainer (``CeLoss`` or ``CeLossAbstain``; ``ClusterRoiFeat`` + ``SeparationRoiFeat`` or the ProtoPNet
    pair ``ClusterPatch`` + ``SeparationPatch``; ``OrthogonalityLoss``; the two ``L_norm``; ``TransformLoss``) evaluated by ONE library call.
    ``transform`` stays what it is -- its value enters ``compute`` as ``transform_term``; ``orthogonality`` / ``lnorm_occurrence`` /
    ``lnorm_fc`` may be None (weight 0).  Construction needs no device and checks what the kernels cover; ``compute`` runs on the GPU
    only."""

    TERMS = ("ce", "cluster", "separation", "orthogonality", "lnorm_occurrence", "transform", "lnorm_fc")

    def __init__(self, ce, cluster, separation, orthogonality=None, lnorm_occurrence=None, transform=None, lnorm_fc=None):
        self.ce, self.cluster, self.separation = ce, cluster, separation
        self.orthogonality = orthogonality or OrthogonalityLoss(0)
        self.lnorm_occurrence = lnorm_occurrence or L_norm(loss_weight=0)
        self.transform = transform or TransformLoss(0)
        self.lnorm_fc = lnorm_fc or L_norm(loss_weight=0)
        if isinstance(ce, CeLossAbstain):
            if ce.ab_logitpath not in ("joined", "separate"):
                raise AssertionError("ab_logitpath must be 'joined' or 'separate'")
            self.ce_mode = 1 if ce.ab_logitpath == "joined" else 2
        elif isinstance(ce, CeLoss):
            self.ce_mode = 0
        else:
            raise TypeError(f"ce must be a CeLoss or a CeLossAbstain, not {type(ce).__name__}")
        patch = isinstance(cluster, ClusterPatch), isinstance(separation, SeparationPatch)
        if patch[0] != patch[1] or not isinstance(cluster, (ClusterPatch, ClusterRoiFeat)) or not isinstance(separation, (SeparationPatch, SeparationRoiFeat)):
            raise TypeError("cluster / separation must be ClusterRoiFeat + SeparationRoiFeat or ClusterPatch + SeparationPatch")
        self.patch = int(patch[0])
        if cluster.num_classes != separation.num_classes or (self.orthogonality.loss_weight != 0 and self.orthogonality.num_classes != cluster.num_classes):
            raise ValueError("the cluster, separation and orthogonality costs must group the prototypes into the same number of classes")
        if self.orthogonality.mode not in ("per_class", "all"):
            raise ValueError("mode must be 'per_class' or 'all'")
        self.reductions = [_reduction_code(x.reduction) for x in (ce, cluster, separation)]
        self.map_reduction = _reduction_code(self.lnorm_occurrence.reduction) if self.lnorm_occurrence.loss_weight != 0 else 1
        self.map_p, self.fc_p = _norm_p(self.lnorm_occurrence, "the occurrence maps"), _norm_p(self.lnorm_fc, "the last layer")
        if self.lnorm_occurrence.mask is not None:
            raise ValueError("L_norm of the occurrence maps takes no mask")
        self._mask = None

    @classmethod
    def from_config(cls, criterion: dict, model, abstain_class: bool) -> "FusedCriterion":
        """From a ``train.criterion`` block of the reference's XProto configs, as ``XProtoNet_Base.get_criterion`` reads it (:54-81)."""
        cfg, K = criterion, model.num_classes
        from .prune import require_balanced

        require_balanced(model, "the one-launch criterion (it indexes equal class blocks)")
        ce = CeLossAbstain(**cfg["CeLossAbstain"]) if abstain_class else CeLoss(**cfg["CeLoss"])
        return cls(ce, ClusterRoiFeat(num_classes=K, **cfg["ClusterRoiFeat"]),
                   SeparationRoiFeat(num_classes=K, **cfg["SeparationRoiFeat"], abstain_class=bool(abstain_class)),
                   OrthogonalityLoss(num_classes=K, **cfg["OrthogonalityLoss"]), L_norm(**cfg["Lnorm_occurrence"]),
                   TransformLoss(**cfg["trans_occurrence"]), L_norm(**cfg["Lnorm_FC"], mask=1 - torch.t(model.prototype_class_identity)))

    def _describe(self, logit, scores, occ, protos, fc_w):
        for name, t in (("logit", logit), ("similarities", scores), ("prototype_vectors", protos), ("fc_weight", fc_w)):
            if t is not None and t.dtype != torch.float32:
                raise TypeError(f"FusedCriterion: {name} must be float32, not {t.dtype}")
        if logit.dim() != 2 or scores.dim() != 2 or scores.shape[0] != logit.shape[0]:
            raise ValueError("FusedCriterion: logit is (N, K) and similarities (N, P)")
        d = _lib.ProtoLossDesc()
        d.N, d.K, d.P = logit.shape[0], logit.shape[1], scores.shape[1]
        d.K_real = d.K - 1 if self.ce_mode else d.K
        d.C, d.patch = self.cluster.num_classes, self.patch
        d.ce_mode, d.ab_weight = self.ce_mode, float(getattr(self.ce, "ab_weight", 0.0))
        d.ce_reduction, d.cluster_reduction, d.sep_reduction = self.reductions
        d.sep_abstain = int(bool(getattr(self.separation, "abstain_class", False)))
        d.ortho_mode, d.map_p, d.map_reduction, d.fc_p = int(self.orthogonality.mode == "all"), self.map_p, self.map_reduction, self.fc_p
        d.w_ce, d.w_cluster, d.w_sep = float(self.ce.loss_weight), float(self.cluster.loss_weight), float(self.separation.loss_weight)
        d.w_ortho = float(self.orthogonality.loss_weight) if protos is not None else 0.0
        d.w_map = float(self.lnorm_occurrence.loss_weight) if occ is not None else 0.0
        d.w_fc = float(self.lnorm_fc.loss_weight) if fc_w is not None else 0.0
        if protos is not None:
            if protos.shape[0] != d.P or protos.numel() != d.P * protos.shape[1]:
                raise ValueError("FusedCriterion: prototype_vectors is (P, D, 1, ...)")
            d.D = protos.shape[1]
        if occ is not None and d.w_map != 0:
            if occ.shape[0] != d.N or occ.shape[1] != d.P:
                raise ValueError("FusedCriterion: occurrence_map is (N, P, 1, [T,] H, W)")
            d.S, d.map_dtype = occ.numel() // (d.N * d.P), _lib.dtype_code(occ.dtype)
        mask = None
        if fc_w is not None and d.w_fc != 0:
            if fc_w.dim() != 2 or fc_w.shape[1] != d.P:
                raise ValueError("FusedCriterion: fc_weight is (K, P)")
            d.fc_rows = fc_w.shape[0]
            if self.lnorm_fc.mask is not None:
                if self._mask is None or self._mask.device != fc_w.device:
                    self._mask = self.lnorm_fc.mask.to(device=fc_w.device, dtype=torch.float32).contiguous()
                if self._mask.shape != fc_w.shape:
                    raise ValueError("FusedCriterion: the mask of the last-layer norm must have the weight's shape")
                mask = self._mask
        return d, mask

    def compute(self, logit, similarities, occurrence_map, prototype_vectors, fc_weight, target, transform_term=None, stats=None):
        """``(loss, terms)``: the differentiable sum and the detached (7,) fp32 vector of the weighted terms in ``TERMS`` order.
        ``transform_term``: the value of ``TransformLoss.compute`` / ``compute_from_maps`` (None = 0); it is added in the launch and
        receives the upstream gradient.  ``stats = (cm, loss_sum)``: a (K_real * K_real) int64 confusion matrix [label, prediction] and
        a (7,) fp32 vector, both updated in the same launch."""
        for t in (logit, similarities, occurrence_map, prototype_vectors, fc_weight, target, transform_term) + tuple(stats or ()):
            if t is not None and not t.is_cuda:
                raise RuntimeError("protoasnet_amd.losses run on the GPU only; there is no CPU fallback")
        if target.dtype != torch.int64:
            target = target.long()
        if stats is not None:
            cm, loss_sum = stats
            k = logit.shape[1] - 1 if self.ce_mode else logit.shape[1]
            if cm.dtype != torch.int64 or cm.numel() != k * k or loss_sum.dtype != torch.float32 or loss_sum.numel() != 7 or not (
                    cm.is_contiguous() and loss_sum.is_contiguous()):
                raise ValueError("FusedCriterion: stats is (int64 confusion matrix of K_real * K_real, float32 loss_sum of 7), both contiguous")
        return _FusedLossFn.apply(self, target, stats, logit, similarities, occurrence_map, prototype_vectors, fc_weight, transform_term)
