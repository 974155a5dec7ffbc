"""Seeded inputs and the case list shared by tests/golden/make_golden_loss_recipe.py (which runs the reference's loss classes as its
training loop applies them) and tests/test_gpu_proto_loss.py (which runs ``losses.FusedCriterion`` on the same inputs), plus the gates
both proto-loss test files use."""
import torch

# The project's own gates for the loss classes against the reference's fixture (tests/test_cpu_losses.py).
LOSS_RTOL, LOSS_ATOL = 1e-6, 1e-7
GRAD_RTOL, GRAD_ATOL = 1e-5, 1e-7
# A bf16 gradient is the fp32 gradient rounded to 8 significant bits: half a unit in the last place is 2^-9 of the value.
BF16_RTOL = 2.0 ** -8

N, D, MAP = 5, 32, (4, 7, 7)

# The `train.criterion` weights of the reference's two video configs (Ours_ProtoASNet_Video.yml:31-58 with abstain_class: True,
# Baseline_XprotoNet_Video.yml:31-58 with abstain_class: False); the transform term is an input of the fused call, not part of it.
_OURS = dict(ce=("CeLossAbstain", dict(loss_weight=1, ab_weight=0.3, ab_logitpath="joined", reduction="mean")),
             cluster=("ClusterRoiFeat", dict(loss_weight=0.8, reduction="mean")), sep=("SeparationRoiFeat", dict(loss_weight=0.08, reduction="mean")),
             ortho=dict(loss_weight=0.0, mode="per_class"), lmap=dict(p=2, loss_weight=0.0, reduction="mean"), lfc=dict(p=1, loss_weight=1e-4))
_BASE = dict(_OURS, ce=("CeLoss", dict(loss_weight=1, reduction="mean")))
_LIVE = dict(ortho=dict(loss_weight=0.01, mode="per_class"), lmap=dict(p=2, loss_weight=1e-2, reduction="mean"))

CASES = [
    # tag, recipe, abstain_class, classes of the prototype groups, prototypes, map dtype
    ("ours_video", _OURS, True, 4, 40, "fp32"),
    ("ours_video_live", dict(_OURS, **_LIVE), True, 4, 40, "fp32"),
    ("baseline_video", _BASE, False, 3, 30, "fp32"),
    ("baseline_video_live", dict(_BASE, **_LIVE), False, 3, 30, "fp32"),
    # what g6_losses.npz does not hold at this size: the ProtoPNet signs, the other norms and reductions, a bf16 map
    ("patch_signs", dict(_BASE, cluster=("ClusterPatch", dict(loss_weight=0.8, reduction="mean")),
                         sep=("SeparationPatch", dict(loss_weight=0.08, reduction="sum"))), False, 3, 30, "fp32"),
    ("other_norms", dict(_OURS, ce=("CeLossAbstain", dict(loss_weight=0.5, ab_weight=0.7, ab_logitpath="separate", reduction="sum")),
                         ortho=dict(loss_weight=0.01, mode="all"), lmap=dict(p=1, loss_weight=1e-2, reduction="sum"),
                         lfc=dict(p=2, loss_weight=1e-2)), True, 4, 40, "fp32"),
    ("ours_video_live_bf16", dict(_OURS, **_LIVE), True, 4, 40, "bf16"),
]
OUTPUTS = ("logit", "scores", "protos", "occ", "fc_w")


def make_inputs(tag):
    """The tensors one training step hands to the criterion, from a generator seeded by the case."""
    _, _, abstain, C, P, map_dtype = next(c for c in CASES if c[0] == tag)
    g = torch.Generator().manual_seed(1000 + [c[0] for c in CASES].index(tag))
    k_real = C - 1 if abstain else C
    occ = torch.rand((N, P, 1) + MAP, generator=g) - 0.3
    if map_dtype == "bf16":
        occ = occ.bfloat16()
    identity = torch.zeros(P, C)
    identity[torch.arange(P), torch.arange(P) // (P // C)] = 1
    return {"logit": torch.randn(N, C, generator=g), "scores": torch.rand(N, P, generator=g), "protos": torch.rand(P, D, 1, 1, 1, generator=g),
            "occ": occ, "fc_w": torch.randn(C, P, generator=g) * 0.5, "target": torch.randint(0, k_real, (N,), generator=g),
            "prototype_class_identity": identity}


def build_losses(mod, tag):
    """The seven loss objects of ``XProtoNet_Base.get_criterion`` from classes of ``mod`` (the reference's loss module or
    ``protoasnet_amd.losses``); the transform slot is None."""
    _, r, abstain, C, P, _ = next(c for c in CASES if c[0] == tag)
    identity = make_inputs(tag)["prototype_class_identity"]
    ce = getattr(mod, r["ce"][0])(**r["ce"][1])
    cluster = getattr(mod, r["cluster"][0])(num_classes=C, **r["cluster"][1])
    sep_kw = dict(abstain_class=abstain) if r["sep"][0] == "SeparationRoiFeat" else {}
    sep = getattr(mod, r["sep"][0])(num_classes=C, **r["sep"][1], **sep_kw)
    return (ce, cluster, sep, mod.OrthogonalityLoss(num_classes=C, **r["ortho"]), mod.L_norm(**r["lmap"]), None,
            mod.L_norm(**r["lfc"], mask=1 - torch.t(identity)))


def eager_terms(objs, t):
    """The recipe as the training loop writes it (Video_XProtoNet_e2e.py:86-110), the transform term left out: the list of terms."""
    ce, cluster, sep, ortho, lmap, _, lfc = objs
    return [ce.compute(logits=t["logit"], target=t["target"]), cluster.compute(t["scores"], t["target"]), sep.compute(t["scores"], t["target"]),
            ortho.compute(t["protos"]), lmap.compute(t["occ"], dim=(-3, -2, -1)), lfc.compute(t["fc_w"])]
