"""CPU: the host side of the fused loss criterion (losses.FusedCriterion over csrc/proto_loss.hip): the C-ABI surface, construction from
the reference's ``train.criterion`` blocks, what the constructor refuses, and that the trainer only builds it when asked.  The arithmetic
is a GPU matter (tests/test_gpu_proto_loss.py)."""
import json
import os
import re
import subprocess

import pytest
import torch

from conftest import GOLDEN, REPO

ENTRY_POINTS = ("pasn_proto_loss_fwd", "pasn_proto_loss_bwd")


def test_header_declares_and_library_exports_the_two_entry_points():
    import protoasnet_amd
    from protoasnet_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "protoasnet_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pasn_[a-z0-9_]+)\s*\(", text))
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES
    assert "pasn_proto_loss_desc" in text
    assert "proto_loss.hip" in protoasnet_amd.build.SOURCES


def test_descriptor_binding_matches_the_header_layout(tmp_path):
    """The ctypes structure and the C struct must agree field by field (a C program prints the offsets the header gives)."""
    import ctypes

    from protoasnet_amd import _lib

    names = [n for n, _ in _lib.ProtoLossDesc._fields_]
    body = "".join(f'printf("%zu\\n", offsetof(pasn_proto_loss_desc, {n}));' for n in names)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "protoasnet_amd.h"\nint main(void) {' + body
                   + 'printf("%zu\\n", sizeof(pasn_proto_loss_desc)); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(_lib.ProtoLossDesc, n).offset for n in names] + [ctypes.sizeof(_lib.ProtoLossDesc)]
    assert got == want


class _Model:
    def __init__(self, K, P):
        self.num_classes = K
        self.prototype_class_identity = torch.zeros(P, K)
        self.prototype_class_identity[torch.arange(P), torch.arange(P) // (P // K)] = 1


def test_from_config_accepts_the_reference_criterion_blocks():
    from protoasnet_amd import losses

    cfgs = json.load(open(os.path.join(GOLDEN, "reference_criterion_configs.json")))
    assert sorted(cfgs) == ["Baseline_XProtoNet_Image.yml", "Baseline_XprotoNet_Video.yml", "Ours_ProtoASNet_Image.yml", "Ours_ProtoASNet_Video.yml"]
    for name, c in cfgs.items():
        abstain = c["abstain_class"]
        K = 4 if abstain else 3
        fc = losses.FusedCriterion.from_config(c["criterion"], _Model(K, 10 * K), abstain)
        assert fc.ce_mode == (1 if abstain else 0), name
        assert type(fc.ce).__name__ == ("CeLossAbstain" if abstain else "CeLoss")
        assert fc.patch == 0 and fc.separation.abstain_class == abstain and fc.cluster.num_classes == K
        assert fc.ce.loss_weight == 1 and fc.cluster.loss_weight == 0.8 and fc.separation.loss_weight == 0.08
        assert fc.reductions == [0, 0, 0] and fc.fc_p == 1 and fc.lnorm_fc.loss_weight == 1e-4
        assert fc.transform.loss_weight == 1e-3 and fc.lnorm_occurrence.loss_weight == 0
        assert fc.orthogonality.loss_weight == (0.01 if name == "Ours_ProtoASNet_Image.yml" else 0.0)
        assert fc.lnorm_fc.mask.shape == (K, 10 * K) and float(fc.lnorm_fc.mask.sum()) == 10 * K * (K - 1)
    # the abstention settings of a config are used whenever abstain_class asks for them
    video = cfgs["Baseline_XprotoNet_Video.yml"]["criterion"]
    assert losses.FusedCriterion.from_config(video, _Model(4, 40), True).ce_mode == 1


def test_constructor_rejects_what_the_kernels_do_not_cover():
    from protoasnet_amd import losses as L

    def build(ce=None, cluster=None, sep=None, ortho=None, lmap=None, lfc=None):
        return L.FusedCriterion(ce or L.CeLoss(1, "mean"), cluster or L.ClusterRoiFeat(0.8, 4, "mean"), sep or L.SeparationRoiFeat(0.08, 4, "mean"),
                                ortho, lmap, None, lfc)

    assert build().ce_mode == 0
    with pytest.raises(ValueError, match="max is not a valid value for reduction"):  # torch's words for a criterion's bad reduction
        build(ce=L.CeLoss(1, "max"))
    with pytest.raises(ValueError, match="none is not a valid value for reduction"):
        build(cluster=L.ClusterRoiFeat(0.8, 4, "none"))
    with pytest.raises(ValueError, match="not a valid value for reduction"):
        build(lmap=L.L_norm(p=2, loss_weight=1e-4, reduction="avg"))
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        build(lmap=L.L_norm(p=3, loss_weight=1e-4, reduction="mean"))
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        build(lfc=L.L_norm(p="fro", loss_weight=1e-4))
    assert build(lmap=L.L_norm(p=3, loss_weight=0)).map_p == 1  # a term that is off is never computed: its p is not judged
    ab = L.CeLossAbstain(1, 0.3, "mean", "joined")
    ab.ab_logitpath = "both"  # (the class itself refuses it at construction, with the same words)
    with pytest.raises(AssertionError, match="ab_logitpath must be 'joined' or 'separate'"):
        build(ce=ab)
    with pytest.raises(AssertionError, match="ab_logitpath"):
        L.CeLossAbstain(1, 0.3, "mean", "both")
    bad = L.OrthogonalityLoss(0.01, 4, "per_class")
    bad.mode = "rows"
    with pytest.raises(ValueError, match="mode must be 'per_class' or 'all'"):
        build(ortho=bad)
    with pytest.raises(TypeError, match="ClusterPatch \\+ SeparationPatch"):
        build(cluster=L.ClusterPatch(0.8, 4, "mean"))
    with pytest.raises(ValueError, match="same number of classes"):
        build(sep=L.SeparationRoiFeat(0.08, 5, "mean"))
    assert build(cluster=L.ClusterPatch(0.8, 4, "mean"), sep=L.SeparationPatch(0.08, 4, "mean")).patch == 1
    assert build(ce=L.CeLossAbstain(1, 0.3, "sum", "separate")).ce_mode == 2


def test_compute_refuses_cpu_tensors():
    from protoasnet_amd import losses as L

    fc = L.FusedCriterion(L.CeLoss(1, "mean"), L.ClusterRoiFeat(0.8, 2, "mean"), L.SeparationRoiFeat(0.08, 2, "mean", abstain_class=False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fc.compute(torch.zeros(2, 2), torch.zeros(2, 4), None, None, None, torch.tensor([0, 1]))


def test_trainer_builds_the_fused_criterion_only_when_asked(monkeypatch, tmp_path):
    """``train.fused_loss`` is absent from the reference's configs: the default path never constructs the fused criterion and runs an
    epoch on the CPU stand-in as before; with the key set the trainer holds one built from its own seven loss objects."""
    from protoasnet_amd import losses
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG, Toy, _batches

    built = []
    real = losses.FusedCriterion.__init__

    def spy(self, *a, **k):
        built.append(1)
        real(self, *a, **k)

    monkeypatch.setattr(losses.FusedCriterion, "__init__", spy)
    b = _batches(3, 2)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": dict(TRAIN_CFG, save=False)}
    assert "fused_loss" not in cfg["train"]
    t = DPTrainer(Toy(), cfg, {"train": b, "val": b}, log=lambda *_: None)
    m = t.run_epoch(0, "train")
    assert t.fused is None and not built and len(m["loss_terms"]) == 7
    t_off = DPTrainer(Toy(), dict(cfg, train=dict(cfg["train"], fused_loss=False)), {"train": b, "val": b}, log=lambda *_: None)
    assert t_off.fused is None and not built
    t_on = DPTrainer(Toy(), dict(cfg, train=dict(cfg["train"], fused_loss=True)), {"train": b, "val": b}, log=lambda *_: None)
    assert built == [1] and t_on.fused.ce is t_on.CeLoss and t_on.fused.lnorm_fc is t_on.Lnorm_fc and t_on.fused.ce_mode == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the CPU stand-in cannot run it: an error, never the eager path
        t_on.run_epoch(0, "val")
