"""CPU: the host side of the on-device augmentation -- the parameter sampler (torchvision's RandomResizedCrop.get_params and the
reference's RandomRotateVideo angle, restated), ``DeviceClipPipeline.from_config`` on the reference configs' ``data`` keys, the trainer's
per-rank seeding, and the ``pasn_clip_augment`` symbol of the C-ABI."""
import json
import math
import os
import re

import pytest
import torch

from conftest import GOLDEN, REPO
from protoasnet_amd import _lib, data


def _draw(n, H, W, ratio, deg, seed=0):
    return data.sample_augment_params(n, H, W, ratio, deg, torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("H,W,ratio,deg", [(112, 112, 0.7, 15), (224, 224, 0.7, 15), (37, 53, 0.5, 7.3), (64, 48, 0.08, 90)])
def test_sampler_invariants(H, W, ratio, deg):
    t = _draw(2000, H, W, ratio, deg)
    assert t.shape == (2000, 6) and t.dtype == torch.float32
    i, j, h, w = (t[:, k].long() for k in range(4))
    assert bool((t[:, :4] == t[:, :4].round()).all())
    assert bool((i >= 0).all() and (j >= 0).all() and (h >= 1).all() and (w >= 1).all())
    assert bool((i + h <= H).all() and (j + w <= W).all())
    # area in [ratio, 1] of H*W and aspect in [3/4, 4/3], up to the rounding of h and w to integers
    area = (h * w).double() / (H * W)
    slack = (h + w + 1).double() / (H * W)
    assert bool((area >= ratio - slack).all() and (area <= 1.0).all())
    aspect = w.double() / h.double()
    tol_a = 1.0 / h.double() + 1.0 / w.double()
    assert bool((aspect >= 0.75 * (1 - tol_a) - 1e-9).all() and (aspect <= (4.0 / 3.0) * (1 + tol_a) + 1e-9).all())
    ang = torch.rad2deg(torch.atan2(t[:, 5].double(), t[:, 4].double()))
    assert bool((ang.abs() <= deg + 1e-4).all())
    assert float(ang.max()) > 0.8 * deg and float(ang.min()) < -0.8 * deg  # the whole range is drawn
    assert bool(((t[:, 4].double() ** 2 + t[:, 5].double() ** 2 - 1).abs() < 1e-6).all())
    # crops really vary: positions and sizes both
    assert len(set(h.tolist())) > 3 and len(set(i.tolist())) > 3


def test_sampler_central_crop_fallback():
    """A plane far wider than 4/3 at scale 1: no attempt fits, torchvision's fallback takes the central crop at aspect 4/3."""
    t = _draw(50, 10, 100, 1.0, 0.0)
    expect = torch.tensor([[0, (100 - 13) // 2, 10, 13, 1.0, 0.0]], dtype=torch.float32).expand(50, 6)
    assert torch.equal(t, expect)
    t = _draw(5, 100, 10, 1.0, 0.0)  # the tall case: full width, height from 3/4
    assert torch.equal(t[0], torch.tensor([(100 - 13) // 2, 0, 13, 10, 1.0, 0.0]))


def test_sampler_is_deterministic_per_seed():
    a, b, c = _draw(64, 112, 112, 0.7, 15, seed=5), _draw(64, 112, 112, 0.7, 15, seed=5), _draw(64, 112, 112, 0.7, 15, seed=6)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert torch.equal(data.identity_augment_params(3, 9, 11), torch.tensor([[0, 0, 9, 11, 1.0, 0.0]] * 3))


class _Model(torch.nn.Module):
    """The attributes DeviceClipPipeline and DPTrainer read (the HIP models need a GPU; the pipeline's host side does not)."""

    def __init__(self):
        super().__init__()
        self.cnn_backbone = torch.nn.Sequential(torch.nn.Conv3d(3, 4, 1))
        self.add_on_layers = torch.nn.Sequential(torch.nn.Conv3d(4, 4, 1))
        self.occurrence_module = torch.nn.Sequential(torch.nn.Conv3d(4, 2, 1))
        self.prototype_vectors = torch.nn.Parameter(torch.rand(2, 4, 1, 1, 1))
        self.last_layer = torch.nn.Linear(2, 2, bias=False)
        self.num_classes, self.num_prototypes = 2, 2
        self.prototype_class_identity = torch.eye(2)


def test_from_config_reads_the_reference_data_keys():
    """The six reference configs' ``data`` sections (tests/golden/reference_data_configs.json: augmentation, rotation, crop ratio,
    normalize as src/configs/*.yml set them)."""
    cfgs = json.load(open(os.path.join(GOLDEN, "reference_data_configs.json")))
    assert len(cfgs) == 6
    for name, dc in cfgs.items():
        p = data.DeviceClipPipeline.from_config(_Model(), dc, seed=1)
        assert p.augment is bool(dc["augmentation"]) and p.augment, name
        assert p.rotate_degrees == float(dc["transform_rotate_degrees"]) == 15.0, name
        assert p.min_crop_ratio == float(dc["transform_min_crop_ratio"]) == 0.7, name
        assert p.normalize is bool(dc["normalize"]), name
    off = data.DeviceClipPipeline.from_config(_Model(), {"augmentation": False, "normalize": False}, seed=0)
    assert off.augment is False and off.normalize is False and off.min_crop_ratio == 1.0 and off.rotate_degrees == 0.0
    with pytest.raises(ValueError):
        data.DeviceClipPipeline(_Model(), min_crop_ratio=0.0)


def test_trainer_seeds_the_pipeline_by_seed_and_rank():
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG

    def table(rank, seed):
        cfg = {"abstain_class": False, "save_dir": "", "train": dict(TRAIN_CFG, seed=seed),
               "data": {"augmentation": True, "transform_rotate_degrees": 15, "transform_min_crop_ratio": 0.7, "normalize": True}}
        t = DPTrainer(_Model(), cfg, {}, rank=rank, world_size=1, log=lambda *_: None)
        p = t.clip_pipeline()
        assert p is t.clip_pipeline() and p.augment
        return data.sample_augment_params(16, 112, 112, p.min_crop_ratio, p.rotate_degrees, p.generator)

    assert torch.equal(table(0, 3), table(0, 3))      # a rerun draws the same crops
    assert not torch.equal(table(0, 3), table(1, 3))  # ranks draw different ones
    assert not torch.equal(table(0, 3), table(0, 4))


def test_clip_augment_symbol_is_declared_and_exported():
    text = open(os.path.join(REPO, "include", "protoasnet_amd.h")).read()
    assert re.search(r"int pasn_clip_augment\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "pasn_clip_augment" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "pasn_clip_augment")
    assert _lib.I32 == 3 and "PASN_I32 = 3" in text
