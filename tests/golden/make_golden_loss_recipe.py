#!/usr/bin/env python3
"""Golden fixture of the WHOLE loss recipe (tests/golden/g11_loss_recipe.npz): the reference's loss classes (src/loss/loss.py) applied as
its training loop applies them (Video_XProtoNet_e2e.py:86-110), produced by RUNNING THE REFERENCE on the CPU in the build container, at
the weights of its two video configs and at the settings g6_losses.npz does not reach at this size (tests/proto_loss_cases.py).  The
reference module is imported the way make_golden_losses.py imports it (placeholder torchvision modules; only classes that never touch
it run).  Nothing of the reference is copied: inputs come from the seeded generators of proto_loss_cases.py (the tests regenerate
them), only the terms, their sum and the gradients are stored.  A bf16 map enters the reference as the same values in fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_loss_recipe.py <reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["PASN_REFERENCE"]  # a reference checkout
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

for name in ("torchvision", "torchvision.ops", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.models"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision.ops"].sigmoid_focal_loss = None
sys.modules["torchvision.transforms.functional"].affine = None
sys.modules["torchvision.transforms.functional"].InterpolationMode = types.SimpleNamespace(BILINEAR="bilinear")

from src.loss import loss as ref  # noqa: E402  (reference)

sys.path.insert(0, os.path.join(REPO, "tests"))
from proto_loss_cases import CASES, OUTPUTS, build_losses, eager_terms, make_inputs  # noqa: E402  (shared with tests/test_gpu_proto_loss.py)


def main():
    out = {}
    for case in CASES:
        tag = case[0]
        t = make_inputs(tag)
        leaves = {k: t[k].float().clone().requires_grad_() for k in OUTPUTS}
        terms = eager_terms(build_losses(ref, tag), dict(t, **leaves))
        total = sum(terms)
        total.backward()
        out[tag + "_loss"] = total.detach().numpy()
        out[tag + "_terms"] = np.array([float(x.detach()) for x in terms], dtype=np.float32)
        for k, leaf in leaves.items():
            out[f"{tag}_grad_{k}"] = (torch.zeros_like(leaf) if leaf.grad is None else leaf.grad).numpy()
    path = os.path.join(HERE, "g11_loss_recipe.npz")
    np.savez_compressed(path, **out)
    print(f"g11_loss_recipe.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(CASES)} cases")


if __name__ == "__main__":
    main()
