#!/usr/bin/env python3
"""G8: golden fixtures of the local explanation, produced by RUNNING THE REFERENCE'S OWN HELPERS on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_explain.py

Runs only in the build container (needs the reference tree).  ``src/utils/explainability_utils.py`` is imported as it lies and its
``get_src``, ``get_normalized_upsample_occurence_maps``, ``get_heatmap`` and ``load_data_and_model_products`` are *called*; nothing of
them is copied here, only their numerical results are stored (``g8_explain.npz``).

What this image lacks and how the import still succeeds:

* ``cv2`` is absent: a placeholder module is registered whose ``applyColorMap(img, cmap)`` looks the uint8 image up in a seeded
  256 x 3 table (``lut_bgr``, stored).  The reference's own ``get_heatmap`` (divide by 255, flip BGR -> RGB) and its overlay
  expression ``src + 0.3 * heatmap`` (local_explainability.py:76, :104) then produce the expected overlays.
* ``src.data.as_dataloader`` pulls in the dataset stack; a placeholder with ``class_labels`` (all ``load_data_and_model_products``
  needs of it) is registered.  ``torchvision`` gets empty placeholders (the model files import it at module top).
* There is no GPU: ``Tensor.cuda`` is patched to identity.

Inputs are not stored: the occurrence maps and clips come from the seeded recipe ``case_inputs`` (restated in the tests), the
g2 model from ``protoasnet_amd.synth``.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PASN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

LUT_BGR = np.random.default_rng(8).integers(0, 256, size=(256, 3), dtype=np.uint8)


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)
    return sys.modules[name]


_tvm = _placeholder("torchvision.models")
_placeholder("torchvision", models=_tvm)
_placeholder("cv2", applyColorMap=lambda img, cmap: LUT_BGR[img], COLORMAP_TURBO=20)
_placeholder("src.data.as_dataloader", class_labels=["No AS", "Early AS", "Significant AS"])
torch.Tensor.cuda = lambda self, *a, **k: self

import src.utils.explainability_utils as ref_x  # noqa: E402  (reference)
from src.models.XProtoNet import construct_XProtoNet  # noqa: E402  (reference)

from protoasnet_amd import synth  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

# (name, occurrence-map grid (T', H', W') or (H', W'), clip grid, seed); two maps each (P = 2: the reference's .squeeze() keeps P)
CASES = [("video_int", (2, 4, 4), (8, 28, 28), 81), ("video_frac", (3, 5, 6), (7, 17, 23), 82), ("image", (5, 6), (37, 45), 83)]
P_MAPS = 2


def case_inputs(grid, out, seed):
    """(occ (P, 1, *grid) fp32 >= 0, src (P, 3, *out) fp32, the normalised clip) -- tests/test_*_explain.py restate this."""
    rng = np.random.default_rng(seed)
    occ = np.abs(rng.standard_normal((P_MAPS, 1) + tuple(grid))).astype(np.float32) * np.float32(3.0)
    grey = rng.random((P_MAPS, 1) + tuple(out), dtype=np.float32)
    src = np.repeat((grey - np.float32(0.099)) / np.float32(0.171), 3, axis=1)
    return occ, src


def g2_loader():
    batches = []
    for bi, (seed, labels) in enumerate(((11, [0, 1]), (12, [2, 1]))):
        batches.append({"cine": synth.echo_clips((2, 3, 224, 224), seed=seed), "target_AS": torch.tensor(labels),
                        "filename": [f"case{bi}_{a}" for a in range(2)]})
    return batches


DATA_CONFIG = dict(view="plax", frames=1, img_size=224, interval_quant=1.0, interval_unit="cycle", iterate_intervals=False)


def main():
    out = {"lut_bgr": LUT_BGR}
    for name, grid, size, seed in CASES:
        occ, src = case_inputs(grid, size, seed)
        imgs, upsampler = ref_x.get_src(src)
        maps = ref_x.get_normalized_upsample_occurence_maps(occ, upsampler)
        overlay = imgs + 0.3 * ref_x.get_heatmap(maps)
        out[f"{name}_maps"] = maps.astype(np.float32)
        out[f"{name}_overlays"] = overlay.astype(np.float32)
        print(name, maps.shape, maps.dtype, overlay.shape, overlay.dtype)

    m = construct_XProtoNet("resnet18", pretrained=False, img_size=224, prototype_shape=(40, 512, 1, 1), num_classes=4,
                            add_on_layers_type="regular")
    synth.load_synth(m)
    m.eval()
    with tempfile.TemporaryDirectory() as tmp:
        cfg = dict(DATA_CONFIG, dataset_root=os.path.join(tmp, "data"))
        data, products = ref_x.load_data_and_model_products(m, g2_loader(), "val", cfg, True, os.path.join(tmp, "run"), log=lambda *a: None)
    for tag, d in (("data", data), ("products", products)):
        keys = sorted(d)
        out[f"{tag}_keys"] = np.array(keys)
        out[f"{tag}_shapes"] = np.array([str(tuple(np.asarray(d[k]).shape)) for k in keys])
        out[f"{tag}_dtypes"] = np.array([str(np.asarray(d[k]).dtype) for k in keys])
        for k in keys:
            if k in ("protoL_input_", "inputs"):
                continue
            out[f"{tag}__{k}"] = np.asarray(d[k])
    path = os.path.join(HERE, "g8_explain.npz")
    np.savez_compressed(path, **out)
    print(f"g8_explain.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
