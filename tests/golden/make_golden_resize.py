"""Writes g10_resize.npz: small raw windows and their reference resize, the fixture of the device resize (pasn_cine_resize).

The outputs are the float64 scipy.ndimage restatement of ``skimage.transform.resize(window, shape)`` (scikit-image >= 0.19 defaults,
tests/resize_cases.py).  Where scikit-image imports, the restatement is first asserted equal to it to 1e-12.

    python tests/golden/make_golden_resize.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from resize_cases import pattern, skimage_resize  # noqa: E402

# name -> (window shape, output shape, source dtype)
CASES = {
    "shrink": ((10, 60, 80), (4, 16, 16), np.uint8),
    "grow_t": ((6, 20, 24), (16, 20, 24), np.uint8),
    "mixed": ((12, 30, 20), (5, 40, 11), np.uint8),
    "image": ((1, 50, 70), (1, 17, 23), np.uint8),
    "radius": ((3, 9, 7), (1, 1, 2), np.uint8),
    "fp32": ((8, 40, 44), (16, 24, 24), np.float32),
}


def main():
    try:
        from skimage.transform import resize
    except ImportError:
        resize = None
    out = {}
    for i, (name, (si, so, dt)) in enumerate(CASES.items()):
        x = pattern(si, dt, seed=i)
        y = skimage_resize(x, so)
        if resize is not None:
            assert np.abs(resize(x, so) - y).max() <= 1e-12, name
        out[name + "_x"], out[name + "_y"] = x, y
    np.savez_compressed(os.path.join(HERE, "g10_resize.npz"), **out)
    print("wrote g10_resize.npz", "(checked against skimage)" if resize is not None else "(skimage not importable: restatement only)")


if __name__ == "__main__":
    main()
