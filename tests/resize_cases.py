"""The test oracle of the clip resize: scikit-image >= 0.19's ``resize(window, (T, H, W))`` with its defaults, restated on scipy.ndimage
(skimage/transform/_warps.py: ``convert_to_float``, ``gaussian_filter(mode='mirror')`` when an axis shrinks,
``zoom(order=1, mode='mirror', grid_mode=True)``, ``_clip_warp_output``).  scipy is imported where it is used, so GPU tests can
import the shared shapes without it."""
from __future__ import annotations

import numpy as np

# (window shape, output shape): shrinking, growing, mixed, degenerate, and a Gaussian radius longer than the axis
SHAPE_CASES = [
    ((10, 60, 80), (4, 16, 16)),       # shrink everywhere
    ((6, 20, 24), (16, 20, 24)),       # grow in T only (equal H, W: no filter on them)
    ((12, 30, 20), (5, 40, 11)),       # mixed
    ((1, 50, 70), (1, 17, 23)),        # image window (T_w = 1)
    ((3, 9, 7), (1, 1, 2)),            # radius > axis length: mirror folding more than once
    ((20, 13, 11), (3, 5, 4)),
    ((4, 5, 6), (7, 11, 13)),          # grow everywhere
    ((2, 31, 33), (1, 8, 8)),
    ((7, 1, 9), (3, 4, 2)),            # a length-1 axis
    ((40, 60, 80), (32, 11, 11)),
]


def skimage_resize(window: np.ndarray, shape) -> np.ndarray:
    """float64 ``skimage.transform.resize(window, shape)`` (>= 0.19, defaults) on scipy.ndimage."""
    from scipy import ndimage

    x = np.asarray(window)
    if x.dtype == np.uint8:
        x = x.astype(np.float64) / 255.0
    elif x.dtype in (np.float32, np.float64):
        x = x.astype(np.float64)
    else:
        raise TypeError(f"unsupported dtype {x.dtype}")
    factors = np.divide(x.shape, shape)
    if np.any(factors > 1):  # anti_aliasing defaults on when any axis shrinks
        sigma = np.maximum(0, (factors - 1) / 2)
        x = ndimage.gaussian_filter(x, sigma, cval=0.0, mode="mirror")
    y = ndimage.zoom(x, 1.0 / factors, order=1, mode="mirror", cval=0.0, grid_mode=True)
    return np.clip(y, x.min(), x.max()) if x.size else y


def pattern(shape, dtype=np.uint8, seed: int = 0) -> np.ndarray:
    """A smooth synthetic echo-like window plus noise."""
    rng = np.random.default_rng(seed)
    t, h, w = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    v = 0.5 + 0.3 * np.sin(6.0 * h + 2.0 * t) * np.cos(5.0 * w - 3.0 * t) + 0.1 * rng.standard_normal(shape)
    v = np.clip(v, 0.0, 1.0)
    return np.round(v * 255.0).astype(np.uint8) if dtype == np.uint8 else v.astype(np.float32)
