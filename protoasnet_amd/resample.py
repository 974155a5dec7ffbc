"""Host band tables of the reference's clip resize (``skimage.transform.resize(window, (T, H, W))``, as_dataloader.py:204-207).

scikit-image >= 0.19 with its defaults (order=1, mode='reflect', anti_aliasing on when an axis shrinks, clip=True,
preserve_range=False) computes, on the window converted to float (uint8 / 255):

    f = n_in / n_out per axis,  sigma = max(0, (f - 1) / 2)
    scipy.ndimage.gaussian_filter(x, sigma, mode='mirror', truncate=4.0)   (only if an axis shrinks; radius int(4 sigma + 0.5))
    scipy.ndimage.zoom(., 1 / f, order=1, mode='mirror', grid_mode=True)   (source coordinate (o + 0.5) f - 0.5)
    clip to the input's range

Both steps are separable and linear, so the whole operator is ``A_T (x) A_H (x) A_W`` applied to the window.  Each ``A_axis`` is a
banded, non-negative matrix whose rows sum to 1 (the final clip is a no-op).  ``axis_bands`` builds it in float64 from the
definitions above (Gaussian taps with mirror index folding, composed with the linear tent) and rounds it to fp32 once; the device
kernel (``pasn_cine_resize``, csrc/cine_resize.hip) applies the three tables.  No scipy at run time.
"""
from __future__ import annotations

import functools
from typing import Dict, Iterable, Tuple

import numpy as np


def _mirror(idx: np.ndarray, n: int) -> np.ndarray:
    """scipy.ndimage 'mirror' extension (d c b | a b c d | c b a), folded as often as needed."""
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    k = np.mod(idx, period)
    return np.where(k < n, k, period - k)


def axis_matrix(n_in: int, n_out: int, antialias: bool = True) -> np.ndarray:
    """The dense float64 (n_out, n_in) operator of one axis."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"axis lengths must be positive, got {n_in} -> {n_out}")
    f = n_in / n_out
    sigma = max(0.0, (f - 1.0) / 2.0) if antialias else 0.0
    gauss = np.eye(n_in)
    if sigma > 0.0:  # gaussian_filter1d: taps exp(-x^2 / 2 sigma^2) / sum, radius int(truncate * sigma + 0.5)
        radius = int(4.0 * sigma + 0.5)
        x = np.arange(-radius, radius + 1)
        taps = np.exp(-0.5 / (sigma * sigma) * x.astype(np.float64) ** 2)
        taps /= taps.sum()
        gauss = np.zeros((n_in, n_in))
        rows = np.arange(n_in)[:, None]
        np.add.at(gauss, (np.broadcast_to(rows, (n_in, x.size)), _mirror(rows + x[None, :], n_in)), np.broadcast_to(taps, (n_in, x.size)))
    # zoom, order 1, grid_mode: the linear tent at (o + 0.5) f - 0.5 on the mirrored signal
    c = (np.arange(n_out) + 0.5) * f - 0.5
    i0 = np.floor(c).astype(np.int64)
    w1 = c - i0
    tent = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(tent, (o, _mirror(i0, n_in)), 1.0 - w1)
    np.add.at(tent, (o, _mirror(i0 + 1, n_in)), w1)
    return tent @ gauss


@functools.lru_cache(maxsize=256)
def axis_bands(n_in: int, n_out: int, antialias: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """``(start int32[n_out], weights fp32[n_out, S])``: row o of the axis operator is ``weights[o]`` on input indices
    ``start[o] .. start[o] + S - 1`` (S, the widest row's span, is shared; the narrower rows are zero-padded).  Cached per
    ``(n_in, n_out, antialias)``; the arrays are read-only."""
    m = axis_matrix(int(n_in), int(n_out), bool(antialias))
    nz = m != 0.0
    first = nz.argmax(axis=1)
    last = n_in - 1 - nz[:, ::-1].argmax(axis=1)
    span = int((last - first + 1).max())
    start = np.minimum(first, n_in - span).astype(np.int32)  # a band never reaches past the axis
    assert np.all(np.diff(start) >= 0), "band starts must be non-decreasing (the kernel's tile unions rely on it)"
    idx = start[:, None].astype(np.int64) + np.arange(span)[None, :]
    weights = np.take_along_axis(m, idx, axis=1).astype(np.float32)
    start.setflags(write=False)
    weights.setflags(write=False)
    return start, weights


def apply_bands(window: np.ndarray, shape: Tuple[int, ...], antialias: bool = True) -> np.ndarray:
    """The fp32 band tables applied to a (T_w, H0, W0) window in float64 (uint8 scaled by 1/255): what the kernel computes, up to
    its fp32 accumulation."""
    x = np.asarray(window)
    x = x.astype(np.float64) / 255.0 if x.dtype == np.uint8 else x.astype(np.float64)
    for axis, n_out in enumerate(shape):
        start, w = axis_bands(x.shape[axis], n_out, antialias)
        dense = np.zeros((n_out, x.shape[axis]))
        np.put_along_axis(dense, start[:, None].astype(np.int64) + np.arange(w.shape[1])[None, :], w.astype(np.float64), axis=1)
        x = np.moveaxis(np.tensordot(dense, x, axes=([1], [axis])), 0, axis)
    return x


def pack_tables(keys: Iterable[Tuple[int, int]], antialias: bool = True) -> Tuple[np.ndarray, Dict[Tuple[int, int], int]]:
    """The band tables of ``keys`` ((n_in, n_out) pairs) in one int32 buffer, and each key's offset in it (in int32 units):
    ``n_in, n_out, S, start[n_out], weights[n_out * S]`` (fp32 bit patterns)."""
    parts, offsets, at = [], {}, 0
    for key in dict.fromkeys(keys):
        start, w = axis_bands(key[0], key[1], antialias)
        block = np.concatenate([np.array([key[0], key[1], w.shape[1]], np.int32), start, w.reshape(-1).view(np.int32)])
        offsets[key] = at
        parts.append(block)
        at += block.size
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


# ---- the launch over a ragged batch (data.RawCineBatch) ------------------------------------------------------------------------------
_RAW_BUDGET = 32 * 1024   # LDS bytes of staged input rows per workgroup
_TMP_BUDGET = 96 * 1024   # LDS bytes of W-pass rows per workgroup
_device_tables: Dict[tuple, tuple] = {}  # (device, keys) -> (int32 device tensor, offsets)
_in_flight: list = []     # (pinned descriptor table, event of its upload)


def _tables_on(device, keys) -> Tuple["object", Dict[Tuple[int, int], int]]:
    import torch

    key = (str(device), tuple(sorted(set(keys))))
    if key not in _device_tables:
        if len(_device_tables) > 64:
            _device_tables.clear()
        buf, offsets = pack_tables(key[1])
        _device_tables[key] = (torch.from_numpy(buf).to(device), offsets)
    return _device_tables[key]


def _union_spans(n_in: int, n_out: int, tile: int) -> np.ndarray:
    """Input span (the union of the bands) of each tile of ``tile`` consecutive outputs."""
    start, w = axis_bands(n_in, n_out)
    lo = start[0::tile].astype(np.int64)
    hi = start[np.minimum(np.arange(tile - 1, n_out + tile - 1, tile), n_out - 1)].astype(np.int64) + w.shape[1]
    return hi - lo


def launch_geometry(windows: np.ndarray, shape: Tuple[int, int, int], elem_bytes: int, pixels_per_block: int) -> Tuple[int, ...]:
    """``(tile_h, tile_w, tmp_rows, raw_pitch, chunk_rows, band_floats)`` of a launch over clips of ``windows`` ((N, 5): offset, first,
    T_w, H0, W0)."""
    _, H, W = shape
    sizes = sorted({(int(h0), int(w0)) for h0, w0 in windows[:, 3:5]})
    tile_w = min(W, pixels_per_block)
    tile_h = max(1, min(H, pixels_per_block // tile_w))
    while True:
        tmp_rows = max(int(_union_spans(h0, H, tile_h).max()) for h0, _ in sizes)
        if tmp_rows * tile_w * 4 <= _TMP_BUDGET or tile_h == 1:
            break
        tile_h -= 1
    span = max(int(_union_spans(w0, W, tile_w).max()) for _, w0 in sizes) * elem_bytes
    raw_pitch = (span + 15 + 15) // 16 * 16
    chunk_rows = max(1, min(tmp_rows, _RAW_BUDGET // raw_pitch))
    s_h = max(axis_bands(h0, H)[1].shape[1] for h0, _ in sizes)
    s_w = max(axis_bands(w0, W)[1].shape[1] for _, w0 in sizes)
    return tile_h, tile_w, tmp_rows, raw_pitch, chunk_rows, tile_w * (s_w + 1) + tile_h * (s_h + 1)


def resize_raw(batch, shape: Tuple[int, int, int], out_dtype, mean: float = 0.0, std: float = 1.0):
    """``pasn_cine_resize`` over a ``data.RawCineBatch`` already on the device: (N, T, H, W) in ``out_dtype``, ``(v - mean) / std`` of the
    resized window in [0, 1].  Waits on the batch's upload event (``batch.ready``) first."""
    import torch

    from . import _lib

    T, H, W = (int(s) for s in shape)
    if batch.buffer.device.type != "cuda":
        raise ValueError("resize_raw takes a RawCineBatch on the device (batch.to(device))")
    device = batch.buffer.device
    windows = batch.windows.numpy()
    n = windows.shape[0]
    keys = [(int(tw), T) for tw in windows[:, 2]] + [(int(h), H) for h in windows[:, 3]] + [(int(w), W) for w in windows[:, 4]]
    bands, offsets = _tables_on(device, keys)
    desc = np.zeros((n, 8), np.int64)
    desc[:, :5] = windows
    desc[:, 5] = [offsets[(int(tw), T)] for tw in windows[:, 2]]
    desc[:, 6] = [offsets[(int(h), H)] for h in windows[:, 3]]
    desc[:, 7] = [offsets[(int(w), W)] for w in windows[:, 4]]
    lib = _lib.lib()
    elem = 1 if batch.dtype == torch.uint8 else 4
    geo = launch_geometry(windows, (T, H, W), elem, lib.pasn_cine_resize_pixels_per_block(T))
    _in_flight[:] = [(b, e) for b, e in _in_flight if not e.query()]
    host = torch.from_numpy(desc).pin_memory()
    desc_dev = host.to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _in_flight.append((host, ev))
    if batch.ready is not None:
        torch.cuda.current_stream(device).wait_event(batch.ready)
    y = torch.empty((n, T, H, W), dtype=out_dtype, device=device)
    _lib.check(lib.pasn_cine_resize(batch.buffer.data_ptr(), batch.buffer.numel(), desc_dev.data_ptr(), bands.data_ptr(), bands.numel(),
                                    y.data_ptr(), n, T, H, W, *geo, float(mean), float(std), _lib.dtype_code(batch.dtype),
                                    _lib.dtype_code(out_dtype), _lib.current_stream()))
    return y
