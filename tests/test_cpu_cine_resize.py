"""CPU: the host side of the device clip resize -- band tables against the scipy restatement of skimage's resize, and the ragged
collate of raw cine windows (``data.collate_raw_cines`` / ``RawCineBatch``)."""
import numpy as np
import pytest
import torch

from protoasnet_amd import data, resample
from resize_cases import SHAPE_CASES, pattern, skimage_resize


def _apply(mats, x):
    for axis, m in enumerate(mats):
        x = np.moveaxis(np.tensordot(m, x, axes=([1], [axis])), 0, axis)
    return x


def _dense(n_in, n_out):
    start, w = resample.axis_bands(n_in, n_out)
    m = np.zeros((n_out, n_in))
    np.put_along_axis(m, start[:, None].astype(np.int64) + np.arange(w.shape[1])[None, :], w.astype(np.float64), axis=1)
    return m


@pytest.mark.parametrize("si,so", SHAPE_CASES, ids=[f"{a}->{b}" for a, b in SHAPE_CASES])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_band_tensor_product_equals_restatement(si, so, dtype):
    """The float64 axis operators, applied as a tensor product, equal scipy's 3-D filter + zoom to 1e-12; the fp32 tables they are
    rounded to stay within fp32 rounding of them."""
    x = pattern(si, dtype, seed=sum(si))
    ref = skimage_resize(x, so)
    xf = x.astype(np.float64) / (255.0 if dtype == np.uint8 else 1.0)
    assert np.abs(_apply([resample.axis_matrix(a, b) for a, b in zip(si, so)], xf) - ref).max() <= 1e-12
    assert np.abs(_apply([_dense(a, b) for a, b in zip(si, so)], xf) - ref).max() <= 1e-6
    assert np.array_equal(resample.apply_bands(x, so), _apply([_dense(a, b) for a, b in zip(si, so)], xf))


@pytest.mark.parametrize("n_in,n_out", [(600, 112), (800, 112), (1080, 112), (1440, 112), (600, 224), (800, 224), (40, 32), (24, 16),
                                        (12, 32), (1, 1), (1, 7), (9, 1), (3, 1), (5, 5)])
def test_band_rows_are_nonnegative_and_sum_to_one(n_in, n_out):
    start, w = resample.axis_bands(n_in, n_out)
    m = resample.axis_matrix(n_in, n_out)
    assert start.dtype == np.int32 and w.dtype == np.float32 and w.shape[0] == n_out
    assert (w >= 0).all() and (m >= 0).all()
    assert np.abs(m.sum(axis=1) - 1.0).max() <= 1e-12
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    assert (np.diff(start) >= 0).all() and start.min() >= 0 and (start + w.shape[1]).max() <= n_in
    assert np.abs(w.astype(np.float64) - np.take_along_axis(m, start[:, None] + np.arange(w.shape[1])[None, :], axis=1)).max() <= 6e-8
    assert resample.axis_bands(n_in, n_out) is resample.axis_bands(n_in, n_out)  # cached
    assert not w.flags.writeable


def test_band_spans_of_the_reference_shapes():
    assert resample.axis_bands(600, 112)[1].shape[1] == 20
    assert resample.axis_bands(800, 112)[1].shape[1] == 26
    assert resample.axis_bands(100, 112)[1].shape[1] == 2  # growing: the linear tent only


def test_pack_tables_layout():
    buf, off = resample.pack_tables([(600, 112), (40, 32), (600, 112)])
    assert list(off) == [(600, 112), (40, 32)]
    for (n_in, n_out), o in off.items():
        start, w = resample.axis_bands(n_in, n_out)
        assert list(buf[o:o + 3]) == [n_in, n_out, w.shape[1]]
        assert np.array_equal(buf[o + 3:o + 3 + n_out], start)
        assert np.array_equal(buf[o + 3 + n_out:o + 3 + n_out + w.size].view(np.float32), w.reshape(-1))


def _item(cine, s, e, name, label=0, **kw):
    return dict(cine=cine, window_start=s, window_end=e, filename=name, target_AS=label, **kw)


def test_collate_packs_ragged_windows_and_deduplicates_sources():
    a, b, c = pattern((12, 30, 40), seed=1), pattern((7, 20, 26), seed=2), pattern((5, 9, 11), seed=3)
    items = [_item(a, 2, 6, "a.mat", 1, interval_idx=0), _item(b, 0, 7, "b.mat", 2, interval_idx=0),
             _item(a, 5, 11, "a.mat", 1, interval_idx=1), _item(torch.from_numpy(c), 1, 2, "c.mat", 0, interval_idx=0)]
    batch = data.collate_raw_cines(items)
    raw = batch["cine"]
    assert isinstance(raw, data.RawCineBatch) and len(raw) == 4 and raw.dtype == torch.uint8
    # one copy of a.mat over frames [2, 11) (its two windows), b.mat whole, c.mat frame 1 only; each source 16-byte aligned
    sizes = [9 * 30 * 40, 7 * 20 * 26, 1 * 9 * 11]
    offs = [0, (sizes[0] + 15) // 16 * 16]
    offs.append(offs[1] + (sizes[1] + 15) // 16 * 16)
    assert raw.buffer.numel() == offs[2] + (sizes[2] + 15) // 16 * 16
    assert raw.windows.tolist() == [[offs[0], 0, 4, 30, 40], [offs[1], 0, 7, 20, 26], [offs[0], 3, 6, 30, 40], [offs[2], 0, 1, 9, 11]]
    for i, (src, s, e) in enumerate([(a, 2, 6), (b, 0, 7), (a, 5, 11), (c, 1, 2)]):
        assert np.array_equal(raw.window(i).numpy(), src[s:e])
    assert batch["filename"] == ["a.mat", "b.mat", "a.mat", "c.mat"]
    assert batch["target_AS"].tolist() == [1, 2, 1, 0] and batch["window_start"].tolist() == [2, 0, 5, 1]
    assert batch["interval_idx"].tolist() == [0, 0, 1, 0]


def test_collate_fp32_sources_and_items_without_filename():
    a = pattern((4, 10, 13), np.float32, seed=4)
    raw = data.collate_raw_cines([dict(cine=a, window_start=0, window_end=2, target_AS=0),
                                  dict(cine=a, window_start=1, window_end=4, target_AS=1)])["cine"]
    assert raw.dtype == torch.float32 and raw.buffer.dtype == torch.uint8
    assert raw.windows[0, 0] % 16 == 0 and raw.windows[1, 0] % 16 == 0 and raw.windows[0, 0] != raw.windows[1, 0]  # two sources
    assert np.array_equal(raw.window(1).numpy(), a[1:4])


def test_raw_batch_pin_memory_hook(monkeypatch):
    """``DataLoader(pin_memory=True)`` reaches ``RawCineBatch.pin_memory`` through the sample dict."""
    from torch.utils.data._utils.pin_memory import pin_memory

    pinned = []

    def fake_pin(self, *a, **k):
        c = self.clone()
        pinned.append(c)
        return c

    monkeypatch.setattr(torch.Tensor, "pin_memory", fake_pin)
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: any(self is p for p in pinned))
    batch = data.collate_raw_cines([_item(pattern((3, 8, 8)), 0, 2, "x")])
    out = pin_memory(batch)
    assert isinstance(out["cine"], data.RawCineBatch) and any(out["cine"].buffer is p for p in pinned) and out["cine"].is_pinned()
    assert out["cine"].pin_memory() is out["cine"]


def test_collate_refusals():
    u8 = pattern((4, 8, 8))
    with pytest.raises(ValueError, match="single-channel"):
        data.collate_raw_cines([_item(np.zeros((4, 8, 8, 3), np.uint8), 0, 2, "x")])
    with pytest.raises(ValueError, match="single-channel"):
        data.collate_raw_cines([_item(np.zeros((1, 3, 4, 8, 8), np.uint8), 0, 2, "x")])
    with pytest.raises(TypeError, match="uint8 or float32"):
        data.collate_raw_cines([_item(u8.astype(np.int16), 0, 2, "x")])
    with pytest.raises(TypeError, match="uint8 or float32"):
        data.collate_raw_cines([_item(u8.astype(np.float64), 0, 2, "x")])
    for s, e in ((2, 2), (3, 1), (0, 5), (-1, 2)):
        with pytest.raises(ValueError, match="empty or out-of-range window"):
            data.collate_raw_cines([_item(u8, s, e, "x")])
    with pytest.raises(TypeError, match="one source dtype"):
        data.collate_raw_cines([_item(u8, 0, 2, "x"), _item(u8.astype(np.float32), 0, 2, "y")])
    with pytest.raises(ValueError, match="differ in shape"):
        data.collate_raw_cines([_item(u8, 0, 2, "x"), _item(pattern((4, 8, 9)), 0, 2, "x")])
    with pytest.raises(ValueError, match="empty batch"):
        data.collate_raw_cines([])


def test_pipeline_from_config_reads_the_output_shape():
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.features = torch.nn.Linear(1, 1)

    p = data.DeviceClipPipeline.from_config(M(), {"frames": 32, "img_size": 112, "normalize": True})
    assert (p.frames, p.img_size) == (32, 112)
    q = data.DeviceClipPipeline.from_config(M(), {})
    with pytest.raises(ValueError, match="output shape"):
        q.resize(data.collate_raw_cines([_item(pattern((3, 8, 8)), 0, 2, "x")])["cine"])


def test_launch_geometry_covers_every_tile():
    """tmp_rows / raw_pitch bound every tile's band unions, and the tile fits the instance's pixels per block."""
    windows = np.array([[0, 0, 40, 600, 800], [0, 0, 12, 100, 90], [0, 0, 60, 1080, 1440]])
    tile_h, tile_w, tmp_rows, raw_pitch, chunk_rows, band_floats = resample.launch_geometry(windows, (32, 112, 112), 1, 512)
    assert tile_h * tile_w <= 512 and raw_pitch % 16 == 0 and chunk_rows >= 1
    for h0, w0 in ((600, 800), (100, 90), (1080, 1440)):
        sh, wh = resample.axis_bands(h0, 112)
        sw, ww = resample.axis_bands(w0, 112)
        for t in range(0, 112, tile_h):
            e = min(t + tile_h, 112) - 1
            assert sh[e] + wh.shape[1] - sh[t] <= tmp_rows
        assert sw[-1] + ww.shape[1] - sw[0] + 15 <= raw_pitch
        assert tile_w * (ww.shape[1] + 1) + tile_h * (wh.shape[1] + 1) <= band_floats
