"""GPU: ``pasn_clip_augment`` (crop + bilinear resize, rotation, normalisation of a grey clip in one launch) against a torch restatement of
torchvision 0.14's formulas, written here: ``F.interpolate(bilinear, align_corners=False)`` of the crop, then ``F.rotate``'s
``_get_inverse_affine_matrix(centre, -angle)`` + ``_gen_affine_grid`` + ``grid_sample(mode="nearest", padding_mode="zeros")``, then
``(v - mean) / std``.  Pixels whose nearest source index flips when the sampling coordinates move by +-1e-4 px are excluded (two exact
implementations may round those either way); every other pixel must agree to fp32 / bf16 rounding."""
import math

import pytest
import torch
import torch.nn.functional as F

from protoasnet_amd import _lib
from protoasnet_amd.data import ECHO_MEAN, ECHO_STD

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table(rows):
    return torch.tensor([[i, j, h, w, math.cos(math.radians(a)), math.sin(math.radians(a))] for i, j, h, w, a in rows], dtype=torch.float32)


def _launch(x, params, out_dtype, normalize=True, param_dtype=torch.float32):
    """x (N,1,T,H,W) or (N,1,H,W) on the GPU; params (N,6) fp32 on the host."""
    n, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    T = x.shape[2] if x.dim() == 5 else 1
    y = torch.empty(x.shape, dtype=out_dtype, device=DEV)
    if param_dtype == torch.int32:  # crop as int32, cos / sin as their fp32 bit patterns
        p = params[:, :4].to(torch.int32)
        p = torch.cat([p, params[:, 4:].contiguous().view(torch.int32)], dim=1).contiguous().to(DEV)
    else:
        p = params.contiguous().to(DEV)
    mean, std = (ECHO_MEAN, ECHO_STD) if normalize else (0.0, 1.0)
    scale = 1.0 / 255.0 if x.dtype == torch.uint8 else 1.0
    _lib.check(_lib.lib().pasn_clip_augment(x.data_ptr(), y.data_ptr(), p.data_ptr(), n, T, H, W, H, W, scale, mean, std,
                                            _lib.dtype_code(x.dtype), _lib.dtype_code(out_dtype),
                                            _lib.I32 if param_dtype == torch.int32 else _lib.F32, _lib.current_stream()))
    torch.cuda.synchronize()
    return y


def _rotate_nearest(img, cos_t, sin_t, nudge=0.0):
    """torchvision 0.14 F.rotate(img, angle, NEAREST, expand=False, fill=0) on (B,1,H,W) float64, the sampling grid moved by `nudge` px."""
    _, _, h, w = img.shape
    # _get_inverse_affine_matrix(center=[0, 0], angle=-angle, translate=0, scale=1, shear=0): rot = -angle
    # a = cos(rot), b = -sin(rot), c = sin(rot), d = cos(rot); inverted matrix = [d, -b, 0, -c, a, 0]
    theta = torch.tensor([[[cos_t, -sin_t, 0.0], [sin_t, cos_t, 0.0]]], dtype=torch.float64)
    # _gen_affine_grid(theta, w, h, ow=w, oh=h)
    base = torch.empty(1, h, w, 3, dtype=torch.float64)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + 0.5, w * 0.5 + 0.5 - 1, steps=w, dtype=torch.float64))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + 0.5, h * 0.5 + 0.5 - 1, steps=h, dtype=torch.float64).unsqueeze(-1))
    base[..., 2].fill_(1)
    grid = base.view(1, h * w, 3).bmm(theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float64))
    grid = grid.view(1, h, w, 2) + torch.tensor([2.0 * nudge / w, 2.0 * nudge / h], dtype=torch.float64)
    return F.grid_sample(img, grid.expand(img.shape[0], h, w, 2), mode="nearest", padding_mode="zeros", align_corners=False)


def _reference(x, params, normalize=True):
    """The restatement, plus the mask of pixels whose nearest source index is unambiguous.  x on the host, (N,1,T,H,W) or (N,1,H,W)."""
    video = x.dim() == 5
    xv = x if video else x.unsqueeze(2)
    n, _, T, H, W = xv.shape
    # in float64, as the reference's dataset holds its clip (skimage resize -> torch.tensor of float64)
    xf = xv.double() / 255.0 if x.dtype == torch.uint8 else xv.double()
    mean, std = (ECHO_MEAN, ECHO_STD) if normalize else (0.0, 1.0)
    outs, masks = [], []
    ramp = torch.arange(1, H * W + 1, dtype=torch.float64).view(1, 1, H, W)  # source index + 1 of every resized pixel (0: outside)
    for k in range(n):
        i, j, h, w = (int(v) for v in params[k, :4])
        c, s = float(params[k, 4]), float(params[k, 5])
        crop = xf[k, 0, :, i:i + h, j:j + w].unsqueeze(1)                            # (T,1,h,w)
        res = F.interpolate(crop, size=(H, W), mode="bilinear", align_corners=False)  # (T,1,H,W)
        rot = _rotate_nearest(res, c, s)
        outs.append(((rot - mean) / std).squeeze(1))
        lo, hi = _rotate_nearest(ramp, c, s, -1e-4), _rotate_nearest(ramp, c, s, 1e-4)
        masks.append((lo == hi).view(1, H, W).expand(T, H, W))
    out, mask = torch.stack(outs).unsqueeze(1), torch.stack(masks).unsqueeze(1)
    return (out, mask) if video else (out[:, :, 0], mask[:, :, 0])


def _normalised(x):
    """(x * scale - mean) / std in fp32, each operation rounded once (tensor operands: torch turns a division by a Python scalar on the
    GPU into a multiplication by its reciprocal)."""
    xf = x.float()
    full = lambda v: torch.full_like(xf, v)  # noqa: E731
    if x.dtype == torch.uint8:
        xf = xf * full(1.0 / 255.0)
    return (xf - full(ECHO_MEAN)) / full(ECHO_STD)


def _clip(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.rand(shape, generator=g).to(dtype)


def _compare(y, ref, mask, out_dtype):
    y, ref = y.double().cpu(), ref.double()
    assert float(mask.float().mean()) > 0.97, "too many ambiguous pixels: the restatement, not the kernel, is off"
    if out_dtype == torch.float32:
        bad = ((y - ref).abs() > 1e-5 * (1 + ref.abs())) & mask
    else:
        bad = ((y - ref).abs() > 2.0 ** -8 * ref.abs() + 1e-5) & mask  # within bf16 rounding of the exact value
    assert not bool(bad.any()), f"{int(bad.sum())} pixels differ; worst {float(((y - ref).abs() * mask).max()):.3g}"


CROPS = [(0, 0, None, None, 15.0), (3, 5, 20, 30, -15.0), (7, 1, 25, 41, 7.3), (1, 9, 31, 17, -7.3)]


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(4, 1, 3, 37, 53), (4, 1, 1, 48, 40), (4, 1, 37, 53)], ids=["video_37x53", "t1", "image_4d"])
def test_clip_augment_matches_the_torchvision_restatement(in_dtype, out_dtype, shape):
    H, W = shape[-2], shape[-1]
    rows = [(i, j, min(h or H, H), min(w or W, W), a) for i, j, h, w, a in CROPS]
    rows = [(min(i, H - h), min(j, W - w), h, w, a) for i, j, h, w, a in rows]
    params = _table(rows)
    x = _clip(shape, in_dtype)
    y = _launch(x.to(DEV), params, out_dtype)
    ref, mask = _reference(x, params)
    _compare(y, ref, mask, out_dtype)


def test_clip_augment_int32_table_and_unnormalised_output():
    x = _clip((3, 1, 4, 40, 44), torch.uint8, seed=2)
    params = _table([(2, 3, 30, 35, 12.0), (0, 0, 40, 44, -3.0), (10, 0, 28, 44, 0.0)])
    y32 = _launch(x.to(DEV), params, torch.float32, normalize=False, param_dtype=torch.int32)
    yf = _launch(x.to(DEV), params, torch.float32, normalize=False)
    assert torch.equal(y32, yf)
    ref, mask = _reference(x, params, normalize=False)
    _compare(yf, ref, mask, torch.float32)


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_identity_parameters_are_plain_normalisation_bit_for_bit(in_dtype, out_dtype):
    x = _clip((3, 1, 5, 33, 47), in_dtype, seed=1).to(DEV)
    params = torch.tensor([[0, 0, 33, 47, 1.0, 0.0]] * 3, dtype=torch.float32)
    y = _launch(x, params, out_dtype)
    assert torch.equal(y, _normalised(x).to(out_dtype))


@pytest.mark.parametrize("size", [48, 37])
def test_ninety_degrees_is_rot90(size):
    """rotate(+90) of the full crop is torch.rot90(k=1): pins the sign of the angle, which a restatement could share with the kernel
    (torchvision's rotate() negates the angle that affine() takes)."""
    x = _clip((2, 1, 3, size, size), torch.float32, seed=4).to(DEV)
    params = _table([(0, 0, size, size, 90.0)] * 2)
    y = _launch(x, params, torch.float32)
    assert torch.equal(y, torch.rot90(_normalised(x), k=1, dims=(-2, -1)))


def test_clip_augment_repeats_bit_for_bit():
    x = _clip((8, 1, 16, 112, 112), torch.uint8, seed=7).to(DEV)
    params = _table([(k, 2 * k, 112 - 3 * k, 100 - k, (-1) ** k * 1.7 * k) for k in range(8)])
    first = _launch(x, params, torch.bfloat16)
    for _ in range(25):
        assert torch.equal(_launch(x, params, torch.bfloat16), first)


def test_clip_augment_rejects_bad_arguments():
    x = torch.zeros(1, 1, 2, 8, 8, device=DEV)
    y = torch.empty_like(x)
    p = torch.zeros(1, 6, device=DEV)
    lib = _lib.lib()
    with pytest.raises(ValueError):
        _lib.check(lib.pasn_clip_augment(x.data_ptr(), y.data_ptr(), p.data_ptr(), 1, 2, 8, 8, 8, 8, 1.0, 0.0, 0.0, 0, 0, 0, _lib.current_stream()))
    with pytest.raises(ValueError):
        _lib.check(lib.pasn_clip_augment(x.data_ptr(), y.data_ptr(), p.data_ptr(), 1, 2, 8, 8, 8, 8, 1.0, 0.0, 1.0, 0, 2, 0, _lib.current_stream()))
