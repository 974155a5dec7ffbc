"""Device side of the input pipeline.

The reference's dataset does, per clip and on the host (``src/data/as_dataloader.py:184-231``): load the cine, resize to
(T, H, W) in [0, 1] (skimage), optional augmentation, ``bin_to_norm`` ((x - 0.099) / 0.171, :173-182), ``gray_to_gray3``
(expand to 3 identical channels, :168-170), ``.float()``.  The last three steps triple the bytes that cross PCIe and that the first
conv reads.  Here the clip stays SINGLE-channel (fp32, bf16 or uint8) until it is on the GPU: normalisation is fused into the first
layer's loads (``HipTrunk.set_input_normalization``) and the channel expansion is folded into the first conv's weights (summed over
the input channels: 9 spatial taps instead of 27 for the X3D stem) -- ``pasn_x3d_stem_gray_fwd`` / ``pasn_first_conv_gray_fwd``.

Training takes the grey clip too: ``DeviceClipPipeline.normalized`` runs the train split's augmentation (torchvision's
``RandomResizedCropVideo`` + the reference's ``RandomRotateVideo``, as_dataloader.py:127-133) and ``bin_to_norm`` in ONE launch
(``pasn_clip_augment``, csrc/augment.hip) on per-clip parameters drawn here, on the host, from a private generator
(``sample_augment_params``).

The reference's host resize (``skimage.transform.resize(cine[window_start:window_end], (frames, img_size, img_size))``,
as_dataloader.py:204-207) runs on the device too: a dataset returns the raw cine with its window, ``collate_raw_cines`` packs a batch
into a ``RawCineBatch`` (each distinct source, keyed by filename, stored once and only over the frames its windows cover) and
``DeviceClipPipeline`` resizes it in one ``pasn_cine_resize`` launch (csrc/cine_resize.hip; band tables in ``resample.py``) before the
normalisation / augmentation above.  Choosing the window (``transform_time_dilation``, ``compute_intervals``) and decoding the cine
stay in the user's dataset.

``bin_to_norm`` / ``gray_to_gray3`` keep the reference's names and semantics for code that still wants the 3-channel tensor.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib, resample

ECHO_MEAN, ECHO_STD = 0.099, 0.171  # as_dataloader.py:180-181


def gray_to_gray3(in_tensor: torch.Tensor) -> torch.Tensor:
    """1xTxHxW -> 3xTxHxW view (as_dataloader.py:166-170)."""
    return in_tensor.expand(3, *([-1] * (in_tensor.dim() - 1)))


def bin_to_norm(in_tensor: torch.Tensor) -> torch.Tensor:
    """[0, 1] pixels -> normalised (as_dataloader.py:172-182)."""
    return (in_tensor - ECHO_MEAN) / ECHO_STD


class GreyInputError(ValueError, NotImplementedError):
    """A grey clip the training pass (or ``DeviceClipPipeline.normalized``) refuses: uint8 pixels, or a clip that meets an input
    normalisation left on the trunk by someone else.  A ``ValueError``; also a ``NotImplementedError``, which is what every grey clip in
    train mode raised before the training pass accepted normalised ones, so callers that catch that keep catching these refusals."""


def sample_augment_params(n: int, height: int, width: int, min_crop_ratio: float, rotate_degrees: float,
                          generator: torch.Generator) -> torch.Tensor:
    """Per-clip parameters of ``pasn_clip_augment``: float32 (n, 6) rows {i, j, h, w, cos t, sin t}.

    The crop restates torchvision's ``RandomResizedCrop.get_params`` (scale (min_crop_ratio, 1), ratio (3/4, 4/3), log-uniform aspect,
    10 attempts, then the central-crop fallback); the angle is uniform in [-rotate_degrees, rotate_degrees] (video_transforms.py:26).
    Every draw comes from ``generator``, so a seed fixes the table."""
    area = height * width
    log_ratio = (math.log(3.0 / 4.0), math.log(4.0 / 3.0))
    rows = []
    for _ in range(n):
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(min_crop_ratio, 1.0, generator=generator).item()
            aspect = math.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator).item())
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                i = int(torch.randint(0, height - h + 1, size=(1,), generator=generator).item())
                j = int(torch.randint(0, width - w + 1, size=(1,), generator=generator).item())
                break
        else:  # central crop at the nearest allowed aspect
            in_ratio = float(width) / float(height)
            if in_ratio < 3.0 / 4.0:
                w, h = width, int(round(width / (3.0 / 4.0)))
            elif in_ratio > 4.0 / 3.0:
                h, w = height, int(round(height * (4.0 / 3.0)))
            else:
                w, h = width, height
            i, j = (height - h) // 2, (width - w) // 2
        angle = torch.empty(1).uniform_(-float(rotate_degrees), float(rotate_degrees), generator=generator).item() if rotate_degrees else 0.0
        t = math.radians(angle)
        rows.append((i, j, h, w, math.cos(t), math.sin(t)))
    return torch.tensor(rows, dtype=torch.float32).reshape(n, 6)


def identity_augment_params(n: int, height: int, width: int) -> torch.Tensor:
    """The table under which ``pasn_clip_augment`` is plain normalisation: full crop, no rotation."""
    return torch.tensor([[0, 0, height, width, 1.0, 0.0]], dtype=torch.float32).repeat(n, 1)


class RawCineBatch:
    """A ragged batch of raw cine windows on the host or the device: what ``collate_raw_cines`` builds and ``DeviceClipPipeline`` resizes.

    ``buffer``: the sources as one flat uint8 tensor (each source C-contiguous (frames, H0, W0) in ``dtype``, uint8 or float32, at a
    16-byte aligned offset; the length a multiple of 16).  ``windows``: int64 (N, 5) host tensor, per clip {byte offset of its source,
    first frame of the window inside the stored frames, T_w, H0, W0}.  ``ready``: the event of an asynchronous upload to wait on before
    reading ``buffer`` (set by whoever issued the copy on another stream), or None."""

    def __init__(self, buffer: torch.Tensor, windows: torch.Tensor, dtype: torch.dtype, ready=None):
        if buffer.dtype != torch.uint8 or buffer.dim() != 1 or buffer.numel() % 16:
            raise ValueError("RawCineBatch.buffer is a flat uint8 tensor whose length is a multiple of 16")
        if windows.dtype != torch.int64 or windows.dim() != 2 or windows.shape[1] != 5 or windows.device.type != "cpu":
            raise ValueError("RawCineBatch.windows is an int64 (N, 5) host tensor")
        if dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"raw cines are uint8 or float32, not {dtype}")
        self.buffer, self.windows, self.dtype, self.ready = buffer, windows, dtype, ready

    def __len__(self) -> int:
        return int(self.windows.shape[0])

    @property
    def device(self) -> torch.device:
        return self.buffer.device

    def is_pinned(self) -> bool:
        return self.buffer.is_pinned()

    def pin_memory(self, device=None) -> "RawCineBatch":
        """The batch with its buffer in page-locked memory (``DataLoader(pin_memory=True)`` calls this)."""
        return self if self.buffer.is_cuda or self.buffer.is_pinned() else RawCineBatch(self.buffer.pin_memory(), self.windows, self.dtype)

    def to(self, device, non_blocking: bool = False) -> "RawCineBatch":
        """The batch with its buffer on ``device`` (the window table stays on the host: the launch reads it there)."""
        return RawCineBatch(self.buffer.to(device, non_blocking=non_blocking), self.windows, self.dtype, self.ready)

    def window(self, i: int) -> torch.Tensor:
        """Clip ``i``'s raw window (T_w, H0, W0) as a view of the buffer (host or device)."""
        off, first, tw, h0, w0 = (int(v) for v in self.windows[i])
        es = 1 if self.dtype == torch.uint8 else 4
        start = off + first * h0 * w0 * es
        return self.buffer[start:start + tw * h0 * w0 * es].view(self.dtype).view(tw, h0, w0)


def _as_cine(cine, i: int) -> np.ndarray:
    a = cine.detach().cpu().numpy() if isinstance(cine, torch.Tensor) else np.asarray(cine)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"collate_raw_cines: item {i}'s cine has shape {tuple(a.shape)}; it takes the single-channel (T, H, W) cine "
                         "(a 3-channel clip is already resized: collate it with the default collate)")
    if a.dtype not in (np.uint8, np.float32):
        raise TypeError(f"collate_raw_cines: item {i}'s cine is {a.dtype}; raw cines are uint8 or float32")
    return a


def collate_raw_cines(items) -> dict:
    """``collate_fn`` for dataset items carrying the full single-channel ``cine`` (T x H0 x W0, uint8 or float32) with ``window_start`` /
    ``window_end`` (the frame window, end exclusive, as_dataloader.py:225-231) instead of the resized clip.

    ``batch["cine"]`` is a ``RawCineBatch``: one flat buffer in which each distinct source (keyed by ``filename``; an item without one is
    its own source) is stored ONCE, over the frame range its windows cover -- many intervals of one cine (``iterate_intervals``) cost one
    copy.  Every other key collates as ``default_collate`` does."""
    if not items:
        raise ValueError("collate_raw_cines: empty batch")
    sources, order, dtype = {}, [], None
    for i, it in enumerate(items):
        a = _as_cine(it["cine"], i)
        s, e = int(it["window_start"]), int(it["window_end"])
        if not 0 <= s < e <= a.shape[0]:
            raise ValueError(f"collate_raw_cines: item {i} has the empty or out-of-range window [{s}, {e}) of a {a.shape[0]}-frame cine")
        if dtype is None:
            dtype = a.dtype
        elif a.dtype != dtype:
            raise TypeError(f"collate_raw_cines: one batch holds one source dtype, got {dtype} and {a.dtype}")
        key = ("file", it["filename"]) if it.get("filename") is not None else ("item", i)
        if key in sources:
            src = sources[key]
            if src["cine"].shape != a.shape:
                raise ValueError(f"collate_raw_cines: two cines named {it['filename']!r} differ in shape: {src['cine'].shape} and {a.shape}")
            src["lo"], src["hi"] = min(src["lo"], s), max(src["hi"], e)
        else:
            sources[key] = {"cine": a, "lo": s, "hi": e}
        order.append((key, s, e))
    es = dtype.itemsize
    at = 0
    for src in sources.values():
        src["off"] = at
        at += (src["hi"] - src["lo"]) * src["cine"].shape[1] * src["cine"].shape[2] * es
        at = (at + 15) // 16 * 16
    buffer = torch.zeros(max(at, 16), dtype=torch.uint8)
    flat = buffer.numpy()
    for src in sources.values():
        part = np.ascontiguousarray(src["cine"][src["lo"]:src["hi"]]).reshape(-1).view(np.uint8)
        flat[src["off"]:src["off"] + part.size] = part
    windows = torch.tensor([[sources[k]["off"], s - sources[k]["lo"], e - s, *sources[k]["cine"].shape[1:]] for k, s, e in order],
                           dtype=torch.int64)
    rest = torch.utils.data.default_collate([{k: v for k, v in it.items() if k != "cine"} for it in items])
    rest["cine"] = RawCineBatch(buffer, windows, torch.uint8 if dtype == np.uint8 else torch.float32)
    return rest


class DeviceClipPipeline:
    """Batches of single-channel clips -> what ``model(x)`` takes, with the normalisation and channel expansion left to the GPU.

    ``pipe = DeviceClipPipeline(model, normalize=True)`` configures the model's trunk once; ``x = pipe(cine)`` takes a host or
    device batch shaped (N,T,H,W) / (N,1,T,H,W) (video) or (N,H,W) / (N,1,H,W) (image) in [0, 1] (float) or [0, 255] (uint8), moves
    it to the model's device asynchronously (one third of the reference's bytes, a twelfth for uint8) and returns the (N,1,...)
    tensor the HIP trunk accepts directly.  ``normalize=False``: the clip is already normalised.

    In train mode ``pipe(cine)`` returns ``normalized(cine, augment)``: the training pass takes a materialised, normalised clip
    (``augment=True`` draws a crop and an angle per clip: ``rotate_degrees``, ``min_crop_ratio``, from a generator seeded by ``seed``).

    ``cine`` may also be a ``RawCineBatch`` (``collate_raw_cines``): its windows are first resized to (``frames``, ``img_size``,
    ``img_size``) on the device (``pasn_cine_resize``; ``frames`` is 1 for an image model).  Eval: one launch to [0, 1] in the model's
    dtype, normalisation fused into the trunk as for clips.  Train without augmentation: one launch, normalised in its epilogue.  Train
    with augmentation: the resize, then ``pasn_clip_augment`` (the reference's order: resize, then crop / rotate).
    """

    def __init__(self, model: torch.nn.Module, normalize: bool = True, video: Optional[bool] = None, augment: bool = False,
                 rotate_degrees: float = 0.0, min_crop_ratio: float = 1.0, seed: int = 0, frames: Optional[int] = None,
                 img_size: Optional[int] = None):
        self.model = model
        self.trunk = getattr(model, "cnn_backbone", None) or getattr(model, "features")
        self.device = next(model.parameters()).device
        self.normalize = normalize
        self.video = type(model).__name__.startswith("Video") if video is None else bool(video)
        self.augment, self.rotate_degrees, self.min_crop_ratio = bool(augment), float(rotate_degrees), float(min_crop_ratio)
        if not 0.0 < self.min_crop_ratio <= 1.0:
            raise ValueError(f"min_crop_ratio must lie in (0, 1], not {min_crop_ratio}")
        self.generator = torch.Generator().manual_seed(int(seed))
        self._identity = {}      # (n, H, W) -> identity parameter table on the device
        self._affine = None      # the trunk's input normalisation as this pipeline last set it (None: never set)
        self._in_flight = []     # (pinned table, event of its upload): a pinned buffer lives until its copy has completed
        self.frames = None if frames is None else int(frames)        # output shape of a RawCineBatch's resize
        self.img_size = None if img_size is None else int(img_size)

    @classmethod
    def from_config(cls, model: torch.nn.Module, data_cfg: dict, seed: int = 0) -> "DeviceClipPipeline":
        """The reference's ``data`` keys (src/configs/*.yml): ``augmentation``, ``transform_rotate_degrees``, ``transform_min_crop_ratio``,
        ``normalize``, and ``frames`` / ``img_size`` (the resize of raw batches).  ``transform_time_dilation`` is the dataset's (it picks
        the frame window)."""
        return cls(model, normalize=bool(data_cfg.get("normalize", True)), augment=bool(data_cfg.get("augmentation", False)),
                   rotate_degrees=float(data_cfg.get("transform_rotate_degrees", 0.0) or 0.0),
                   min_crop_ratio=float(data_cfg.get("transform_min_crop_ratio", 1.0) or 1.0), seed=seed,
                   frames=data_cfg.get("frames"), img_size=data_cfg.get("img_size"))

    def resize(self, raw: "RawCineBatch", out_dtype: torch.dtype = torch.float32, normalize: bool = False) -> torch.Tensor:
        """One ``pasn_cine_resize`` launch: the batch's windows resized to (N,1,frames,img_size,img_size) ((N,1,img_size,img_size) for
        an image model) in [0, 1], or normalised by ``bin_to_norm`` in the epilogue when ``normalize``.  A host batch is uploaded
        asynchronously first."""
        if self.img_size is None or (self.video and self.frames is None):
            raise ValueError("resizing a RawCineBatch needs the output shape: DeviceClipPipeline(frames=..., img_size=...) or from_config "
                             "with the data config's frames / img_size")
        if raw.device != self.device:
            raw = raw.to(self.device, non_blocking=True)
        frames = self.frames if self.video else 1
        mean, std = (ECHO_MEAN, ECHO_STD) if normalize else (0.0, 1.0)
        y = resample.resize_raw(raw, (frames, self.img_size, self.img_size), out_dtype, mean, std)
        return y.unsqueeze(1) if self.video else y.reshape(len(raw), 1, self.img_size, self.img_size)

    def _grey(self, cine: torch.Tensor) -> torch.Tensor:
        x = cine
        if x.dim() == (4 if self.video else 3):  # (N,T,H,W) / (N,H,W): add the channel axis
            x = x.unsqueeze(1)
        if x.dim() != (5 if self.video else 4) or x.shape[1] != 1:
            raise ValueError("DeviceClipPipeline takes single-channel clips (N,[1,]%sH,W); a 3-channel tensor goes to the model as it is"
                             % ("T," if self.video else ""))
        if x.dtype not in (torch.uint8, torch.float32, torch.bfloat16):
            x = x.float()
        return x

    def _params(self, n: int, height: int, width: int, augment: bool) -> torch.Tensor:
        if not augment:
            key = (n, height, width)
            if key not in self._identity:
                self._identity[key] = identity_augment_params(n, height, width).to(self.device)
            return self._identity[key]
        self._in_flight = [(b, e) for b, e in self._in_flight if not e.query()]
        host = sample_augment_params(n, height, width, self.min_crop_ratio, self.rotate_degrees, self.generator).pin_memory()
        table = host.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._in_flight.append((host, ev))
        return table

    def normalized(self, cine: torch.Tensor, augment: bool = False) -> torch.Tensor:
        """The normalised grey clip (N,1,...) in the model's compute dtype, what the training pass takes: ONE ``pasn_clip_augment`` launch
        (crop + bilinear resize + rotation when ``augment``, then ``bin_to_norm`` when ``normalize``).  Switches the trunk's fused input
        normalisation off, since the clip it returns is already normalised.  A normalisation on the trunk that this pipeline did not set
        (``set_input_normalization``, another pipeline) is never dropped silently: ``GreyInputError``."""
        have = tuple(self.trunk.input_affine)
        if have != (1.0, 0.0) and have != self._affine:
            raise GreyInputError("the trunk carries an input normalisation this pipeline did not set (set_input_normalization or another "
                                 "DeviceClipPipeline); normalized() would drop it, and a normalised grey clip on top of it would be normalised "
                                 "twice.  Call set_input_normalization(None) first, or train on the reference's 3-channel clip")
        out_dtype = self.model._dtype() if hasattr(self.model, "_dtype") else torch.float32
        if isinstance(cine, RawCineBatch):
            if not augment:  # resize + bin_to_norm: one launch
                y = self.resize(cine, out_dtype, normalize=self.normalize)
                self.trunk.set_input_normalization(None)
                self._affine = tuple(self.trunk.input_affine)
                return y
            cine = self.resize(cine, torch.float32)  # the reference resizes first, then crops and rotates
        x = self._grey(cine).contiguous().to(self.device, non_blocking=True)
        n, height, width = x.shape[0], x.shape[-2], x.shape[-1]
        frames = x.shape[2] if x.dim() == 5 else 1
        y = torch.empty(x.shape, dtype=out_dtype, device=self.device)
        params = self._params(n, height, width, augment)
        mean, std = (ECHO_MEAN, ECHO_STD) if self.normalize else (0.0, 1.0)
        _lib.check(_lib.lib().pasn_clip_augment(
            x.data_ptr(), y.data_ptr(), params.data_ptr(), n, frames, height, width, height, width, 1.0 / 255.0 if x.dtype == torch.uint8 else 1.0,
            mean, std, _lib.dtype_code(x.dtype), _lib.dtype_code(out_dtype), _lib.F32, _lib.current_stream()))
        self.trunk.set_input_normalization(None)
        self._affine = tuple(self.trunk.input_affine)
        return y

    def __call__(self, cine: torch.Tensor) -> torch.Tensor:
        if self.model.training:
            return self.normalized(cine, self.augment)
        if isinstance(cine, RawCineBatch):
            cine = self.resize(cine, self.model._dtype() if hasattr(self.model, "_dtype") else torch.float32)
        x = self._grey(cine)
        scale = 1.0 / 255.0 if x.dtype == torch.uint8 else 1.0
        if self.normalize:
            self.trunk.set_input_normalization(ECHO_MEAN, ECHO_STD, scale)
        else:
            self.trunk.set_input_normalization(None)
        self._affine = tuple(self.trunk.input_affine)
        return x.contiguous().to(self.device, non_blocking=True)
