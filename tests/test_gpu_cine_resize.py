"""GPU: ``pasn_cine_resize`` (csrc/cine_resize.hip) -- raw cine windows resized to model clips on the device -- against the fixture of
the reference resize (g10_resize.npz) and a float64 numpy application of the host band tables; ragged batches; the normalising
epilogue; resize + augmentation; ``DPTrainer`` evaluation, training and push on raw batches."""
import os

import numpy as np
import pytest
import torch

from protoasnet_amd import _lib, data, resample
from protoasnet_amd.data import ECHO_MEAN, ECHO_STD, DeviceClipPipeline, collate_raw_cines
from test_cpu_trainer import TRAIN_CFG
from test_gpu_models import BF16_LOGITS
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_resize.npz")
CASES = ("shrink", "grow_t", "mixed", "image", "radius", "fp32")


def _pattern(shape, seed=0, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    t, h, w = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    v = np.clip(0.5 + 0.3 * np.sin(6 * h + 2 * t) * np.cos(5 * w - 3 * t) + 0.1 * rng.standard_normal(shape), 0, 1)
    return np.round(v * 255).astype(np.uint8) if dtype == np.uint8 else v.astype(np.float32)


def _raw(windows):
    """A device RawCineBatch of whole windows (each its own source)."""
    items = [dict(cine=w, window_start=0, window_end=w.shape[0], filename=f"w{i}", target_AS=0) for i, w in enumerate(windows)]
    return collate_raw_cines(items)["cine"].to(DEV)


def _resize(windows, shape, out_dtype=torch.float32, mean=0.0, std=1.0):
    y = resample.resize_raw(_raw(windows), shape, out_dtype, mean, std)
    torch.cuda.synchronize()
    return y.cpu()


def _check_fp32(y, ref, what, tol=5e-6):
    err = float(np.abs(y.double().numpy() - ref).max())
    assert err <= tol, f"{what}: max abs {err:.3g} > {tol}"


def _check_bf16(y, ref64, what):
    """RNE(bf16) of the fp64 result, with at most 1 ulp where that result lies within 1e-5 of a rounding midpoint."""
    r = torch.from_numpy(ref64)
    want = r.float().to(torch.bfloat16)
    diff = (y.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    lo = want.double()
    ulp = ((want.view(torch.int16) + 1).view(torch.bfloat16).double() - lo).abs()
    near = ((r - (lo + ulp / 2)).abs() < 1e-5) | ((r - (lo - ulp / 2)).abs() < 1e-5)
    assert int(diff.max()) <= 1, f"{what}: {int(diff.max())} ulp"
    bad = (diff > 0) & ~near
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs differ from RNE away from a rounding midpoint"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", CASES)
def test_golden_resize(golden, case):
    x, ref = golden[case + "_x"], golden[case + "_y"]
    shape = ref.shape
    bands = resample.apply_bands(x, shape)
    y = _resize([x], shape)[0]
    _check_fp32(y, ref, f"{case} vs reference")
    _check_fp32(y, bands, f"{case} vs host bands")
    _check_bf16(_resize([x], shape, torch.bfloat16)[0], bands, f"{case} bf16")


@pytest.mark.parametrize("si,so", [((40, 600, 800), (32, 112, 112)), ((24, 600, 800), (16, 224, 224)), ((1, 600, 800), (1, 224, 224)),
                                   ((12, 100, 90), (32, 112, 112)), ((60, 1080, 1440), (16, 112, 112))],
                         ids=["video", "x3d_headline", "image", "grow", "widest_band"])
def test_full_shapes_against_host_bands(si, so):
    x = _pattern(si, seed=si[0])
    _check_fp32(_resize([x], so)[0], resample.apply_bands(x, so), f"{si}->{so}")


def test_fp32_source_full_shape():
    x = _pattern((8, 300, 400), seed=5, dtype=np.float32)
    _check_fp32(_resize([x], (16, 112, 112))[0], resample.apply_bands(x, (16, 112, 112)), "fp32 source")


def test_ragged_batch_equals_per_clip_launches_bitwise():
    wins = [_pattern((40, 600, 800), 1), _pattern((12, 100, 90), 2), _pattern((24, 300, 500), 3), _pattern((3, 64, 80), 4)]
    shape = (32, 112, 112)
    batch = _resize(wins, shape)
    for i, w in enumerate(wins):
        assert torch.equal(batch[i], _resize([w], shape)[0]), f"clip {i}"
    for _ in range(5):
        assert torch.equal(_resize(wins, shape), batch)


def test_shared_source_windows_and_interval_batch():
    """Several windows of one cine (``iterate_intervals``): one stored copy, each window resized as if alone."""
    cine = _pattern((30, 120, 160), 6)
    items = [dict(cine=cine, window_start=s, window_end=s + 12, filename="one.mat", target_AS=0) for s in (0, 6, 12, 18)]
    raw = collate_raw_cines(items)["cine"]
    assert raw.buffer.numel() == 30 * 120 * 160
    y = resample.resize_raw(raw.to(DEV), (16, 64, 64), torch.float32).cpu()
    for k, s in enumerate((0, 6, 12, 18)):
        assert torch.equal(y[k], _resize([cine[s:s + 12]], (16, 64, 64))[0])


def test_normalising_epilogue(golden):
    for case in ("shrink", "fp32"):
        x, ref = golden[case + "_x"], golden[case + "_y"]
        plain = _resize([x], ref.shape)
        norm = _resize([x], ref.shape, mean=ECHO_MEAN, std=ECHO_STD)
        want = (plain.numpy() - np.float32(ECHO_MEAN)) / np.float32(ECHO_STD)  # IEEE fp32 subtraction and division
        assert np.array_equal(norm.numpy(), want)


def _pipe_model():
    return synth_model(CFG_VIDEO_X3D).to(DEV)


def test_resize_then_augment_equals_clip_augment(golden):
    x = golden["fp32_x"]
    T, H, W = golden["fp32_y"].shape
    m = _pipe_model().train()
    pipe = DeviceClipPipeline(m, normalize=True, augment=True, rotate_degrees=20, min_crop_ratio=0.6, seed=7, frames=T, img_size=H)
    raw = collate_raw_cines([dict(cine=x, window_start=0, window_end=x.shape[0], filename="g", target_AS=0)] * 1)["cine"]
    got = pipe.normalized(raw, augment=True)
    params = data.sample_augment_params(1, H, W, 0.6, 20, torch.Generator().manual_seed(7)).to(DEV)
    clip = torch.from_numpy(golden["fp32_y"]).float().reshape(1, 1, T, H, W).to(DEV)
    want = torch.empty_like(clip)
    _lib.check(_lib.lib().pasn_clip_augment(clip.data_ptr(), want.data_ptr(), params.data_ptr(), 1, T, H, W, H, W, 1.0, ECHO_MEAN, ECHO_STD,
                                            _lib.F32, _lib.F32, _lib.F32, _lib.current_stream()))
    torch.cuda.synchronize()
    assert got.shape == (1, 1, T, H, W)
    assert float((got - want).abs().max()) <= 1e-5


def test_pipeline_eval_returns_the_unit_clip_with_fused_normalisation():
    m = _pipe_model().eval()
    pipe = DeviceClipPipeline(m, normalize=True, frames=4, img_size=64)
    x = _pattern((9, 100, 120), 8)
    raw = collate_raw_cines([dict(cine=x, window_start=1, window_end=9, filename="e", target_AS=0)])["cine"]
    y = pipe(raw)
    assert y.shape == (1, 1, 4, 64, 64) and y.dtype == torch.float32
    _check_fp32(y[0, 0].cpu(), resample.apply_bands(x[1:9], (4, 64, 64)), "eval clip")
    assert tuple(pipe.trunk.input_affine) != (1.0, 0.0)  # normalisation fused into the trunk


# ---- DPTrainer on raw batches -------------------------------------------------------------------------------------------------------
def _loaders(n, B=2, seed=30):
    """The same clips as raw uint8 batches and as host-resized fp32 clips (numpy bands)."""
    class L(list):
        batch_size = B

    raw, pre = L(), L()
    for b in range(n):
        items = []
        for i in range(B):
            cine = _pattern((10 + i, 90 + 7 * b, 110 + 5 * i), seed + 10 * b + i)
            s = i % 3
            items.append(dict(cine=cine, window_start=s, window_end=s + 7, filename=f"c{b}_{i}", target_AS=(b + i) % 3, interval_idx=i))
        batch = collate_raw_cines(items)
        raw.append(batch)
        clips = np.stack([resample.apply_bands(it["cine"][it["window_start"]:it["window_end"]], (4, 64, 64)) for it in items])
        pre.append(dict(batch, cine=torch.from_numpy(clips).float().unsqueeze(1)))
    return raw, pre


def _trainer(m, loaders, **kw):
    from protoasnet_amd.trainer import DPTrainer

    cfg = {"abstain_class": False, "save_dir": "", "train": dict(TRAIN_CFG, save=False, **kw),
           "data": {"augmentation": False, "normalize": True, "frames": 4, "img_size": 64}}
    return DPTrainer(m, cfg, loaders, log=lambda *_: None)


def _eval_logits(m, loader):
    out = []
    h = m.register_forward_hook(lambda mod, inp, o: out.append(o[0].detach().float().cpu()))
    try:
        res = _trainer(m, {"val": loader}).evaluate("val")
    finally:
        h.remove()
    return torch.cat(out), res


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_trainer_evaluate_on_raw_batches(dtype):
    raw, pre = _loaders(3)
    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    if dtype == torch.bfloat16:
        m.set_compute_dtype(torch.bfloat16)
    lr, res_r = _eval_logits(m, raw)
    lp, res_p = _eval_logits(m, pre)
    assert lr.shape == lp.shape == (6, 3)
    tol = 1e-4 if dtype == torch.float32 else BF16_LOGITS
    assert float((lr - lp).abs().max()) <= tol
    assert res_r["accuracy"] == res_p["accuracy"]


@pytest.mark.timeout(900)
def test_trainer_train_step_and_push_on_raw_batches():
    raw, pre = _loaders(2)
    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    t = _trainer(m, {"train": raw[:1]}, accumulation_steps=1)
    res = t.run_epoch(0, mode="train")
    assert np.isfinite(res["loss"])
    assert any(not torch.equal(p, before[n]) for n, p in m.named_parameters())
    # push: the same winners on raw batches as on the pre-resized clips (fp32)
    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    got = {}
    for tag, loader in (("raw", raw), ("pre", pre)):
        t = _trainer(m, {"train_push": loader})
        got[tag] = t.push(replace_prototypes=False)
    assert torch.equal(got["raw"]["proto_index"].cpu(), got["pre"]["proto_index"].cpu())
    assert float((got["raw"]["proto_dist"] - got["pre"]["proto_dist"]).abs().max()) <= 1e-4


@pytest.mark.timeout(600)
def test_dataloader_pin_memory_and_upload_overlap():
    """``DataLoader(collate_fn=collate_raw_cines, pin_memory=True)``: pinned raw batches, staged on the copy stream by the trainer."""
    cines = [_pattern((12, 80, 96), 40 + i) for i in range(4)]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 4

        def __getitem__(self, i):
            return dict(cine=cines[i], window_start=1, window_end=9, filename=f"f{i}", target_AS=i % 3)

    loader = torch.utils.data.DataLoader(DS(), batch_size=2, collate_fn=collate_raw_cines, pin_memory=True)
    batches = list(loader)
    assert all(isinstance(b["cine"], data.RawCineBatch) and b["cine"].is_pinned() for b in batches)
    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    t = _trainer(m, {"val": loader})
    staged = list(t.staged(loader))
    assert all(s["cine"].device.type == "cuda" and s["cine"].ready is not None for s in staged)
    x = t.prepare_input(staged[1]["cine"])
    torch.cuda.synchronize()
    want = np.stack([resample.apply_bands(c[1:9], (4, 64, 64)) for c in cines[2:]])
    assert float(np.abs(((x.float().cpu().numpy() * ECHO_STD + ECHO_MEAN)[:, 0]) - want).max()) <= 1e-5
