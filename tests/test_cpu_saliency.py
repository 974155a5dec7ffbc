"""CPU: RISE saliency -- the C-ABI / Python surface with its argument checks (no device), and the numpy restatement of
tests/saliency_cases.py (what the GPU tests hold the kernels to) against the properties the definitions promise."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import protoasnet_amd
import saliency_cases as sc
from protoasnet_amd import _lib, faithfulness, model_builder, saliency
from util import CFG_PPNET, CFG_XPROTO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_rise_apply", "pasn_rise_scores", "pasn_rise_stage_masks", "pasn_rise_maps_workspace_bytes", "pasn_rise_maps")
# (clip grid, coarse grid): the three the definitions were drafted on, the two odd ones of the GPU tests, a grid that divides nothing
CASES = [((4, 24, 24), (2, 4, 4)), ((1, 23, 17), (1, 5, 3)), ((3, 9, 7), (2, 2, 2)), ((7, 17, 23), (2, 3, 4)), ((37, 45), (1, 5, 4)),
         ((5, 5, 5), (16, 7, 7))]


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pasn_\w+)", nm))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
        assert getattr(lib, name) is not None
    assert "saliency" in protoasnet_amd.__all__ and protoasnet_amd.saliency is saliency  # exported lazily, like its neighbours
    assert "rise.hip" in protoasnet_amd.build.SOURCES


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    wrong = {what: rc for what, rc in sc.abi_refusals(lib, _lib.F32, _lib.U8).items() if rc != 1}
    assert not wrong, wrong
    with pytest.raises(ValueError, match="lattice"):
        _lib.check(lib.pasn_rise_apply(256, 0, 0.0, 1, 3, 4, 24, 24, 17, 4, 4, 1 << 31, 0, 0, 0, 1, _lib.F32, 256, 0))
    # the masks a block stages shrink as the lattice grows, and the workspace grows with clips, maps and masks
    stage, size = lib.pasn_rise_stage_masks, lib.pasn_rise_maps_workspace_bytes
    assert 1 <= stage(16, 20, 18) < stage(4, 7, 7) <= 64
    assert size(2, 1, 64, 16, 224, 224, 4, 7, 7) == 2 * size(1, 1, 64, 16, 224, 224, 4, 7, 7) and size(1, 1, 64, 16, 224, 224, 4, 7, 7) % 16 == 0
    assert size(1, 3, 64, 4, 24, 24, 2, 4, 4) > size(1, 1, 64, 4, 24, 24, 2, 4, 4) and size(1, 1, 65, 4, 24, 24, 2, 4, 4) > size(1, 1, 64, 4, 24, 24, 2, 4, 4)


def test_keep_comes_from_p():
    assert saliency.keep_threshold(0.5) == 1 << 31 == sc.keep_of(0.5)
    assert saliency.keep_threshold(0.25) == 1 << 30 and saliency.keep_threshold(2.0 ** -32) == 1
    assert saliency.keep_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1  # floor(p 2^32) = 2^32 - 1 here; min() guards the rounding of p itself
    assert saliency.keep_threshold(0.3) == int(np.floor(0.3 * 2.0 ** 32)) == sc.keep_of(0.3)
    for p in (0.0, 1.0, -0.1, 1.5, float("nan"), 2.0 ** -33):
        with pytest.raises(ValueError):
            saliency.keep_threshold(p)


def test_python_surface_raises_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    x = torch.zeros(2, 3, 4, 24, 24)
    ok = dict(grid=(2, 4, 4), p=0.5, seed=1, clip0=0, m0=0, Mc=2)
    for bad in (dict(grid=(0, 4, 4)), dict(grid=(17, 4, 4)), dict(grid=(2, 33, 4)), dict(grid=(2, 4, 33)), dict(grid=(16, 21, 21)), dict(grid=(4, 4)),
                dict(grid=(2.0, 4, 4)), dict(p=0.0), dict(p=1.0), dict(seed=-1), dict(seed=1 << 64), dict(clip0=-1), dict(clip0=(1 << 32) - 1),
                dict(m0=-1), dict(Mc=0), dict(m0=65534, Mc=2), dict(Mc=True)):
        with pytest.raises(ValueError):
            saliency.masked_clips(x, **{**ok, **bad})
    with pytest.raises(TypeError):
        saliency.masked_clips(x.half(), **ok)
    with pytest.raises(ValueError, match="baseline"):
        saliency.masked_clips(x, baseline=x[:1], **ok)
    with pytest.raises(ValueError):
        saliency.masked_clips(torch.zeros(2, 65, 4, 24, 24), **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.masked_clips(x, **ok)
    s = torch.zeros(2, 5, 1)
    for bad in (dict(norm="mean"), dict(p=1.0), dict(grid=(2, 4, 33)), dict(shape=(24,)), dict(shape=(4, 0, 24)), dict(seed=-1),
                dict(maps=False, saliency=False)):
        with pytest.raises(ValueError):
            saliency.saliency_maps(s, **{**dict(shape=(4, 24, 24), grid=(2, 4, 4), p=0.5), **bad})
    with pytest.raises(ValueError):
        saliency.saliency_maps(s.double(), (4, 24, 24), (2, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.saliency_maps(s, (4, 24, 24), (2, 4, 4), 0.5)
    sim, sel = torch.zeros(2, 5, 12), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="target"):
        saliency.mask_scores(sim, None, sel, None, target="logit")
    with pytest.raises(ValueError):
        saliency.mask_scores(sim, None, sel.long(), None)
    with pytest.raises(ValueError):
        saliency.mask_scores(None, torch.zeros(2, 5, 4), None, torch.zeros(2, dtype=torch.int32), target="class", K_real=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.mask_scores(sim, None, sel, None)
    # the model entry point
    with pytest.raises(NotImplementedError, match="RISE"):
        saliency.rise(model_builder.build(CFG_PPNET).eval(), torch.zeros(1, 3, 224, 224))
    m = model_builder.build(CFG_XPROTO).eval()
    assert m.rise.__func__ is type(m).rise  # on the head-B mixin, next to faithfulness
    xi = torch.zeros(1, 3, 224, 224)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.rise(xi)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.rise(xi)
    # the sweep's kinds
    for kinds in ((), ("random", "model"), ("model", "model"), ("model", "rise", "blur")):
        with pytest.raises(ValueError, match="kinds"):
            faithfulness.FaithfulnessAccumulator(m, kinds=kinds)
    with pytest.raises(ValueError, match="rise"):
        faithfulness.FaithfulnessAccumulator(m, rise=dict(masks=8))
    acc = faithfulness.FaithfulnessAccumulator(m)
    assert acc.kinds == ("model", "random") == faithfulness.FaithfulnessAccumulator.KINDS


def test_grid_defaults():
    assert saliency.check_grid(None, (16, 224, 224), True) == (4, 7, 7) and saliency.check_grid(None, (1, 224, 224), False) == (1, 7, 7)
    assert saliency.check_grid((5, 4), (1, 37, 45), False) == (1, 5, 4) and saliency.check_grid((16, 20, 18), (4, 4, 4), True) == (16, 20, 18)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,grid", CASES, ids=[f"{s}/{g}" for s, g in CASES])
def test_masks_stay_inside_the_lattice_and_the_unit_interval(shape, grid):
    T, H, W = sc.thw(shape)
    ct, ch, cw = sc.cells(shape, grid)
    assert (ct, ch, cw) == (-(-T // grid[0]), -(-H // grid[1]), -(-W // grid[2]))
    seen = set()
    for keep in (sc.keep_of(0.5), sc.keep_of(0.1), 2 ** 32 - 1):
        for m in range(12):
            st, sh, sw = sc.shifts(shape, grid, 9, 3, m)
            assert 0 <= st < ct and 0 <= sh < ch and 0 <= sw < cw
            seen.add((st, sh, sw))
            for (n, c, s, g) in ((T, ct, st, grid[0]), (H, ch, sh, grid[1]), (W, cw, sw, grid[2])):
                i, f = sc.axis(n, c, s)
                assert i.min() >= 0 and i.max() + 1 <= g + 1  # the upper neighbour exists: the lattice has g + 2 points
                assert f.dtype == np.float32 and f.min() >= 0.0 and f.max() < 1.0
            mk = sc.mask(shape, grid, keep, 9, 3, m)
            assert mk.dtype == np.float32 and mk.shape == (T, H, W) and mk.min() >= 0.0 and mk.max() <= 1.0
        lat = sc.lattice(grid, keep, 9, 3, 0)
        assert lat.shape == tuple(g + 2 for g in grid) and set(np.unique(lat)) <= {0.0, 1.0}
    assert np.array_equal(sc.mask(shape, grid, 2 ** 32 - 1, 9, 3, 0), np.ones((T, H, W), np.float32))  # every word is below 2^32 - 1 here
    if ct * ch * cw > 4:
        assert len(seen) > 1


def test_one_frame_reads_the_lower_plane_exactly():
    shape, grid, keep = (1, 23, 17), (1, 5, 3), sc.keep_of(0.5)
    for m in range(6):
        assert sc.shifts(shape, grid, 4, 0, m)[0] == 0  # a cell of one frame has one shift
        i, f = sc.axis(1, 1, 0)
        assert i.tolist() == [0] and f.tolist() == [0.0]
        lat = sc.lattice(grid, keep, 4, 0, m)
        lower = lat.copy()
        lower[1:] = 1.0 - lower[1:]  # whatever the upper planes hold ...
        _, sh, sw = sc.shifts(shape, grid, 4, 0, m)
        (iy, fy), (ix, fx) = sc.axis(23, 5, sh), sc.axis(17, 6, sw)
        iy, ix, fy, fx = iy[:, None], ix[None, :], fy[:, None], fx[None, :]
        plane = sc.lerp(sc.lerp(lat[0][iy, ix], lat[0][iy, ix + 1], fx), sc.lerp(lat[0][iy + 1, ix], lat[0][iy + 1, ix + 1], fx), fy)
        assert np.array_equal(sc.mask(shape, grid, keep, 4, 0, m)[0], plane)  # ... the mask is the bilinear map of plane 0
    # an image given as (H, W) is the clip (1, H, W)
    assert np.array_equal(sc.mask((23, 17), grid, keep, 4, 0, 2), sc.mask(shape, grid, keep, 4, 0, 2))


def test_masks_depend_on_seed_clip_and_index_only():
    shape, grid, keep = (3, 9, 7), (2, 2, 2), sc.keep_of(0.5)
    base = sc.mask(shape, grid, keep, 5, 2, 1)
    assert np.array_equal(base, sc.mask(shape, grid, keep, 5, 2, 1))
    assert not np.array_equal(base, sc.mask(shape, grid, keep, 6, 2, 1)) and not np.array_equal(base, sc.mask(shape, grid, keep, 5, 3, 1))
    assert not np.array_equal(base, sc.mask(shape, grid, keep, 5, 2, 2)) and not np.array_equal(base, sc.mask(shape, grid, keep, 5 + (1 << 32), 2, 1))
    # the keep fraction of many lattice points is p
    frac = np.mean([sc.lattice((4, 7, 7), sc.keep_of(0.3), 1, 0, m).mean() for m in range(64)])
    assert abs(frac - 0.3) < 0.01


def test_masked_clips_of_the_restatement():
    shape, grid, V = (3, 9, 7), (2, 2, 2), 189
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 3, V)).astype(np.float32)
    base = rng.standard_normal((2, 3, V)).astype(np.float32)
    ones = sc.masked_ref(x, shape, grid, 2 ** 32 - 1, 0, 0, 0, 2, fill=np.float32(0.0))  # the all-ones mask: 0 + (x - 0) 1
    assert np.array_equal(ones, np.broadcast_to(x[:, None], ones.shape))
    out = sc.masked_ref(x, shape, grid, sc.keep_of(0.5), 3, 4, 2, 3, baseline=base)
    lo, hi = np.minimum(x, base)[:, None], np.maximum(x, base)[:, None]
    assert out.shape == (2, 3, 3, V) and (out >= lo - 1e-6).all() and (out <= hi + 1e-6).all()  # a blend of the two
    again = sc.masked_ref(x[1:], shape, grid, sc.keep_of(0.5), 3, 5, 3, 1, baseline=base[1:])
    assert np.array_equal(again[0, 0], out[1, 1])  # clip 5, mask 3, whatever the batch and the chunk
    # bf16: one rounding to nearest even, ties included; NaN is canonical
    f = np.array([1.0, 1.00390625, 1.01171875, np.inf, np.nan], np.float32)  # 1 + 2^-8 ties to 1, 1 + 3 2^-8 ties up to 1 + 2^-6
    assert sc.narrow(f, np.zeros(1, np.uint16)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x7F80, 0x7FC0]
    assert sc.narrow(np.array([-np.nan], np.float32), np.zeros(1, np.float32)).view(np.uint32).tolist() == [0x7FC00000]


def test_saliency_sums_and_norms():
    shape, grid, keep, M = (3, 9, 7), (2, 2, 2), sc.keep_of(0.5), 9
    rng = np.random.default_rng(2)
    scores = rng.standard_normal((M, 2)).astype(np.float32)
    sal, u8, cov = sc.saliency_ref(scores, shape, grid, keep, 1, 0, "coverage")
    masks = np.stack([sc.mask(shape, grid, keep, 1, 0, m).reshape(-1) for m in range(M)]).astype(np.float64)
    assert np.allclose(cov, masks.sum(0), rtol=1e-14) and np.allclose(sal[1], (scores[:, 1].astype(np.float64) @ masks) / cov, rtol=1e-6)
    exp, _, _ = sc.saliency_ref(scores, shape, grid, keep, 1, 0, "expected")
    assert np.allclose(exp[0], (scores[:, 0].astype(np.float64) @ masks) / (M * 0.5), rtol=1e-6)
    assert u8.dtype == np.uint8 and u8.shape == (2, 189) and u8.min() == 0 and u8.max() == 254  # (max - min) / (max - min + 1e-7) < 1
    # equal power-of-two scores: S = s Cov exactly at every step, so the coverage norm gives s everywhere and the map is all zeros
    flat, zeros, _ = sc.saliency_ref(np.full((M, 1), 0.5, np.float32), shape, grid, keep, 1, 0, "coverage")
    assert (flat == 0.5).all() and not zeros.any()
    # a keep so small that a voxel is never covered: 0, not NaN
    dark, _, cov0 = sc.saliency_ref(scores[:2], shape, grid, sc.keep_of(0.02), 1, 0, "coverage")
    assert (cov0 == 0).any() and np.isfinite(dark).all() and (dark[:, cov0 == 0] == 0).all()


def test_planted_box_is_found():
    case = sc.BOX_CASE
    scores = sc.box_scores()
    assert scores.shape == (case["M"], 1) and 0.0 <= scores.min() and scores.max() <= 1.0
    for norm in saliency.NORMS:
        sal, _, _ = sc.saliency_ref(scores, case["shape"], case["grid"], sc.keep_of(case["p"]), case["seed"], case["clip"], norm)
        inside, outside, hit = sc.box_summary(sal[0])
        print(f"{norm}: mean inside {inside:.3f}, outside {outside:.3f}, argmax inside {hit}")
        assert inside > outside and hit
