"""GPU: RISE saliency (csrc/rise.hip through protoasnet_amd.saliency) against the numpy restatement of tests/saliency_cases.py: the masked
clips and the maps bit for bit, the class scores against float64, a planted box, the whole path against the model run on the
restatement's clips, and DPTrainer.evaluate_faithfulness with the "rise" kind against its batches."""
import numpy as np
import pytest
import torch

import saliency_cases as sc
from conftest import TOL_SIM, assert_close
from protoasnet_amd import _lib, faithfulness, saliency, synth
from test_cpu_trainer import TRAIN_CFG
from util import CFG_PPNET, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"

# clip grid, coarse grid.  "odd": V = 2737 is odd, every row but the first starts off the 16-byte grid, and V < one tile of 4096; "image":
# no frame axis, V = 1665 odd; "small": V = 6272, two tiles of the apply kernel and 25 blocks of the maps kernel, the last one partial;
# "lattice": 7920 lattice points -- more than one Philox call per thread of a block, and a stage of only four masks.
GRIDS = {"odd": ((7, 17, 23), (2, 3, 4)), "image": ((37, 45), (1, 5, 4)), "small": ((8, 28, 28), (2, 4, 4)), "lattice": ((5, 21, 19), (16, 20, 18))}
KEEP = sc.keep_of(0.5)


def _raw(t):
    """The bit patterns of a device tensor, on the host: float32 as it is, bf16 as uint16."""
    t = t.cpu()
    return t.numpy() if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _clips(shape, N, C, dtype, seed):
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    x = torch.from_numpy(rng.standard_normal((N, C) + shape).astype(np.float32)).to(DEV).to(dtype)
    x.view(-1)[3], x.view(-1)[V + 1], x.view(-1)[-1], x.view(-1)[V // 2] = float("nan"), -0.0, float("inf"), float("-inf")
    base = torch.from_numpy(rng.standard_normal((N, C) + shape).astype(np.float32)).to(DEV).to(dtype)
    return x, base


# ---- 1. pasn_rise_apply --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", ["odd", "image"])
def test_masked_clips_equal_the_restatement_bitwise(name, C, dtype):
    shape, grid = GRIDS[name]
    N, V, m0, Mc, seed, clip0 = 2, int(np.prod(shape)), 2, 3, 0x1234567890ABCDEF, 5
    x, base = _clips(shape, N, C, dtype, V + C)
    fill = -0.7173  # not a bf16 number: rounded once, to nearest even
    fill_raw = _raw(torch.tensor([fill], dtype=dtype))[0]
    for baseline in (None, base):
        got = saliency.masked_clips(x, grid, 0.5, seed, clip0, m0, Mc, baseline=baseline, fill=fill)
        assert got.shape == (N, Mc, C) + shape and got.dtype == dtype
        want = sc.masked_ref(_raw(x).reshape(N, C, V), shape, grid, KEEP, seed, clip0, m0, Mc,
                             None if baseline is None else _raw(base).reshape(N, C, V), fill_raw)
        bad = _bits(_raw(got).reshape(want.shape)) != _bits(want)
        assert not bad.any(), (baseline is not None, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert np.isnan(sc.widen(want)).any() and np.isinf(sc.widen(want)).any()  # the special values went through


def test_masked_clips_of_a_large_lattice_and_of_two_tiles():
    for name, dtype in (("lattice", torch.float32), ("small", torch.bfloat16)):
        shape, grid = GRIDS[name]
        V = int(np.prod(shape))
        x, _ = _clips(shape, 1, 2, dtype, 7)
        got = saliency.masked_clips(x, grid, 0.5, 3, 9, 1, 2)
        want = sc.masked_ref(_raw(x).reshape(1, 2, V), shape, grid, KEEP, 3, 9, 1, 2, None, _raw(torch.zeros(1, dtype=dtype))[0])
        assert np.array_equal(_bits(_raw(got).reshape(want.shape)), _bits(want)), name


def test_masked_clips_do_not_depend_on_the_batching():
    shape, grid = GRIDS["odd"]
    x, base = _clips(shape, 3, 3, torch.float32, 11)
    whole = saliency.masked_clips(x, grid, 0.3, 21, 40, 0, 5, baseline=base).view(torch.int32)
    for m0, Mc in ((0, 2), (2, 3), (4, 1)):  # the masks m0 .. m0 + Mc - 1 of a chunked call are slices of the whole
        part = saliency.masked_clips(x, grid, 0.3, 21, 40, m0, Mc, baseline=base).view(torch.int32)
        assert torch.equal(part, whole[:, m0:m0 + Mc]), (m0, Mc)
    for n in range(3):  # clip n of a batch at clip0 is the single clip at clip0 + n
        alone = saliency.masked_clips(x[n:n + 1], grid, 0.3, 21, 40 + n, 0, 5, baseline=base[n:n + 1]).view(torch.int32)
        assert torch.equal(alone[0], whole[n]), n
    assert not torch.equal(whole[0], whole[1]) and not torch.equal(whole[:, 0], whole[:, 1])
    other = saliency.masked_clips(x, grid, 0.3, 22, 40, 0, 5, baseline=base).view(torch.int32)
    assert not torch.equal(other, whole)


# ---- 2. pasn_rise_maps ---------------------------------------------------------------------------------------------------------------------
def _maps_case(shape, grid, N, M, k, norm, seed, clip0, scores=None, p=0.5):
    rng = np.random.default_rng(M * 31 + k)
    if scores is None:
        scores = rng.standard_normal((N, M, k)).astype(np.float32)
        scores.reshape(-1)[::5] = 0.0  # negative and zero scores included
    d = torch.from_numpy(scores).to(DEV)
    sal, u8, cov = saliency.saliency_maps(d, shape, grid, p, seed, clip0, norm, maps=True, saliency=True, cov=True)
    V = int(np.prod(shape))
    assert sal.shape == (N, k) + tuple(shape) and u8.shape == sal.shape and cov.shape == (N,) + tuple(shape)
    assert sal.dtype == torch.float32 and u8.dtype == torch.uint8 and cov.dtype == torch.float64
    for n in range(N):
        r_sal, r_u8, r_cov = sc.saliency_ref(scores[n], shape, grid, sc.keep_of(p), seed, clip0 + n, norm)
        assert np.array_equal(cov[n].reshape(V).cpu().numpy(), r_cov), (n, "cov")
        assert np.array_equal(sal[n].reshape(k, V).cpu().numpy().view(np.uint32), r_sal.view(np.uint32)), (n, "saliency")
        assert np.array_equal(u8[n].reshape(k, V).cpu().numpy(), r_u8), (n, "maps")
    # the uint8 maps alone (the fp32 values then live in the workspace) are the same maps
    _, alone, none = saliency.saliency_maps(d, shape, grid, p, seed, clip0, norm, maps=True, saliency=False)
    assert none is None and torch.equal(alone, u8)
    return sal, u8, cov


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["odd", "image", "small"])
def test_maps_equal_the_restatement_bitwise(name, k):
    shape, grid = GRIDS[name]
    stage = saliency.stage_masks(grid)
    assert stage == 64  # these lattices are small: a block stages 64 masks at a time
    for norm in saliency.NORMS:
        for M in (1, 37, stage + 1):
            _maps_case(shape, grid, 2, M, k, norm, seed=77, clip0=3)


def test_maps_of_a_large_lattice_and_of_five_maps():
    shape, grid = GRIDS["lattice"]
    stage = saliency.stage_masks(grid)
    assert stage == 4
    _maps_case(shape, grid, 1, stage + 1, 2, "coverage", seed=5, clip0=0)
    # five maps: a launch of four and a launch of one
    _maps_case(GRIDS["odd"][0], GRIDS["odd"][1], 2, 9, 5, "expected", seed=6, clip0=1)


def test_degenerate_maps():
    shape, grid = GRIDS["odd"]
    V = int(np.prod(shape))
    # all-zero scores: S = 0 under both norms; equal power-of-two scores under "coverage": S = s Cov exactly at every step
    for norm, s in (("coverage", 0.0), ("expected", 0.0), ("coverage", 0.5)):
        sal, u8, _ = _maps_case(shape, grid, 1, 37, 2, norm, 1, 0, scores=np.full((1, 37, 2), s, np.float32))
        assert not bool(u8.any()) and bool((sal == s).all()), (norm, s)
    _maps_case(shape, grid, 1, 1, 1, "coverage", 1, 0)  # M = 1
    # a keep so small that some voxel is never covered: 0 there, not NaN
    p = 0.02
    _, _, r_cov = sc.saliency_ref(np.ones((2, 1), np.float32), shape, grid, sc.keep_of(p), 1, 0, "coverage")
    assert (r_cov == 0).any() and (r_cov > 0).any()
    sal, _, cov = _maps_case(shape, grid, 1, 2, 1, "coverage", 1, 0, p=p)
    assert bool((cov == 0).any()) and bool((sal.reshape(-1)[cov.reshape(-1) == 0] == 0).all()) and bool(torch.isfinite(sal).all())


def test_planted_box_is_found_on_the_device():
    case = sc.BOX_CASE
    scores = torch.from_numpy(sc.box_scores()).to(DEV)[None]  # (1, M, 1), from the restatement's masks
    for norm in saliency.NORMS:
        sal, _, _ = saliency.saliency_maps(scores, case["shape"], case["grid"], case["p"], case["seed"], case["clip"], norm, maps=False)
        inside, outside, hit = sc.box_summary(sal[0, 0].cpu().numpy())
        print(f"{norm}: mean inside {inside:.3f}, outside {outside:.3f}, argmax inside {hit}")
        assert inside > outside and hit


# ---- 3. pasn_rise_scores -------------------------------------------------------------------------------------------------------------------
def test_scores_kernel():
    N, M, k, P, K, K_real = 3, 37, 2, 12, 4, 3
    rng = np.random.default_rng(8)
    sim = rng.random((N, M, P), dtype=np.float32)
    logits = (4 * rng.standard_normal((N, M, K))).astype(np.float32)
    sel = rng.integers(0, P, (N, k)).astype(np.int32)
    cls = rng.integers(0, K_real, N).astype(np.int32)
    d_sim, d_logits = torch.from_numpy(sim).to(DEV), torch.from_numpy(logits).to(DEV)
    got = saliency.mask_scores(d_sim, None, torch.from_numpy(sel).to(DEV), None, "prototype")
    assert got.shape == (N, M, k) and np.array_equal(got.cpu().numpy().view(np.uint32), sc.scores_ref(sim, None, sel, None, "prototype", K_real).view(np.uint32))
    prob = saliency.mask_scores(None, d_logits, None, torch.from_numpy(cls).to(DEV), "class", K_real)
    err = float(np.abs(prob.cpu().numpy() - sc.scores_ref(None, logits, None, cls, "class", K_real)).max())
    print(f"max |prob - float64| = {err:.3g}")
    assert prob.shape == (N, M, 1) and err <= 1e-6  # fp32 softmax of three terms, values <= 1: the bound of test_curves_kernel_against_float64
    # an index outside its range reads nothing: NaN for that (clip, map) only
    sel[1, 0], sel[2, 1], cls[0], cls[2] = P, -1, K_real, -1
    got = saliency.mask_scores(d_sim, None, torch.from_numpy(sel).to(DEV), None, "prototype")
    assert torch.isnan(got).all(1).cpu().tolist() == [[False, False], [True, False], [False, True]]
    assert torch.isnan(got).any(1).cpu().tolist() == [[False, False], [True, False], [False, True]]
    prob = saliency.mask_scores(None, d_logits, None, torch.from_numpy(cls).to(DEV), "class", K_real)
    assert torch.isnan(prob).all(1).cpu().tolist() == [[True], [False], [True]]


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,shape", [(CFG_VIDEO_X3D, (2, 3, 4, 64, 64)), (CFG_XPROTO, (2, 3, 224, 224))], ids=["x3d_s", "xprotonet_image"])
def test_rise_end_to_end(cfg, shape):
    m = synth_model(cfg).to(DEV).eval()
    x = synth.echo_clips(shape).to(DEV)
    N, C, vol = shape[0], shape[1], tuple(shape[2:])
    V, k, M, seed, clip0 = int(np.prod(vol)), 2, 32, 13, 6
    grid = saliency.GRID_VIDEO if len(vol) == 3 else saliency.GRID_IMAGE
    r = m.rise(x, select=k, masks=M, seed=seed, clip0=clip0)
    e = m.explain(x, select=k, maps=None)
    assert torch.equal(r.selected, e.selected) and torch.equal(r.pred, e.pred)
    assert r.maps.shape == (N, k) + vol and r.maps.dtype == torch.uint8 and r.saliency.shape == (N, k) + vol and r.scores.shape == (N, M, k)
    # the maps are the restatement's of the device's own scores
    scores = r.scores.cpu().numpy()
    for n in range(N):
        r_sal, r_u8, _ = sc.saliency_ref(scores[n], vol, grid, KEEP, seed, clip0 + n, "coverage")
        assert np.array_equal(r.saliency[n].reshape(k, V).cpu().numpy().view(np.uint32), r_sal.view(np.uint32)), n
        assert np.array_equal(r.maps[n].reshape(k, V).cpu().numpy(), r_u8), n
    # the scores are the model's on the restatement's masked clips
    clips = sc.masked_ref(x.reshape(N, C, V).cpu().numpy(), vol, grid, KEEP, seed, clip0, 0, M, None, np.float32(0.0))
    with torch.no_grad():
        _, sim, _ = m(torch.from_numpy(clips).to(DEV).reshape((N * M, C) + vol))
    want = sim.reshape(N, M, -1).gather(2, e.selected.long()[:, None, :].expand(N, M, k))
    assert_close(r.scores, want, TOL_SIM, name="scores")
    # the curves under "rise" are the curves under its maps, handed over as a tensor
    args = dict(masks=M, seed=seed, clip0=clip0)
    a = faithfulness.perturbation_curves(m, x, select=k, steps=4, mode="both", saliency="rise", rise=args)
    b = faithfulness.perturbation_curves(m, x, select=k, steps=4, mode="both", saliency=r.maps)
    for mode in faithfulness.MODES:
        ca, cb = getattr(a, mode), getattr(b, mode)
        for field in ("similarity", "prob", "auc_similarity", "auc_prob", "steps"):
            assert torch.equal(getattr(ca, field), getattr(cb, field)), (mode, field)
    # one seed is one result, two seeds are two
    again, other = m.rise(x, select=k, masks=M, seed=seed, clip0=clip0), m.rise(x, select=k, masks=M, seed=seed + 1, clip0=clip0)
    assert torch.equal(again.maps, r.maps) and torch.equal(again.saliency, r.saliency) and torch.equal(again.scores, r.scores)
    assert not torch.equal(other.maps, r.maps)
    # smaller forwards (24: one clip at a time, chunks of 24 masks, the last one padded) give the same maps for an fp32 model
    alt = m.rise(x, select=k, masks=M, seed=seed, clip0=clip0, max_batch=24)
    assert torch.equal(alt.maps, r.maps)
    # the class target: one map per clip, the probability of the predicted class
    c = m.rise(x, masks=8, target="class", norm="expected", seed=seed, maps=None)
    assert c.maps is None and c.saliency.shape == (N, 1) + vol and bool(((c.scores >= 0) & (c.scores <= 1)).all())


# ---- 5. the sweep --------------------------------------------------------------------------------------------------------------------------
def test_trainer_evaluate_faithfulness_with_rise():
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    batches = [{"cine": synth.echo_clips((2, 3, 4, 64, 64), seed=90 + b), "target_AS": torch.tensor([b, 1]), "filename": [f"a{b}", f"b{b}"]}
               for b in range(2)]
    logs = []
    t = DPTrainer(m, {"abstain_class": True, "train": TRAIN_CFG}, {"train": batches, "val": batches}, log=lambda s, *_: logs.append(str(s)))
    k, S1, args = 2, 5, dict(masks=8, grid=(2, 4, 4))
    res = t.evaluate_faithfulness("val", steps=4, select=k, seed=7, kinds=("model", "random", "rise"), rise=args)
    assert sum("faithfulness" in s for s in logs) == 2 and any("vs rise" in s for s in logs) and any("vs random" in s for s in logs)
    assert set(res) == {"clips", "fractions", "deletion", "insertion", "random", "difference", "rise", "difference_rise"}
    assert res["clips"] == 4 and res["rise"]["insertion"]["similarity"].shape == (k, S1) and res["difference_rise"]["deletion"]["auc_prob"].shape == (k,)
    m.eval()
    # the float64 combination of the batches' own curves; batch b starts at clip 2 b
    kinds = (("model", {}), ("random", dict(saliency="random")), ("rise", dict(saliency="rise")))
    for kind, kw in kinds:
        pairs = [faithfulness.perturbation_curves(m, t.prepare_input(b["cine"]), select=k, steps=4, mode="both", seed=7 + i,
                                                  **({**kw, "rise": dict(args, seed=7, clip0=2 * i)} if kind == "rise" else kw))
                 for i, b in enumerate(batches)]
        for mode in faithfulness.MODES:
            got = res[mode] if kind == "model" else res[kind][mode]
            for field in ("similarity", "prob", "auc_similarity", "auc_prob"):
                rows = np.concatenate([getattr(getattr(p, mode), field).double().cpu().numpy() for p in pairs])  # (clips, k[, S1])
                want = rows.sum(0) / 4.0
                err = float((np.abs(got[field] - want) / np.abs(want)).max())
                assert err <= 1e-12, (kind, mode, field, err)
    d = res["difference_rise"]["insertion"]["auc_similarity"]
    assert np.array_equal(d, res["insertion"]["auc_similarity"] - res["rise"]["insertion"]["auc_similarity"])
    # the default kinds: exactly the dictionary of before
    plain = t.evaluate_faithfulness("val", steps=4, select=k, seed=7)
    assert set(plain) == {"clips", "fractions", "deletion", "insertion", "random", "difference"}
    for mode in faithfulness.MODES:
        assert np.array_equal(plain[mode]["auc_prob"], res[mode]["auc_prob"]) and np.array_equal(plain["random"][mode]["prob"], res["random"][mode]["prob"])


# ---- 6. arguments --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    lib = _lib.lib()
    wrong = {what: rc for what, rc in sc.abi_refusals(lib, _lib.F32, _lib.U8).items() if rc != 1}
    assert not wrong, wrong
    x = torch.zeros((1, 3, 4, 24, 24), device=DEV)
    for bad in (dict(grid=(17, 4, 4)), dict(grid=(2, 33, 4)), dict(grid=(16, 21, 21)), dict(p=1.0), dict(Mc=0), dict(m0=65535)):
        with pytest.raises(ValueError):
            saliency.masked_clips(x, **{**dict(grid=(2, 4, 4), p=0.5, seed=0, clip0=0, m0=0, Mc=1), **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.masked_clips(x.cpu(), (2, 4, 4), 0.5, 0, 0, 0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.saliency_maps(torch.zeros(1, 4, 1), (4, 24, 24), (2, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        saliency.mask_scores(torch.zeros(1, 4, 6), None, torch.zeros(1, 1, dtype=torch.int32), None)
    xi = synth.echo_clips((1, 3, 224, 224)).to(DEV)
    with pytest.raises(NotImplementedError):
        saliency.rise(synth_model(CFG_PPNET).to(DEV).eval(), xi)
    m = synth_model(CFG_XPROTO).to(DEV).eval()
    for bad in (dict(masks=0), dict(masks=65536), dict(target="class", select=2), dict(norm="mean"), dict(maps="float"), dict(max_batch=0), dict(p=0.0)):
        with pytest.raises(ValueError):
            m.rise(xi, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.rise(xi.cpu())
    with pytest.raises(ValueError, match="rise"):
        m.faithfulness(xi, saliency="random", rise=dict(masks=8))
    with pytest.raises(ValueError, match="saliency"):
        m.faithfulness(xi, saliency="blur")
