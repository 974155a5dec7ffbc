"""GPU: explanation faithfulness (csrc/perturb.hip through protoasnet_amd.faithfulness) against the numpy restatement of
tests/faithfulness_cases.py: the step volumes and the perturbed clips bit for bit, the curves against float64, the whole path against the
model run on the restatement's clips, and DPTrainer.evaluate_faithfulness against its batches."""
import numpy as np
import pytest
import torch

import faithfulness_cases as fc
from conftest import TOL_LOGITS, TOL_SIM, assert_close
from protoasnet_amd import _lib, explain, faithfulness, synth
from test_cpu_trainer import TRAIN_CFG
from util import CFG_PPNET, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"

# voxel grid, clips, maps per clip.  "odd": V = 2737 is odd, every row but the first starts off the 16-byte grid, and V < one tile;
# "image": no frame axis, V = 1665 odd; "small" / "mid": 2 and 13 tiles per map, V a multiple of 16; "real": the X3D-S clip, 196 tiles.
GRIDS = {"odd": ((7, 17, 23), 2, 3), "small": ((8, 28, 28), 2, 3), "image": ((37, 45), 2, 3), "mid": ((4, 112, 112), 2, 3),
         "real": ((16, 224, 224), 2, 1)}


@pytest.fixture(scope="module")
def occurrence():
    """The occurrence maps of two synth models, (N, P, Ti, Hi, Wi) on the device: what pasn_explain_maps renders at any clip grid."""
    out = {}
    for key, cfg, shape in (("video", CFG_VIDEO_X3D, (2, 3, 4, 64, 64)), ("image", CFG_XPROTO, (2, 3, 224, 224))):
        m = synth_model(cfg).to(DEV).eval()
        with torch.no_grad():
            _, _, occ, _ = m.push_forward(synth.echo_clips(shape).to(DEV))
        N, P = occ.shape[:2]
        out[key] = occ.reshape((N, P) + (tuple(occ.shape[3:]) if key == "video" else (1,) + tuple(occ.shape[3:]))).contiguous()
    return out


def _device_maps(occurrence, grid, N, k):
    """The device's own uint8 explanation maps of the synth models' occurrence maps, rendered at `grid`: (N k, V) on the host."""
    occ = occurrence["video" if len(grid) == 3 else "image"][:N]
    sel = (torch.arange(N * k, dtype=torch.int32, device=DEV).reshape(N, k) * 3) % occ.shape[1]
    out = grid if len(grid) == 3 else (1,) + grid
    maps, _ = explain._maps_launch(occ, sel, k, out, "uint8", None, None, 0.3, 0.0, 1.0)
    return maps.reshape(N * k, -1).cpu().numpy()


# ---- 1. pasn_perturb_steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_removal_steps_equal_the_restatement(name, occurrence):
    grid, N, k = GRIDS[name]
    V, M = int(np.prod(grid)), N * k
    maps = fc.synthetic_maps(M, V, seed=len(name))
    maps["device"] = _device_maps(occurrence, grid, N, k)
    assert len(np.unique(maps["device"])) > 16  # a heat map, not a constant
    for mname, mp in maps.items():
        pos = fc.positions(mp)  # one sort per map, shared by every set of counts
        d_maps = torch.from_numpy(mp).to(DEV).reshape((N, k) + grid)
        for cname, counts in fc.count_sets(V).items():
            got = faithfulness.removal_steps(d_maps, counts)
            want = torch.from_numpy(fc.steps_of_positions(pos, counts)).to(DEV).reshape(got.shape)
            assert got.dtype == torch.uint8 and got.shape == d_maps.shape
            bad = got != want
            assert not bool(bad.any()), (name, mname, cname, int(bad.sum()), bad.reshape(M, V).nonzero()[:4].tolist())
            # for every s exactly counts[s] voxels have steps <= s
            hist = torch.stack([torch.bincount(r, minlength=65) for r in got.reshape(M, V).int()])
            touched = hist.cumsum(1)[:, :len(counts)].cpu()
            assert torch.equal(touched, torch.tensor(counts).expand(M, -1)), (name, mname, cname)
            if counts[-1] < V:
                assert int(got.max()) == len(counts)  # the voxels no step touches


def test_removal_steps_do_not_depend_on_where_the_maps_lie():
    """The same maps behind a different number of rows (another misalignment of every row) and from a non-contiguous view."""
    grid, V = (7, 17, 23), 7 * 17 * 23
    rng = np.random.default_rng(5)
    mp = torch.from_numpy(rng.integers(0, 256, (5, 1, V), dtype=np.uint8)).to(DEV)
    counts = faithfulness.step_counts(V, 7)
    whole = faithfulness.removal_steps(mp.reshape((5, 1) + grid), counts)
    for m in range(5):
        alone = faithfulness.removal_steps(mp[m:m + 1].reshape((1, 1) + grid), counts)
        assert torch.equal(alone[0], whole[m]), m
    wide = torch.zeros((5, 1, V + 3), dtype=torch.uint8, device=DEV)
    wide[:, :, :V] = mp
    assert torch.equal(faithfulness.removal_steps(wide[:, :, :V].reshape((5, 1) + grid), counts), whole)


# ---- 2. pasn_perturb_apply -----------------------------------------------------------------------------------------------------------------
def _raw(t):
    """The bit patterns of a device tensor, on the host: float32 as it is (np.where copies bits), bf16 as uint16."""
    t = t.cpu()
    return t.numpy() if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("grid", [(7, 17, 23), (8, 28, 28)], ids=["odd", "small"])
def test_perturb_equals_the_restatement_bitwise(grid, C, dtype):
    N, k, V = 2, 2, int(np.prod(grid))
    rng = np.random.default_rng(V + C)
    counts = [0, V // 5, V // 2, V - 3]  # step 4 = S1: the three voxels nothing touches
    steps_np = fc.steps_ref(rng.integers(0, 256, (N * k, V), dtype=np.uint8), counts).reshape(N, k, V)
    assert steps_np.max() == 4 and steps_np.min() == 1  # counts[0] = 0: no voxel has step 0
    steps = torch.from_numpy(steps_np).to(DEV).reshape((N, k) + grid)
    x = torch.from_numpy(rng.standard_normal((N, C) + grid).astype(np.float32)).to(DEV).to(dtype)
    x.view(-1)[3], x.view(-1)[V + 1], x.view(-1)[-1] = float("nan"), -0.0, float("inf")
    base = torch.from_numpy(rng.standard_normal((N, C) + grid).astype(np.float32)).to(DEV).to(dtype)
    ids = [3, 1, 2]  # a strict, unordered subset of the steps 0 .. 3
    fill = -0.7173  # not a bf16 number: rounded once, to nearest even
    fill_raw = _raw(torch.tensor([fill], dtype=dtype))[0]
    for mode in (0, 1):
        for baseline in (None, base):
            got = faithfulness.perturb(x, steps, ids, faithfulness.MODES[mode], baseline=baseline, fill=fill)
            assert got.shape == (N, k, len(ids), C) + grid and got.dtype == dtype
            want = fc.apply_ref(_raw(x).reshape(N, C, V), steps_np, ids, mode, None if baseline is None else _raw(base).reshape(N, C, V),
                                fill_raw)
            g = _bits(_raw(got).reshape(want.shape))
            bad = g != _bits(want)
            assert not bad.any(), (mode, baseline is not None, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # step ids as a device tensor, the mode by number
    again = faithfulness.perturb(x, steps, torch.tensor(ids, dtype=torch.int32, device=DEV), 1, baseline=base)
    assert np.array_equal(_bits(_raw(again)), _bits(_raw(got)))


# ---- 3. pasn_perturb_curves ----------------------------------------------------------------------------------------------------------------
def test_curves_kernel_against_float64():
    N, k, S1, P, K, K_real, V = 3, 2, 5, 12, 4, 3, 1000
    counts = [0, 100, 100, 450, 1000]
    rng = np.random.default_rng(21)
    lib = _lib.lib()
    d_counts = torch.tensor(counts, dtype=torch.int32, device=DEV)
    acc = torch.zeros(faithfulness.accumulator_size(k, S1), dtype=torch.float64, device=DEV)
    want_acc = np.zeros(acc.numel())
    for call in range(2):
        sim = rng.random((N, k, S1, P), dtype=np.float32)
        logits = (4 * rng.standard_normal((N, k, S1, K))).astype(np.float32)
        sel = rng.integers(0, P, (N, k)).astype(np.int32)
        cls = rng.integers(0, K_real, N).astype(np.int32)
        d = [torch.from_numpy(a).to(DEV) for a in (sim, logits, sel, cls)]
        cs = torch.empty((N, k, S1), dtype=torch.float32, device=DEV)
        cp = torch.empty_like(cs)
        auc = torch.empty((N, k, 2), dtype=torch.float64, device=DEV)
        _lib.check(lib.pasn_perturb_curves(*(t.data_ptr() for t in d), d_counts.data_ptr(), N, k, S1, P, K, K_real, V, cs.data_ptr(),
                                           cp.data_ptr(), auc.data_ptr(), acc.data_ptr(), _lib.current_stream()))
        cs, cp, auc = cs.cpu().numpy(), cp.cpu().numpy(), auc.cpu().numpy()
        r_cs, r_cp, _ = fc.curves_ref(sim, logits, sel, cls, counts, V, K_real)
        assert np.array_equal(cs.view(np.uint32), r_cs.view(np.uint32))  # a copy
        e_prob = float(np.abs(cp - r_cp).max())
        # fp32 softmax of at most 8 terms, values <= 1
        own = np.stack([fc.trapezoid(cs, counts, V), fc.trapezoid(cp, counts, V)], -1)  # of the kernel's own curves
        e_auc = float((np.abs(auc - own) / np.abs(own)).max())
        print(f"call {call}: max |prob - float64| = {e_prob:.3g}, max rel |auc - trapezoid| = {e_auc:.3g}")
        assert e_prob <= 1e-6 and e_auc <= 1e-12
        for n in range(N):  # clips in ascending order, as the kernel adds them
            want_acc[:k * S1] += cs[n].reshape(-1).astype(np.float64)
            want_acc[k * S1:2 * k * S1] += cp[n].reshape(-1).astype(np.float64)
            want_acc[2 * k * S1:-1] += auc[n].reshape(-1)
        want_acc[-1] += N
    assert np.array_equal(acc.cpu().numpy(), want_acc)
    # an index outside its range reads nothing: NaN curves for that clip only
    sel[1, 0], cls[2] = P, -1
    d = [torch.from_numpy(a).to(DEV) for a in (sim, logits, sel, cls)]
    cs = torch.empty((N, k, S1), dtype=torch.float32, device=DEV)
    cp, auc = torch.empty_like(cs), torch.empty((N, k, 2), dtype=torch.float64, device=DEV)
    _lib.check(lib.pasn_perturb_curves(*(t.data_ptr() for t in d), d_counts.data_ptr(), N, k, S1, P, K, K_real, V, cs.data_ptr(), cp.data_ptr(),
                                       auc.data_ptr(), 0, _lib.current_stream()))
    nan = torch.isnan(cs).all(-1).cpu()
    assert nan.tolist() == [[False, False], [True, False], [True, True]] and torch.equal(torch.isnan(cp).all(-1).cpu(), nan)


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,shape", [(CFG_VIDEO_X3D, (2, 3, 4, 64, 64)), (CFG_XPROTO, (2, 3, 224, 224))], ids=["x3d_s", "xprotonet_image"])
def test_perturbation_curves_end_to_end(cfg, shape):
    m = synth_model(cfg).to(DEV).eval()
    x = synth.echo_clips(shape).to(DEV)
    N, C, grid = shape[0], shape[1], tuple(shape[2:])
    V, k, S = int(np.prod(grid)), 2, 4
    K_real = m.num_classes - 1
    counts = faithfulness.step_counts(V, S)
    pair = m.faithfulness(x, select=k, steps=S, mode="both")
    e = m.explain(x, select=k, maps="uint8")
    with torch.no_grad():
        logits0, sim0, _ = m(x)
    dele, ins = pair.deletion, pair.insertion
    assert torch.equal(dele.selected, e.selected) and torch.equal(dele.pred, e.pred) and torch.equal(dele.steps, ins.steps)
    assert dele.fractions.tolist() == [c / V for c in counts] and dele.fractions.dtype == torch.float64
    # the restatement's step volume and clips of the device's maps, through the model in the same batch layout
    steps_np = fc.steps_ref(e.maps.reshape(N * k, V).cpu().numpy(), counts).reshape(N, k, V)
    assert np.array_equal(dele.steps.reshape(N, k, V).cpu().numpy(), steps_np)
    sel, pred = e.selected.long(), e.pred.long()
    for mode, cur in ((0, dele), (1, ins)):
        clips = fc.apply_ref(x.reshape(N, C, V).cpu().numpy(), steps_np, list(range(S + 1)), mode, fill=np.float32(0.0))
        with torch.no_grad():
            logits, sim, _ = m(torch.from_numpy(clips).to(DEV).reshape((N * k * (S + 1), C) + grid))
        want_sim = sim.reshape(N, k, S + 1, -1).gather(3, sel[:, :, None, None].expand(N, k, S + 1, 1))[..., 0]
        probs = logits.reshape(N, k, S + 1, -1)[..., :K_real].softmax(-1)
        want_prob = probs.gather(3, pred[:, None, None, None].expand(N, k, S + 1, 1))[..., 0]
        assert cur.similarity.shape == (N, k, S + 1) and cur.similarity.dtype == torch.float32
        assert_close(cur.similarity, want_sim, TOL_SIM, name=f"{cur.mode} similarity")
        assert_close(cur.prob, want_prob, TOL_LOGITS, name=f"{cur.mode} prob")
        own = np.stack([fc.trapezoid(cur.similarity.cpu().numpy(), counts, V), fc.trapezoid(cur.prob.cpu().numpy(), counts, V)])
        got = np.stack([cur.auc_similarity.cpu().numpy(), cur.auc_prob.cpu().numpy()])
        assert cur.auc_prob.dtype == torch.float64 and float((np.abs(got - own) / np.abs(own)).max()) <= 1e-12
    # step 0 of the deletion and step S of the insertion are the untouched clip
    clean_sim = sim0.gather(1, sel)
    clean_prob = logits0[:, :K_real].softmax(1).gather(1, pred[:, None]).expand(N, k)
    for name, cur, s in (("deletion step 0", dele, 0), ("insertion step S", ins, S)):
        assert_close(cur.similarity[..., s], clean_sim, TOL_SIM, name=name + " similarity")
        assert_close(cur.prob[..., s], clean_prob, TOL_LOGITS, name=name + " prob")
    # step S of the deletion and step 0 of the insertion are the baseline: the same clip, the same scores
    print("baseline ends differ by", float((dele.similarity[..., S] - ins.similarity[..., 0]).abs().max()),
          float((dele.prob[..., S] - ins.prob[..., 0]).abs().max()))
    assert torch.equal(dele.similarity[..., S], ins.similarity[..., 0]) and torch.equal(dele.prob[..., S], ins.prob[..., 0])
    # a caller's maps: the device's own, handed back, give the same curves
    mine = faithfulness.perturbation_curves(m, x, select=k, steps=S, mode="deletion", saliency=e.maps)
    assert torch.equal(mine.similarity, dele.similarity) and torch.equal(mine.prob, dele.prob)
    # smaller forwards: 8 = both clips, chunks of two steps, the last one padded; 3 = one clip and one step at a time
    for max_batch in (8, 3):
        alt = m.faithfulness(x, select=k, steps=S, mode="deletion", max_batch=max_batch)
        assert_close(alt.similarity, dele.similarity, TOL_SIM, name=f"max_batch={max_batch} similarity")
        assert_close(alt.prob, dele.prob, TOL_LOGITS, name=f"max_batch={max_batch} prob")
    # the random control: one seed is one volume, two seeds are two
    r0 = faithfulness.perturbation_curves(m, x, select=k, steps=S, mode="insertion", saliency="random", seed=3)
    r1 = faithfulness.perturbation_curves(m, x, select=k, steps=S, mode="insertion", saliency="random", seed=3)
    r2 = faithfulness.perturbation_curves(m, x, select=k, steps=S, mode="insertion", saliency="random", seed=4)
    assert torch.equal(r0.steps, r1.steps) and torch.equal(r0.similarity, r1.similarity) and torch.equal(r0.prob, r1.prob)
    assert torch.equal(r0.auc_prob, r1.auc_prob) and not torch.equal(r0.steps, r2.steps)


def test_refusals_on_the_device():
    x = synth.echo_clips((1, 3, 224, 224)).to(DEV)
    with pytest.raises(NotImplementedError):
        faithfulness.perturbation_curves(synth_model(CFG_PPNET).to(DEV).eval(), x)
    m = synth_model(CFG_XPROTO).to(DEV)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.faithfulness(x)
    m.eval()
    with pytest.raises(ValueError, match="mode"):
        m.faithfulness(x, mode="blur")
    with pytest.raises(ValueError, match="saliency"):
        m.faithfulness(x, saliency=torch.zeros((1, 1, 224, 223), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        faithfulness.removal_steps(torch.zeros((1, 1, 4, 4), dtype=torch.uint8, device=DEV), [3, 2])


# ---- 5. the sweep --------------------------------------------------------------------------------------------------------------------------
def _flat(res):
    out = [np.asarray(res["fractions"]), np.asarray(res["clips"])]
    for d in (res["deletion"], res["insertion"], res["random"]["deletion"], res["random"]["insertion"]):
        out += [d[a] for a in ("similarity", "prob", "auc_similarity", "auc_prob")]
    for d in (res["difference"]["deletion"], res["difference"]["insertion"]):
        out += [d[a] for a in ("auc_similarity", "auc_prob")]
    return out


def test_trainer_evaluate_faithfulness():
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    batches = [{"cine": synth.echo_clips((2, 3, 4, 64, 64), seed=90 + b), "target_AS": torch.tensor([b, 1]), "filename": [f"a{b}", f"b{b}"]}
               for b in range(2)]
    logs = []
    t = DPTrainer(m, {"abstain_class": True, "train": TRAIN_CFG}, {"train": batches, "val": batches}, log=lambda s, *_: logs.append(str(s)))
    m.train()
    res = t.evaluate_faithfulness("val", steps=4, select=2, seed=7)
    assert m.training and any("faithfulness" in s for s in logs)  # left in the mode it was in
    again = t.evaluate_faithfulness("val", steps=4, select=2, seed=7)
    assert all(np.array_equal(a, b) for a, b in zip(_flat(res), _flat(again)))
    m.eval()
    k, S1 = 2, 5
    assert res["clips"] == 4 and res["deletion"]["similarity"].shape == (k, S1) and res["random"]["insertion"]["auc_prob"].shape == (k,)
    # the float64 combination of the batches' own curves
    for kind, saliency in (("model", None), ("random", "random")):
        pairs = [faithfulness.perturbation_curves(m, t.prepare_input(b["cine"]), select=k, steps=4, mode="both", saliency=saliency, seed=7 + i)
                 for i, b in enumerate(batches)]
        for mode in faithfulness.MODES:
            got = res[mode] if kind == "model" else res["random"][mode]
            for field in ("similarity", "prob", "auc_similarity", "auc_prob"):
                rows = np.concatenate([getattr(getattr(p, mode), field).double().cpu().numpy() for p in pairs])  # (clips, k[, S1])
                want = rows.sum(0) / 4.0
                err = float((np.abs(got[field] - want) / np.abs(want)).max())
                assert err <= 1e-12, (kind, mode, field, err)
    d = res["difference"]["deletion"]["auc_prob"]
    assert np.array_equal(d, res["deletion"]["auc_prob"] - res["random"]["deletion"]["auc_prob"])
    two = t.evaluate_faithfulness("val", steps=4, select=2, seed=7, max_clips=3)
    assert two["clips"] == 3
