"""GPU: robustness (csrc/corrupt.hip through protoasnet_amd.robustness) against the numpy restatement of tests/robustness_cases.py: the
corrupted clips bit for bit, the stability statistics against float64, the whole path against the model run on the restatement's clips,
and DPTrainer.evaluate_robustness against its batches."""
import numpy as np
import pytest
import torch

import robustness_cases as rc
from conftest import TOL_LOGITS, TOL_SIM, assert_close
from protoasnet_amd import _lib, robustness, synth
from protoasnet_amd.robustness import Corruption
from test_cpu_trainer import TRAIN_CFG
from util import CFG_PPNET, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _to_device(raw):
    """Raw elements (float32, or bf16 bit patterns as uint16) -> the device tensor."""
    if raw.dtype == np.float32:
        return torch.from_numpy(raw).to(DEV)
    return torch.from_numpy(raw.view(np.int16)).to(DEV).view(torch.bfloat16)


def _raw(t):
    t = t.cpu()
    return t.numpy() if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _assert_bitwise(got, want, what):
    bad = _bits(_raw(got)) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _full(shape, seed):
    """Every stage at once: frame hold, blur, gain + offset per row, both noises."""
    N, C, T, H, W = shape
    rng = np.random.default_rng(seed)
    return Corruption(src_t=rng.integers(-1, T + 1, (N, T)).astype(np.int32),  # (entries outside [0, T) are clamped)
                      taps=robustness.gaussian_taps(1.0), row_a=(0.6 + 0.8 * rng.random(H)).astype(np.float32),
                      row_b=(0.1 * rng.random(H) - 0.05).astype(np.float32), sigma_add=0.05, sigma_mul=0.3)


# ---- 1. pasn_clip_corrupt ------------------------------------------------------------------------------------------------------------------
# "odd": every row off the 16-byte grid; "halo": the plane is smaller than the halo (R = 8); "seams": crosses tile seams both ways
SHAPES = {"odd": (2, 3, 17, 23), "halo": (2, 1, 5, 3), "seams": (1, 2, 70, 150)}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_corrupt_equals_the_restatement_bitwise(name, C, dtype):
    N, T, H, W = SHAPES[name]
    shape = (N, C, T, H, W)
    raw = rc.echo_raw(shape, seed=H + C, bf16=dtype == "bf16")
    raw.reshape(-1)[3] = np.nan if dtype == "fp32" else 0x7FC0  # NaN gives pixel 0
    x = _to_device(raw)
    wide = robustness.gaussian_taps(5.0)  # R = 8
    assert len(wide) == 17
    cases = {"full": _full(shape, 1), "blur_R8": Corruption(taps=wide), "blur_noise": Corruption(taps=wide, sigma_add=0.1, sigma_mul=0.2),
             "plain": Corruption(row_a=np.linspace(1.5, 0.3, H).astype(np.float32), sigma_mul=0.4),
             "offset_only": Corruption(row_b=np.full(H, 0.1, np.float32)), "speckle": Corruption(sigma_mul=0.6)}
    for cname, d in cases.items():
        got = robustness.corrupt(x, d, seed=0xDEADBEEF12345 + C)
        assert got.shape == x.shape and got.dtype == x.dtype
        _assert_bitwise(got, rc.corrupt_ref(raw, seed=0xDEADBEEF12345 + C, **rc.descriptor_kwargs(d)), (name, cname))
    if T == 1:  # an image batch (N, C, H, W) is the same call
        d = cases["blur_noise"]
        got = robustness.corrupt(x[:, :, 0], d, seed=9)
        assert got.shape == (N, C, H, W)
        _assert_bitwise(got, rc.corrupt_ref(raw, seed=9, **rc.descriptor_kwargs(d))[:, :, 0], (name, "image"))


@pytest.mark.parametrize("severity", [1, 5])
@pytest.mark.parametrize("name", list(robustness.CORRUPTIONS))
def test_named_corruptions_equal_the_restatement_bitwise(name, severity):
    shape = (1, 1, 4, 64, 64)
    raw = rc.echo_raw(shape, seed=17)
    x = _to_device(raw)
    got = robustness.corrupt(x, name, severity, seed=23)
    d = robustness.describe(name, severity, shape, seed=23)
    want = rc.corrupt_ref(raw, seed=23, **rc.descriptor_kwargs(d))
    _assert_bitwise(got, want, (name, severity))
    assert not np.array_equal(want, raw) or (name == "frame_hold" and (d.src_t == np.arange(4)).all())  # the corruption does something
    # a non-default normalisation goes through the same arithmetic
    got = robustness.corrupt(x, name, severity, seed=23, mean=0.25, std=0.5)
    _assert_bitwise(got, rc.corrupt_ref(raw, seed=23, mean=0.25, std=0.5, **rc.descriptor_kwargs(d)), (name, severity, "mean/std"))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_all_stages_off_is_the_bitwise_gather_of_frames(dtype):
    shape = (2, 3, 5, 17, 23)
    raw = rc.echo_raw(shape, seed=3, bf16=dtype == "bf16")
    raw.reshape(-1)[[5, 77]] = [np.nan, -0.0] if dtype == "fp32" else [0x7FC1, 0x8000]  # bits survive a copy
    x = _to_device(raw)
    perm = np.stack([np.random.default_rng(n).permutation(5) for n in range(2)]).astype(np.int32)
    got = robustness.corrupt(x, Corruption(src_t=perm), seed=1)
    want = np.stack([raw[n][:, perm[n]] for n in range(2)])
    _assert_bitwise(got, want, "gather")
    _assert_bitwise(robustness.corrupt(x, Corruption()), raw, "identity")
    _assert_bitwise(got, rc.corrupt_ref(raw, src_t=perm), "restatement")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_corrupt_does_not_depend_on_where_the_buffers_lie(dtype):
    shape = (2, 3, 3, 17, 23)
    raw = rc.echo_raw(shape, seed=8, bf16=dtype == "bf16")
    x = _to_device(raw)
    for d in (_full(shape, 2), Corruption(sigma_add=0.1, row_a=np.full(17, 0.7, np.float32))):
        whole = robustness.corrupt(x, d, seed=4)
        # behind a different offset: one element further into a larger buffer (another misalignment of every row)
        for shift in (1, 3):
            buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
            view = buf[shift:shift + x.numel()].view(shape)
            view.copy_(x)
            assert view.is_contiguous() and view.data_ptr() != x.data_ptr()
            assert torch.equal(robustness.corrupt(view, d, seed=4).view(torch.int16 if dtype == "bf16" else torch.int32),
                               whole.view(torch.int16 if dtype == "bf16" else torch.int32)), shift
        # from a non-contiguous view made contiguous
        wide = torch.zeros(shape[:-1] + (shape[-1] + 3,), dtype=x.dtype, device=DEV)
        wide[..., :shape[-1]] = x
        assert torch.equal(robustness.corrupt(wide[..., :shape[-1]], d, seed=4).view(torch.int16 if dtype == "bf16" else torch.int32),
                           whole.view(torch.int16 if dtype == "bf16" else torch.int32))
        # a clip alone: clip n of a batch draws noise stream n, so only clip 0 is comparable
        d0 = Corruption(src_t=None if d.src_t is None else d.src_t[:1], taps=d.taps, row_a=d.row_a, row_b=d.row_b, sigma_add=d.sigma_add,
                        sigma_mul=d.sigma_mul)
        assert torch.equal(robustness.corrupt(x[:1], d0, seed=4).float(), whole[:1].float())


# ---- 2. pasn_stability_stats ---------------------------------------------------------------------------------------------------------------
def _stats_call(case, K_real, k, m, grid, with_labels, acc=None):
    la, lb, sa, sb, oa, ob, labels = case
    N, K = la.shape
    P = sa.shape[1]
    d = [torch.from_numpy(a).to(DEV) for a in (la, lb, sa, sb, oa, ob)]
    lab = torch.from_numpy(labels).to(DEV) if with_labels else None
    clip = torch.empty((N, 4), dtype=torch.float64, device=DEV)
    correct = torch.full((N, 2), -7, dtype=torch.int32, device=DEV)
    sel = torch.empty((N, k), dtype=torch.int32, device=DEV)
    pair = torch.empty((N, k, 4), dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().pasn_stability_stats(*(t.data_ptr() for t in d), _lib.ptr(lab), N, K, K_real, P, grid[0], grid[1], grid[2], k, m,
                                               clip.data_ptr(), correct.data_ptr() if with_labels else 0, sel.data_ptr(), pair.data_ptr(),
                                               _lib.ptr(acc), _lib.current_stream()))
    return clip.cpu().numpy(), correct.cpu().numpy(), sel.cpu().numpy(), pair.cpu().numpy()


@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 7, 7), (16, 7, 7), (16, 16, 16)], ids=["S1", "S49", "S784", "S4096"])
def test_stability_stats_against_float64(grid):
    N, K, G, K_real = 5, 4, 3, 3
    S = int(np.prod(grid))
    case = rc.stats_case(N, K, G, grid, seed=S % 7)  # maps full of ties; planted constant and identical maps
    m = robustness.top_count(0.1, S)
    for k in (1, G):
        for with_labels in (True, False):
            want = rc.stats_ref(*case[:6], case[6] if with_labels else None, K_real, k, m, grid)  # (asserts every variance >= 1e-4 or == 0)
            acc0 = np.arange(robustness.accumulator_size(k), dtype=np.float64) * 0.5
            acc = torch.from_numpy(acc0.copy()).to(DEV)
            clip, correct, sel, pair = _stats_call(case, K_real, k, m, grid, with_labels, acc)
            what = (grid, k, with_labels)
            assert np.array_equal(sel, want["sel"]), what
            assert np.array_equal(clip[:, 0], want["clip"][:, 0]) and np.array_equal(clip[:, 3], want["clip"][:, 3]), what  # flip, overlap
            assert np.array_equal(pair[..., 2], want["pair"][..., 2]), what  # iou: integers in, exact
            if with_labels:
                assert np.array_equal(correct, want["correct"]), what
            else:
                assert (correct == -7).all()  # not touched
            errs = {"tv": np.abs(clip[:, 1] - want["clip"][:, 1]).max(), "drop": np.abs(clip[:, 2] - want["clip"][:, 2]).max(),
                    "dsim": np.abs(pair[..., 0] - want["pair"][..., 0]).max(), "corr": np.abs(pair[..., 1] - want["pair"][..., 1]).max(),
                    "shift": np.abs(pair[..., 3] - want["pair"][..., 3]).max()}
            print(what, {n: f"{float(e):.3g}" for n, e in errs.items()})
            assert max(errs.values()) <= 1e-9, (what, errs)
            assert errs["dsim"] == 0.0  # one exact fp64 difference
            # the planted maps: clip 1 one side constant, clip 2 both, clip 3 identical
            if S > 1:
                assert (pair[1, :, 1] == 0.0).all() and (pair[2, :, 1:] == [1.0, 1.0, 0.0]).all() and (pair[3, :, 1:] == [1.0, 1.0, 0.0]).all()
            else:
                assert (pair[..., 1:] == [1.0, 1.0, 0.0]).all()
            # acc: the device's own rows added in clip order onto the caller's start
            own = {"clip": clip, "correct": correct if with_labels else None, "pair": pair}
            assert np.array_equal(acc.cpu().numpy(), rc.acc_ref(acc0, own, k)), what
            # two calls with the same start are bitwise equal
            acc2 = torch.from_numpy(acc0.copy()).to(DEV)
            again = _stats_call(case, K_real, k, m, grid, with_labels, acc2)
            assert all(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
                       for a, b in zip((clip, correct, sel, pair), again))
            assert torch.equal(acc.view(torch.int64), acc2.view(torch.int64))
    assert 0 < want["clip"][:, 0].sum() < N  # the case flips some predictions and keeps others


def test_stability_refuses_a_map_too_large_for_lds():
    case = rc.stats_case(4, 4, 3, (1, 1, 1), seed=0)
    with pytest.raises(RuntimeError, match="4096"):
        _stats_call(case, 3, 1, 1, (1, 64, 65), True)


def test_stability_and_explain_rank_select_the_same_prototypes():
    """pasn_stability_stats (robustness) and pasn_explain_rank (explanations, faithfulness) report the same predicted class and the same
    k best prototypes: distinct values, a tie across rank k - 1 / k, an all-equal block, NaN logits, all-equal logits."""
    from explain_cases import rank_ref
    from test_gpu_explain import _rank

    logits, sim, occ, fc_w, pred_hand, sel_hand = rc.agreement_case()
    K_real, G, k = rc.AGREE_K_REAL, rc.AGREE_G, rc.AGREE_SELECT
    _, _, sel_s, _ = _stats_call((logits, logits, sim, sim, occ, occ, None), K_real, k, 1, rc.AGREE_GRID, False)
    _, _, _, _, pred_e, sel_e = _rank(*(torch.from_numpy(a) for a in (sim, fc_w, logits)), K_real, k)
    pred_e, sel_e = pred_e.cpu().numpy(), sel_e.cpu().numpy()
    _, _, _, _, pred_r, sel_r = rank_ref(sim, fc_w, logits, K_real, k)
    assert np.array_equal(sel_s, sel_e), (sel_s, sel_e)
    assert np.array_equal(sel_s[:, 0] // G, pred_e)
    assert np.array_equal(sel_s, sel_r.numpy()) and np.array_equal(pred_e, pred_r.numpy())
    assert np.array_equal(pred_e, pred_hand) and np.array_equal(sel_s[:3], sel_hand)


# ---- 3. the whole path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,shape", [(CFG_VIDEO_X3D, (2, 3, 4, 64, 64)), (CFG_XPROTO, (2, 3, 224, 224))], ids=["x3d_s", "xprotonet_image"])
def test_model_robustness_end_to_end(cfg, shape):
    m = synth_model(cfg).to(DEV).eval()
    x = synth.echo_clips(shape).to(DEV)
    labels = torch.tensor([0, 1])
    k = 2
    shape5 = robustness._geometry(shape)
    raw5 = x.cpu().numpy().reshape(shape5)
    d = Corruption(taps=robustness.gaussian_taps(1.5), row_a=np.linspace(1.0, 0.4, shape5[3]).astype(np.float32), sigma_add=0.08, sigma_mul=0.3)
    got = m.robustness(x, d, seed=5, select=k, labels=labels)
    xc = torch.from_numpy(rc.corrupt_ref(raw5, seed=5, **rc.descriptor_kwargs(d)).reshape(shape)).to(DEV)
    want = robustness.stability(m, x, xc, select=k, labels=labels)
    with torch.no_grad():
        _, dist_a, occ_a, logits_a = m.push_forward(x)
        _, dist_b, occ_b, logits_b = m.push_forward(xc)
    S = int(np.prod(occ_a.shape[3:]))
    assert got.m == robustness.top_count(0.1, S) == want.m and got.dsim.shape == (2, k) and got.dsim.dtype == torch.float64
    for f in ("flip", "overlap", "selected", "iou", "shift", "correct"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert_close(got.dsim, want.dsim, TOL_SIM, name="dsim")
    assert_close(got.corr, want.corr, TOL_SIM, name="corr")
    assert_close(got.tv, want.tv, TOL_LOGITS, name="tv")
    assert_close(got.prob_drop, want.prob_drop, TOL_LOGITS, name="prob_drop")
    # against torch on the two forwards
    K_real = m.num_classes - 1
    pa, pb = logits_a[:, :K_real].softmax(1).double(), logits_b[:, :K_real].softmax(1).double()
    pred = logits_a[:, :K_real].argmax(1)
    assert_close(got.tv, 0.5 * (pa - pb).abs().sum(1), TOL_LOGITS, name="tv vs torch")
    assert_close(got.prob_drop, (pa - pb).gather(1, pred[:, None])[:, 0], TOL_LOGITS, name="drop vs torch")
    assert torch.equal(got.flip, (logits_b[:, :K_real].argmax(1) != pred).double())
    assert torch.equal(got.correct[:, 0].long().cpu(), (pred.cpu() == labels).long())
    sel = got.selected.long()
    assert_close(got.dsim, ((1 - dist_b) - (1 - dist_a)).gather(1, sel), TOL_SIM, name="dsim vs torch")
    N, P = occ_a.shape[:2]
    oa, ob = occ_a.reshape(N, P, S), occ_b.reshape(N, P, S)
    for n in range(N):
        for j in range(k):
            cc = torch.corrcoef(torch.stack([oa[n, sel[n, j]], ob[n, sel[n, j]]]).double())[0, 1]
            assert abs(float(cc) - float(got.corr[n, j])) <= 1e-6, (n, j)
    print("corruption moved: tv", got.tv.tolist(), "corr", got.corr.tolist(), "iou", got.iou.tolist())
    assert float(got.tv.max()) > 0 and float(got.corr.min()) < 1  # the corruption is felt
    # every stage off: the same clip twice
    same = m.robustness(x, Corruption(), select=k, labels=labels)
    zero, one = torch.zeros(2, dtype=torch.float64, device=DEV), torch.ones((2, k), dtype=torch.float64, device=DEV)
    assert torch.equal(same.flip, zero) and torch.equal(same.tv, zero) and torch.equal(same.prob_drop, zero) and torch.equal(same.overlap, one[:, 0])
    assert torch.equal(same.corr, one) and torch.equal(same.iou, one) and torch.equal(same.shift, 0 * one) and torch.equal(same.dsim, 0 * one)
    assert torch.equal(same.correct[:, 0], same.correct[:, 1])
    # a named corruption, by name
    if len(shape) == 5:
        held = m.robustness(x, "frame_hold", 5, seed=1)
        assert held.dsim.shape == (2, 1) and held.correct is None
    else:
        with pytest.raises(ValueError, match="more than one frame"):
            m.robustness(x, "frame_hold", 5)


def test_refusals_on_the_device():
    x = synth.echo_clips((1, 3, 224, 224)).to(DEV)
    with pytest.raises(NotImplementedError, match="robustness evaluation covers"):
        robustness.robustness(synth_model(CFG_PPNET).to(DEV).eval(), x, "noise", 1)
    m = synth_model(CFG_XPROTO).to(DEV)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.robustness(x, "noise", 1)
    m.eval()
    with pytest.raises(ValueError, match="select"):
        m.robustness(x, "noise", 1, select=99)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        robustness.corrupt(x[:, :2], "noise", 1)
    with pytest.raises(ValueError, match="taps"):
        robustness.corrupt(x, Corruption(taps=np.ones(19, np.float32) / 19))
    with pytest.raises(ValueError, match="row_a"):
        robustness.corrupt(x, Corruption(row_a=np.ones(7, np.float32)))
    with pytest.raises(TypeError):
        robustness.corrupt(x.to(torch.float16), "noise", 1)


# ---- 4. the sweep --------------------------------------------------------------------------------------------------------------------------
def _flat(res):
    out = [np.asarray(res["clips"])]
    for name, by_severity in res["cells"].items():
        for sev, c in by_severity.items():
            out += [np.asarray(c[f]) for f in ("acc_clean", "acc_corrupted", "flip_rate", "tv", "prob_drop", "overlap", "dsim", "corr", "iou", "shift")]
    return out


def test_trainer_evaluate_robustness():
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    batches = [{"cine": synth.echo_clips((2, 3, 4, 64, 64), seed=90 + b), "target_AS": torch.tensor([b, 1]), "filename": [f"a{b}", f"b{b}"]}
               for b in range(2)]
    logs = []
    t = DPTrainer(m, {"abstain_class": True, "train": TRAIN_CFG}, {"train": batches, "val": batches}, log=lambda s, *_: logs.append(str(s)))
    m.train()
    names, sevs = ("noise", "blur", "frame_hold", "attenuation"), (1, 5)
    res = t.evaluate_robustness("val", corruptions=names, severities=sevs, select=2, seed=7)
    assert m.training  # left in the mode it was in
    lines = [s for s in logs if "robustness" in s]
    assert len(lines) == len(names) * len(sevs) and all(any(f"{n} severity {s} " in ln for ln in lines) for n in names for s in sevs)
    again = t.evaluate_robustness("val", corruptions=names, severities=sevs, select=2, seed=7)
    assert all(np.array_equal(a, b) for a, b in zip(_flat(res), _flat(again)))
    m.eval()
    acc = robustness.RobustnessAccumulator(m, corruptions=names, severities=sevs, select=2, seed=7, abstain_class=True)
    for b in batches:
        acc.update(t.prepare_input(b["cine"]), b["target_AS"])
    own = acc.result()
    assert res["clips"] == own["clips"] == 4 and list(res["cells"]) == list(names) and list(res["cells"]["blur"]) == list(sevs)
    assert all(np.array_equal(a, b) for a, b in zip(_flat(res), _flat(own)))
    cell = res["cells"]["noise"][5]
    assert cell["dsim"].shape == (2,) and 0.0 <= cell["flip_rate"] <= 1.0 and cell["acc_clean"] == res["cells"]["blur"][1]["acc_clean"]
    # ... and the float64 combination of the batches' own statistics
    rows = [robustness.robustness(m, t.prepare_input(b["cine"]), "noise", 5, seed=7 + i, select=2, labels=b["target_AS"])
            for i, b in enumerate(batches)]
    for f, key in (("tv", "tv"), ("flip", "flip_rate"), ("prob_drop", "prob_drop"), ("overlap", "overlap"), ("corr", "corr"), ("iou", "iou")):
        want = torch.cat([getattr(r, f) for r in rows]).cpu().numpy().sum(0) / 4.0
        assert np.abs(np.asarray(cell[key]) - want).max() <= 1e-12, f
    assert cell["acc_corrupted"] == float(torch.cat([r.correct for r in rows])[:, 1].sum()) / 4.0
    # the defaults (every corruption, severities 1, 3, 5), ended by max_clips
    m.train()
    three = t.evaluate_robustness("val", max_clips=3)
    assert three["clips"] == 3 and list(three["cells"]) == list(robustness.CORRUPTIONS) and list(three["cells"]["gain_up"]) == [1, 3, 5]
    # PPNet has no occurrence maps
    tp = DPTrainer(synth_model(CFG_PPNET).to(DEV), {"abstain_class": False, "train": TRAIN_CFG}, {"train": [], "val": []}, log=lambda *_: None)
    with pytest.raises(NotImplementedError, match="robustness evaluation covers XProtoNet and Video_XProtoNet"):
        tp.evaluate_robustness("val")
