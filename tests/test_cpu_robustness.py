"""CPU: robustness -- the C-ABI / Python surface with its argument checks (no device), the severity tables, and the numpy restatement of
tests/robustness_cases.py (what the GPU tests hold the kernels to) against hand-made cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import protoasnet_amd
import robustness_cases as rc
from protoasnet_amd import _lib, model_builder, robustness
from util import CFG_PPNET, CFG_XPROTO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_clip_corrupt", "pasn_stability_stats")
ARG, UNSUPPORTED = 1, 3


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
    assert "pasn_corrupt_desc" in header and ctypes.sizeof(_lib.CorruptDesc) == 64
    assert "robustness" in protoasnet_amd.__all__ and protoasnet_amd.robustness is robustness
    assert "corrupt.hip" in protoasnet_amd.build.SOURCES
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        assert "NOT a Gaussian" in f.read()  # the header says what z is not


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def corrupt(N=2, C=3, T=4, H=64, W=64, dtype=_lib.F32, x=fake, y=fake, desc=True, **fields):
        d = _lib.CorruptDesc(src_t=None, taps=None, row_a=None, row_b=None, seed=0, R=0, sigma_add=0.0, sigma_mul=0.0, mean=0.099, stdv=0.171)
        for key, v in fields.items():
            setattr(d, key, v)
        return lib.pasn_clip_corrupt(x, y, N, C, T, H, W, dtype, ctypes.byref(d) if desc else None, 0)

    for bad in (dict(x=0), dict(y=0), dict(desc=False), dict(R=9, taps=fake), dict(R=-1, taps=fake), dict(R=2), dict(C=2), dict(C=0), dict(C=4),
                dict(N=0), dict(T=0), dict(H=0), dict(W=-1), dict(dtype=_lib.U8), dict(dtype=_lib.I32), dict(x=258),
                dict(N=1 << 16, T=1 << 16)):
        assert corrupt(**bad) == ARG, bad
    with pytest.raises(ValueError, match="R must lie"):
        _lib.check(corrupt(R=9, taps=fake))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        _lib.check(corrupt(C=2))

    def stats(N=2, K=4, K_real=3, P=12, grid=(1, 7, 7), k=2, m=5, **null):
        p = dict(logits_a=fake, logits_b=fake, sim_a=fake, sim_b=fake, occ_a=fake, occ_b=fake, labels=0, clip=fake, correct=0, sel=fake,
                 pair=fake, acc=0)
        p.update(null)
        return lib.pasn_stability_stats(p["logits_a"], p["logits_b"], p["sim_a"], p["sim_b"], p["occ_a"], p["occ_b"], p["labels"], N, K,
                                        K_real, P, grid[0], grid[1], grid[2], k, m, p["clip"], p["correct"], p["sel"], p["pair"], p["acc"], 0)

    for key in ("logits_a", "logits_b", "sim_a", "sim_b", "occ_a", "occ_b", "clip", "sel", "pair"):
        assert stats(**{key: 0}) == ARG, key
    for bad in (dict(N=0), dict(N=65536), dict(P=13), dict(P=0), dict(K=0), dict(K_real=0), dict(K_real=5), dict(k=0), dict(k=4), dict(m=0),
                dict(m=50), dict(grid=(0, 7, 7)), dict(grid=(1, 7, -1)), dict(labels=fake), dict(P=32768, K=4)):
        assert stats(**bad) == ARG, bad
    assert stats(grid=(1, 64, 65)) == UNSUPPORTED and stats(grid=(17, 16, 16), m=1) == UNSUPPORTED
    with pytest.raises(RuntimeError, match="4096"):
        _lib.check(stats(grid=(1, 64, 65)))
    with pytest.raises(ValueError, match="k must lie"):
        _lib.check(stats(k=4))


def test_python_surface_refuses_what_it_cannot_run():
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(NotImplementedError, match="robustness evaluation covers XProtoNet and Video_XProtoNet"):
        robustness.robustness(model_builder.build(CFG_PPNET).eval(), x, "noise", 1)
    m = model_builder.build(CFG_XPROTO).eval()
    assert m.robustness.__func__ is type(m).robustness  # on the head-B mixin, next to faithfulness
    with pytest.raises(RuntimeError, match="GPU only"):
        m.robustness(x, "noise", 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        robustness.corrupt(x, "noise", 1)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.robustness(x, "noise", 1)
    with pytest.raises(ValueError, match="unknown corruption"):
        robustness.describe("fog", 1, x.shape)
    for sev in (0, 6, 1.0, True, None):
        with pytest.raises(ValueError, match="severity"):
            robustness.describe("noise", sev, x.shape)
    with pytest.raises(ValueError, match="more than one frame"):
        robustness.describe("frame_hold", 1, x.shape)
    with pytest.raises(ValueError):
        robustness.RobustnessAccumulator(m, corruptions=["fog"])
    assert robustness.accumulator_size(2) == 6 + 4 * 2 + 1
    assert [robustness.top_count(0.1, S) for S in (1, 49, 784, 4096)] == [1, 5, 79, 410] and robustness.top_count(1.0, 7) == 7
    with pytest.raises(ValueError):
        robustness.top_count(0.0, 49)


# ---- the severity tables -------------------------------------------------------------------------------------------------------------------
def test_corruption_table_is_the_definition_and_monotone():
    want = {"gain_down": (.8, .65, .5, .35, .2), "gain_up": (1.25, 1.5, 1.75, 2., 2.5), "contrast": (.8, .65, .5, .35, .2),
            "attenuation": (.5, 1., 1.5, 2., 3.), "noise": (.02, .04, .08, .12, .16), "speckle": (.1, .2, .3, .45, .6),
            "blur": (.5, .75, 1., 1.5, 2.), "frame_hold": (.1, .2, .3, .4, .5)}
    assert {k: v[0] for k, v in robustness.CORRUPTIONS.items()} == want
    for name, (values, _) in robustness.CORRUPTIONS.items():
        d = np.diff(values)
        assert (d > 0).all() or (d < 0).all(), name  # strictly harsher with the severity
    shape = (2, 3, 8, 16, 12)
    d = robustness.describe("gain_down", 2, shape)
    assert d.row_a.dtype == np.float32 and d.row_a.tolist() == [np.float32(.65)] * 16 and d.row_b is None and d.taps is None
    d = robustness.describe("contrast", 5, shape)
    assert d.row_a.tolist() == [np.float32(.2)] * 16 and d.row_b.tolist() == [np.float32(.4)] * 16
    d = robustness.describe("attenuation", 5, shape)
    assert d.row_a[0] == 1.0 and d.row_a[-1] == np.float32(np.exp(-3.0)) and (np.diff(d.row_a) < 0).all()
    assert d.row_a[5] == np.float32(np.exp(np.float64(-3.0) * 5 / 15))  # float64 on the host, one rounding
    assert robustness.describe("noise", 3, shape).sigma_add == .08 and robustness.describe("speckle", 4, shape).sigma_mul == .45


def test_blur_taps_sum_to_one_and_are_symmetric():
    radii = []
    for sigma in robustness.CORRUPTIONS["blur"][0] + (5.0,):
        t = robustness.gaussian_taps(sigma)
        R = (len(t) - 1) // 2
        radii.append(R)
        assert t.dtype == np.float32 and len(t) == 2 * R + 1 and R == min(8, int(np.ceil(2.5 * sigma)))
        assert np.array_equal(t, t[::-1]) and (np.diff(t[:R + 1]) > 0).all()
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= (2 * R + 1) * 2.0 ** -23  # one fp32 ulp per tap
    assert radii == [2, 2, 3, 4, 5, 8]


def test_frame_hold_never_drops_frame_zero():
    for sev in range(1, 6):
        for seed in range(8):
            src = robustness.describe("frame_hold", sev, (4, 1, 16, 8, 8), seed).src_t
            assert src.dtype == np.int32 and src.shape == (4, 16) and (src[:, 0] == 0).all()
            t = np.arange(16)
            assert (src <= t).all() and (np.diff(src, axis=1) >= 0).all()
            kept = src == t
            for n in range(4):  # a dropped frame shows the last kept one
                assert all(src[n, i] == max(j for j in range(i + 1) if kept[n, j]) for i in range(16))
    a, b = (robustness.frame_hold_table(.5, 3, 16, s) for s in (1, 2))
    assert not np.array_equal(a, b) and np.array_equal(a, robustness.frame_hold_table(.5, 3, 16, 1))
    assert 0.3 < (robustness.frame_hold_table(.5, 64, 16, 0)[:, 1:] != np.arange(1, 16)).mean() < 0.7


# ---- the restatement: corruption -----------------------------------------------------------------------------------------------------------
def test_z_by_hand_and_its_moments():
    # Philox4x32-10, key (0x89ABCDEF, 0x01234567), counter (5, 1, 3, 0) -> c700706d 9c85723f 88e713fa 6a794632; the top 24 bits of each:
    # 13041776 + 10257778 + 8972051 + 6977862 - 33554430 = 5695037 (< 2^24: the conversion is exact), times the fp32 sqrt(3) 2^-24
    z = rc.z_of(0x0123456789ABCDEF, 3, (1 << 32) + 5)
    assert z.dtype == np.float32 and float(z) == float(np.float32(5695037) * np.float32(np.sqrt(3.0) / 2 ** 24))
    assert float(z).hex() == "0x1.2d073a0000000p-1"
    assert float(rc.ZC).hex() == "0x1.bb67ae0000000p-24"
    z = rc.z_of(7, np.arange(4)[:, None], np.arange(250000)[None, :]).ravel().astype(np.float64)
    print(f"10^6 draws: mean {z.mean():.5f} variance {z.var():.5f} max |z| {np.abs(z).max():.5f}")
    assert abs(z.mean()) <= 0.01 and abs(z.var() - 1.0) <= 0.01 and np.abs(z).max() <= 3.4642
    # the largest sum there can be
    assert float(np.float32(4 * (2 ** 24 - 1) - 33554430) * rc.ZC) <= 3.4642


def test_noise_is_shared_by_the_channels_and_follows_the_output_voxel():
    x = np.repeat(rc.echo_raw((2, 1, 3, 9, 11), 4), 3, axis=1)  # a grey clip in three channels
    for kw in (dict(sigma_add=.16), dict(sigma_mul=.6), dict(sigma_add=.08, sigma_mul=.3)):
        y = rc.corrupt_ref(x, seed=11, **kw)
        assert np.array_equal(y[:, 0], y[:, 1]) and np.array_equal(y[:, 0], y[:, 2]) and not np.array_equal(y, x)
        assert not np.array_equal(y, rc.corrupt_ref(x, seed=12, **kw))
    assert not np.array_equal(rc.z_ref(11, 2, 3, 9, 11)[0], rc.z_ref(11, 2, 3, 9, 11)[1])
    # with a frame hold the noise stays that of the OUTPUT frame: held frames differ by their noise only
    src = np.array([[0, 0, 0], [0, 1, 1]], np.int32)
    y = rc.corrupt_ref(x, src_t=src, sigma_add=.1, seed=5)
    assert not np.array_equal(y[0, :, 0], y[0, :, 1])
    assert np.array_equal(rc.corrupt_ref(x, src_t=src)[0, :, 2], x[0, :, 0])  # every stage off: the gather of frames, bitwise


def test_corrupt_restatement_by_hand():
    mean, std = np.float32(.099), np.float32(.171)
    x = ((np.array([0.0, 0.5, 1.0, 0.25], np.float32) - mean) / std).reshape(1, 1, 1, 2, 2)
    pix = x * std + mean
    y = rc.corrupt_ref(x, row_a=np.array([2.0, 0.5], np.float32))  # gain per row, then the clamp
    want = (np.fmin(np.array([[2.0], [0.5]], np.float32) * pix[0, 0, 0], np.float32(1)) - mean) / std
    assert np.array_equal(y[0, 0, 0], want) and y[0, 0, 0, 0, 1] == (np.float32(1) - mean) / std
    # a 3-tap box blur with edge replication on a 1 x 3 row, by hand
    x = ((np.array([0.0, 0.3, 0.9], np.float32) - mean) / std).reshape(1, 1, 1, 1, 3)
    p = x.reshape(3) * std + mean
    t = np.array([.25, .5, .25], np.float32)
    rows = [(np.float32(0) + t[0] * p[max(i - 1, 0)]) + t[1] * p[i] for i in range(3)]
    rows = np.array([rows[i] + t[2] * p[min(i + 1, 2)] for i in range(3)], np.float32)
    cols = ((np.float32(0) + t[0] * rows) + t[1] * rows) + t[2] * rows  # H = 1 < R: the column pass sees the same row three times
    assert np.array_equal(rc.corrupt_ref(x, taps=t).reshape(3), (np.fmin(np.fmax(cols, np.float32(0)), np.float32(1)) - mean) / std)
    # NaN gives pixel 0; bf16 rounds to nearest even once
    x = np.array([np.nan, 0.0], np.float32).reshape(1, 1, 1, 1, 2)
    assert rc.corrupt_ref(x, sigma_add=.1, seed=1)[0, 0, 0, 0, 0] == (np.float32(0) - mean) / std
    assert rc.narrow(np.array([1.00390625, 1.01171875], np.float32), np.zeros(1, np.uint16)).tolist() == [0x3F80, 0x3F82]
    xb = rc.echo_raw((1, 3, 2, 5, 7), 2, bf16=True)
    yb = rc.corrupt_ref(xb, row_a=np.full(5, .5, np.float32))
    assert yb.dtype == np.uint16 and np.array_equal(rc.corrupt_ref(xb), xb)
    assert np.array_equal(yb, rc.narrow(rc.corrupt_ref(rc.widen(xb), row_a=np.full(5, .5, np.float32)), xb))


# ---- the restatement: statistics -----------------------------------------------------------------------------------------------------------
def test_pair_statistics_on_hand_made_maps():
    grid = (2, 3, 4)
    a = (np.arange(24, dtype=np.float32) / 24.0)
    assert rc.pair_ref(a, a, 5, grid) == (1.0, 1.0, 0.0)  # identical maps
    corr, iou, shift = rc.pair_ref(a, a[::-1].copy(), 5, grid)  # disjoint top sets, opposite corners
    assert abs(corr + 1.0) < 1e-12 and iou == 0.0 and shift == 1.0
    const, other = np.full(24, .5, np.float32), np.full(24, .25, np.float32)
    assert rc.pair_ref(const, other, 5, grid)[:2] == (1.0, 1.0)  # both constant: corr 1; the top sets are the first m indices
    assert rc.pair_ref(const, a, 5, grid)[0] == 0.0 and rc.pair_ref(a, const, 5, grid)[0] == 0.0  # exactly one constant
    assert rc.pair_ref(const, a, 5, grid)[2] == 1.0  # argmax of a constant map: index 0 = (0,0,0); of a: (1,2,3)
    # ties: the argmax is the lowest index, the top set fills up in index order
    t = np.array([0, 1, 1, 0, 1, 0] + [0] * 18, np.float32)
    assert rc.top_set(t, 2) == {1, 2} and rc.top_set(t, 4) == {0, 1, 2, 4}
    u = np.array([0, 0, 1, 0, 1, 1] + [0] * 18, np.float32)
    corr, iou, shift = rc.pair_ref(t, u, 2, grid)  # top sets {1, 2} and {2, 4}; argmax 1 = (0,0,1) and 2 = (0,0,2)
    assert iou == 1 / 3 and shift == 1.0 / np.sqrt(1 + 4 + 9)
    assert rc.pair_ref(np.ones(1, np.float32), np.zeros(1, np.float32), 1, (1, 1, 1)) == (1.0, 1.0, 0.0)  # S = 1
    with pytest.raises(AssertionError):  # a nearly constant map is refused: the correlation would be ill-conditioned
        rc.pair_ref(a, const + np.float32(1e-3) * a, 5, grid)


def test_clip_statistics_and_selection_rules():
    assert rc.pred_ref(np.array([1.0, 3.0, 3.0, 9.0], np.float32), 3) == 1  # the lowest index on ties, the abstain logit is not looked at
    assert rc.pred_ref(np.array([1.0, np.nan, 3.0], np.float32), 3) == 1    # NaN counts as the largest value
    sim = np.array([9, 9, 9, .5, .75, .75, .25, 9, 9], np.float32)
    assert rc.select_ref(sim, 3, 4, 3) == [5, 4, 3]  # descending; equal similarities: the HIGHER index first
    la = np.array([[0.0, 2.0, 0.0, 5.0]], np.float32)
    lb = np.array([[2.0, 0.0, 0.0, 5.0]], np.float32)
    sa = np.array([[0, 0, .1, .9, 0, 0, 0, 0]], np.float32)
    sb = np.array([[0, 0, .8, .2, 0, 0, 0, 0]], np.float32)
    occ = np.linspace(0, 1, 8 * 4, dtype=np.float32).reshape(1, 8, 4)
    r = rc.stats_ref(la, lb, sa, sb, occ, occ, np.array([1]), 3, 1, 1, (1, 2, 2))
    e = np.exp(2.0)
    assert r["clip"][0, 0] == 1.0 and r["correct"].tolist() == [[1, 0]] and r["sel"].tolist() == [[3]]
    assert np.allclose(r["clip"][0, 1:3], [(e - 1) / (e + 2), (e - 1) / (e + 2)], rtol=1e-15)
    assert r["clip"][0, 3] == 0.0  # clean top-1 of class 1 is prototype 3, corrupted top-1 of THE SAME block is prototype 2
    assert r["pair"][0, 0].tolist() == [float(np.float64(np.float32(.2)) - np.float64(np.float32(.9))), 1.0, 1.0, 0.0]
    acc = rc.acc_ref(np.zeros(robustness.accumulator_size(1)), r, 1)
    assert acc[0] == 1.0 and acc[4:6].tolist() == [1.0, 0.0] and acc[-1] == 1.0 and acc[7] == 1.0
    c = rc.stats_case(5, 4, 3, (1, 7, 7), seed=1)
    res = rc.stats_ref(*c[:6], c[6], 3, 3, 5, (1, 7, 7))
    assert res["pair"][1, :, 1].tolist() == [0.0] * 3 and res["pair"][2, :, 1:].tolist() == [[1.0, 1.0, 0.0]] * 3  # the planted constants
    assert res["pair"][3, :, 1:].tolist() == [[1.0, 1.0, 0.0]] * 3 and 0 < res["clip"][:, 0].sum() < 5  # identical maps; some flips


def test_the_two_restatements_select_the_same_prototypes():
    """The CPU half of test_gpu_robustness.py::test_stability_and_explain_rank_select_the_same_prototypes: on its six clips the expected
    class and prototypes do not depend on which restatement is asked (robustness_cases against explain_cases), and match the hand values."""
    from explain_cases import rank_ref

    logits, sim, _, fc_w, pred_hand, sel_hand = rc.agreement_case()
    K_real, G, k = rc.AGREE_K_REAL, rc.AGREE_G, rc.AGREE_SELECT
    assert logits.shape == (6, rc.AGREE_K) and sim.shape == (6, rc.AGREE_K * G) and not np.isnan(sim).any()
    pred = [rc.pred_ref(logits[n], K_real) for n in range(6)]
    sel = [rc.select_ref(sim[n], pred[n] * G, G, k) for n in range(6)]
    _, _, _, _, pred_e, sel_e = rank_ref(sim, fc_w, logits, K_real, k)
    assert pred == pred_e.tolist() == pred_hand.tolist()
    assert sel == sel_e.tolist() and sel[:3] == sel_hand.tolist()
    assert all(s[0] // G == p for s, p in zip(sel, pred))


def test_trainer_refuses_ppnet_and_the_cpu():
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG

    loaders = {"train": [], "val": []}
    t = DPTrainer(model_builder.build(CFG_PPNET), {"abstain_class": False, "train": TRAIN_CFG}, loaders, log=lambda *_: None)
    with pytest.raises(NotImplementedError, match="robustness evaluation covers XProtoNet and Video_XProtoNet"):
        t.evaluate_robustness("val")
    t = DPTrainer(model_builder.build(CFG_XPROTO), {"abstain_class": True, "train": TRAIN_CFG}, loaders, log=lambda *_: None)
    with pytest.raises(RuntimeError, match="GPU only"):
        t.evaluate_robustness("val")
