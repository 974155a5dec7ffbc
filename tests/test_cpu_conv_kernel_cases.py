"""CPU: the table of tests/conv_kernel_cases.py, checked without a GPU -- (a) every row reaches exactly the kernel instance it names,
(b) the table claims every instance ``PlanBuilder.conv`` emits in the default plans of the four trunks and in the prototype heads' plans
(the ledger), (c) the fp64 reference agrees with torch's conv3d + eval-mode BatchNorm3d, (d) the bound holds for an fp32-accumulating
emulation of the kernels on every row and FAILS on six ways a kernel goes subtly wrong."""
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_kernel_cases as ck
import train_kernel_cases as tk
import util
from conftest import GOLDEN

F64 = torch.float64
IDS = [c.id for c in ck.CASES]


# ------------------------------------------------------------------------------------------------- (a) instance names
@pytest.mark.parametrize("case", ck.CASES, ids=IDS)
def test_every_row_reaches_the_instance_it_names(case):
    with ck.switches(case):
        name = ck.build(case, "cpu").name
    assert name == case.expect, f"{case.id}: the row runs {name}, its label says {case.expect}"


def test_rows_cover_what_the_table_promises():
    """Per family: a residual row, a sigmoid row with padded output channels, a partial last 8-channel chunk; a gated row where the kernel
    takes a gate; clips no multiple of (and, but for the kernels that demand a whole tile per clip, shorter than) the 32-row tile."""
    fam = {}
    for c in ck.CASES:
        fam.setdefault(c.expect.split("<")[0].replace("igemm_halo", "igemm").replace("igemm_glds", "igemm"), []).append(c)
    assert set(fam) == {"tconv_ws_kernel", "pwconv_ws_kernel", "pwconv_tiny_kernel", "pwconv_persist_kernel", "pwconv_xtile_kernel", "igemm_kernel",
                        "gemm_conv_kernel", "conv3d_mfma_kernel"}
    for name, rows in fam.items():
        assert any(c.res for c in rows), f"{name}: no residual row"
        assert any(c.act == "sigmoid" and c.cout % 8 for c in rows), f"{name}: no sigmoid row with padded output channels"
        assert any(c.cin % 8 for c in rows) and any(c.cin % 16 for c in rows), f"{name}: no partial last 8- / 16-channel chunk"
        if name not in ("tconv_ws_kernel", "pwconv_tiny_kernel", "igemm_kernel"):  # these take no gate
            assert any(c.gate for c in rows), f"{name}: no gated row"
        for c in rows:
            n, (to, ho, wo) = c.nthw[0], ck.out_extent(c)
            assert n >= 2 and (n * to * ho * wo) % 32 != 0, f"{c.id}: rows are a multiple of the tile"
            if c.gate:
                assert (to * ho * wo) % 32 != 0, f"{c.id}: no tile straddles two clips"


# ------------------------------------------------------------------------------------------------- (b) the ledger
@functools.lru_cache(maxsize=None)
def default_plan_meta():
    """[(routing case, ``meta`` row)] of every launch of the eight un-switched routing cases (the four trunks, both compute types), built on
    the CPU with every ``PASN_*`` switch of the environment cleared.  The plan walk the ledgers share (tests/test_cpu_dw_kernel_cases.py)."""
    sys.path.insert(0, GOLDEN)
    import make_routing_snapshot as mrs

    from protoasnet_amd import _lib, backbones
    from protoasnet_amd.plan import PlanBuilder

    dt = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}
    trunks = {"x3d_s": lambda: backbones.X3DFeatures("x3d_s"), "x3d_m": lambda: backbones.X3DFeatures("x3d_m"),
              "resnet2p1d_18": lambda: backbones.resnet2p1d_18(pretrained=False), "resnet18": backbones.ResNet18Features}
    default = [c for c in mrs.CASES if not c[5]]
    assert len(default) == 8
    rows = []
    with _lib.tuning_env(**{k: None for k in os.environ if k.startswith("PASN_")}):
        for name, arch, shape, dtype, in_dtype, _ in default:
            trunk = trunks[arch]()
            pb = PlanBuilder(torch.device("cpu"), dt[dtype], dt[in_dtype], trunk.input_affine)
            with torch.no_grad():
                trunk.build_plan(pb, pb.input(shape))
            rows += [(name, m) for m in pb.meta]
    return tuple(rows)


def _default_plan_names():
    """{instance name: first plan that launches it} over the un-switched routing cases (the four trunks, both compute types) and the
    add-on / occurrence chains of the prototype heads, which run through ``PlanBuilder.conv`` launch by launch."""
    from protoasnet_amd import model_builder
    from protoasnet_amd.plan import Act, PlanBuilder

    seen = {}
    for name, m in default_plan_meta():
        if m["kind"] == "conv":
            seen.setdefault(m["kernel"], f"{name}: {m['shape']}")
    # head A (ProtoPNet add-on layers, both forms) and head B (add-on + occurrence module) behind the trunks' feature maps
    heads = (("ppnet", util.CFG_PPNET, (8, 1, 7, 7)), ("ppnet_bottleneck", util.CFG_PPNET_BOTTLENECK, (8, 1, 7, 7)), ("xprotonet", util.CFG_XPROTO, (8, 1, 7, 7)),
             ("video_x3d", util.CFG_VIDEO_X3D, (32, 16, 7, 7)), ("video_r2plus1d", util.CFG_VIDEO_R2P1D, (2, 8, 14, 14)))
    for tag, cfg, (n, t, h, w) in heads:
        model = model_builder.build(cfg)
        chains = [model.add_on_layers] + ([model.occurrence_module] if hasattr(model, "occurrence_module") else [])
        for dtype in (torch.float32, torch.bfloat16):
            for chain in chains:
                pb = PlanBuilder(torch.device("cpu"), dtype, dtype)
                cin = chain.convs()[0].in_channels
                a = Act(n, t, h, w, cin, ck.round_up(cin, 8), pb._new_buf(16, external=True))
                for conv, act in chain._steps():
                    a = pb.conv(a, conv, None, act)
                for m in pb.meta:
                    seen.setdefault(m["kernel"], f"{tag} head, {dtype}: {m['shape']}")
    return seen


@pytest.fixture(scope="module")
def default_plan_names():
    from protoasnet_amd import _lib

    with _lib.tuning_env(**{k: None for k in os.environ if k.startswith("PASN_")}):
        return _default_plan_names()


def _unclaimed(seen, claimed):
    return {k: v for k, v in seen.items() if k not in claimed}


def test_ledger_every_instance_of_the_default_plans_has_a_row(default_plan_names):
    seen = default_plan_names
    assert len(seen) >= 30, "the collection itself broke"
    missing = _unclaimed(seen, {c.expect for c in ck.CASES})
    assert not missing, "instances a default plan launches and no row of tests/conv_kernel_cases.py runs:\n" + "\n".join(f"  {k}   ({v})" for k, v in missing.items())


def test_ledger_notices_a_row_that_is_gone(default_plan_names):
    """With one claimed production instance taken out of the table the ledger names it."""
    victim = "igemm_halo_kernel<5,2,0>"
    claimed = {c.expect for c in ck.CASES if c.expect != victim}
    assert list(_unclaimed(default_plan_names, claimed)) == [victim]


# ------------------------------------------------------------------------------------------------- (c) the reference
@pytest.mark.parametrize("case", ck.CASES, ids=IDS)
def test_reference_is_conv3d_and_eval_mode_batch_norm_in_fp64(case):
    """Independent restatement: F.conv3d + nn.BatchNorm3d.eval() in fp64 on the same rounded operands.  The reference reads the launch's
    fp32 fold of the norm: scale and bias are each a few 2^-24 off the fp64 fold, relative to |scale| and to |beta| + |mean scale| < 4."""
    dtype, T = ck.DT[case.dtype], ck.tensors(case.id)
    R = ck.reference(case.id)
    x = tk.rnd(T["x"], dtype)
    if case.in_swish:
        v = x * T["gate"].to(F64)[:, :, None, None, None] if case.gate else x
        x = tk.rnd(v * torch.sigmoid(v), dtype)
    bn = nn.BatchNorm3d(case.cout).double().eval()
    with torch.no_grad():
        bn.weight.copy_(T["gamma"]), bn.bias.copy_(T["beta"]), bn.running_mean.copy_(T["mean"]), bn.running_var.copy_(T["var"])
        u = bn(F.conv3d(x, tk.rnd(T["w"], dtype), None, case.s, case.p))
    if case.res:
        u = u + tk.rnd(T["res"], dtype)
    want = ck.ACT[case.act](u)
    assert want.shape == R["ref"].shape
    err = (R["ref"] - want).abs()
    assert bool((err <= 1.1 * 2.0 ** -20 * (R["A"] + 4)).all()), float(err.max())
    assert bool((R["bound"] > 0).all()) and 0.2 < float((R["u"] > 0).double().mean()) < 0.8
    if case.in_swish and dtype == torch.bfloat16:
        assert R["at_risk"] < 2e-3, "the flip term charges a few operands only"


# ------------------------------------------------------------------------------------------------- (d) the bound discriminates
def _emulate(case, gate_of_clip=None, drop_tail_chunk=False, act_first=False):
    """What a correct kernel computes, with fp32 accumulation: torch's fp32 conv on the rounded operands (the input transform taken in
    fp32 and rounded, as the kernels do), fp32 epilogue (norm(conv) rounded once more where the kernel's epilogue does, ``ck.rounds_pre_sum``), output rounded to the dtype.  Returns the launch's layout [N][To][Ho][Wo][Cout_p]."""
    dtype, T = ck.DT[case.dtype], ck.tensors(case.id)
    x = T["x"].to(dtype).float()
    if case.in_swish:
        if case.gate:
            g = T["gate"] if gate_of_clip is None else T["gate"][gate_of_clip]
            x = x * g[:, :, None, None, None]
        x = (x * torch.sigmoid(x)).to(dtype).float()
    if drop_tail_chunk:
        x = x.clone()
        x[:, case.cin // 8 * 8:] = 0.0
    scale, bias = (v.float().view(1, -1, 1, 1, 1) for v in ck.folded(case))
    u = F.conv3d(x, T["w"].to(dtype).float(), None, case.s, case.p) * scale + bias
    if ck.rounds_pre_sum(case):  # the epilogues with an LDS image in the compute dtype
        u = u.to(dtype).float()
    act = ck.ACT[case.act]
    if case.res:
        r = T["res"].to(dtype).float()
        u = act(u) + r if act_first else act(u + r)
    else:
        u = act(u)
    out = torch.zeros(u.shape[0], *u.shape[2:], ck.round_up(case.cout, 8), dtype=dtype)
    out[..., :case.cout] = u.permute(0, 2, 3, 4, 1).to(dtype)
    return out


def _rows(out):
    return out.view(-1, out.shape[-1])


def _must_fail(case, out, what):
    with pytest.raises(AssertionError):
        ck.check(case, out, what)
    return 1


@pytest.mark.parametrize("case", ck.CASES, ids=IDS)
def test_bound_holds_for_fp32_accumulation_and_fails_on_subtle_faults(case):
    good = _emulate(case)
    ratio = ck.check(case, good, "fp32 emulation")
    assert ratio <= 1.0
    to, ho, wo = ck.out_extent(case)
    s, m = to * ho * wo, case.nthw[0] * to * ho * wo
    tried = 0
    # the last partial 8-channel chunk of K dropped for one 32-row tile (the last one, ragged)
    if case.cin % 8:
        bad = good.clone()
        t0 = (m - 1) // 32 * 32
        _rows(bad)[t0:] = _rows(_emulate(case, drop_tail_chunk=True))[t0:]
        tried += _must_fail(case, bad, "partial chunk dropped")
    # the next clip's gate row for the rows of the first tile that straddles clips 0 and 1
    if case.gate:
        n = case.nthw[0]
        bad = good.clone()
        _rows(bad)[s // 32 * 32:s] = _rows(_emulate(case, gate_of_clip=(torch.arange(n) + 1) % n))[s // 32 * 32:s]
        tried += _must_fail(case, bad, "next clip's gate row")
    # the activation applied before the residual
    if case.res and case.act != "none":
        tried += _must_fail(case, _emulate(case, act_first=True), "activation before the residual")
    # one output row written at the neighbouring position
    bad = good.clone()
    _rows(bad)[m // 2 + 1] = _rows(good)[m // 2]
    tried += _must_fail(case, bad, "row at its neighbour's position")
    # sigmoid(0) = 0.5 left in a padded channel; a row the launch never wrote
    if case.cout % 8:
        bad = good.clone()
        bad[0, 0, 0, 0, -1] = 0.5 if case.act == "sigmoid" else 2.0 ** -100
        tried += _must_fail(case, bad, "padded channel not masked")
    bad = good.clone()
    _rows(bad)[m - 1] = float("nan")
    tried += _must_fail(case, bad, "last row unwritten")
    assert tried >= 2
