"""GPU: the steady-state tile pipeline of ``pwconv_persist_kernel``'s gated instances (bf16).

The kernel is persistent: a wave walks 32-row tiles at the stride of the whole grid, with the next tile's rows, the shortcut's rows and
the residual pieces in flight behind the current tile's transform, MFMAs and epilogue, and the clip index / shortcut position advanced
by the tile stride.  The small parity cases (tests/conv_kernel_cases.py, test_conv_with_fused_strided_shortcut) give every wave ONE tile
on a 256-CU device, so none of that runs.  Here M is sized from the device: with at most 4 resident blocks of 4 waves per CU a grid has
at most 16 CUs waves, and M > 3 * 32 * 16 * CUs rows gives every wave at least 3 tiles; M is odd (ragged last tile), the clip length S
is odd (tiles straddle the 3 clips' boundaries while the clip tracking advances by the tile stride), the shortcut reads odd input planes.

Per case (one full launch, one launch over clip 0 alone and one CPU reference, computed once and shared by the three tests):
  (a) the full launch against torch on the bf16-rounded operands, at the tolerances of test_conv_with_fused_strided_shortcut
      (3e-2 * max(1, |ref|max) absolute, 2e-2 relative);
  (b) the op is row-independent, so the rows of clip 0 from the launch over clip 0 alone (about one tile per wave: no steady state) must
      equal the same rows of the full launch BIT FOR BIT;
  (c) padded output channels stay zero.
Every test asserts the instance its launches ran (``plan.meta``)."""
import functools

import pytest
import torch
import torch.nn as nn

from conftest import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = torch.bfloat16
HO, WO = 55, 57  # odd plane; the shortcut's input plane is (2 HO - 1) x (2 WO - 1), odd too

# name -> (inner, cout, shortcut input channels or None (= residual), instance)
CASES = {
    "gate_res_54_24": (54, 24, None, "pwconv_persist_kernel<bf16,4,1,true>"),
    "gate_res_108_48": (108, 48, None, "pwconv_persist_kernel<bf16,8,2,true>"),
    "gate_res_54_20_tail": (54, 20, None, "pwconv_persist_kernel<bf16,4,1,true>"),          # Cout 20 != Cout_p 24
    "gate_res_108_45_tail": (108, 45, None, "pwconv_persist_kernel<bf16,8,2,true>"),        # Cout 45 != Cout_p 48
    "gate_short_54_24_24": (54, 24, 24, "pwconv_persist_kernel<bf16,4,1,false,2>"),
    "gate_short_108_48_24": (108, 48, 24, "pwconv_persist_kernel<bf16,8,2,false,2>"),
    "gate_short_108_48_48": (108, 48, 48, "pwconv_persist_kernel<bf16,8,2,false,4>"),
    "gate_short_108_45_24_tail": (108, 45, 24, "pwconv_persist_kernel<bf16,8,2,false,2>"),  # Cout 45 != Cout_p 48
}


def _rt(x):
    return x.to(DT).float()


def _frames() -> int:
    """Smallest odd T with 3 * T * HO * WO > 3 * 32 * 4 waves * 4 blocks * CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = (3 * 32 * 4 * 4 * cus) // (3 * HO * WO) + 1
    return t + 1 - t % 2


def _norm(c):
    bn = nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
    return bn.eval()


def _fold(bn):
    s = bn.weight.detach() * (bn.running_var + bn.eps).rsqrt()
    return s, bn.bias.detach() - bn.running_mean * s


def _store(rows, shape, cp):
    """fp32 rows [n * T * H * W][C] -> channels-last storage [n][T][H][W][cp] in bf16 on the device, zero padded."""
    out = torch.zeros(shape + (cp,), dtype=DT, device=DEV)
    out.view(-1, cp)[:, : rows.shape[1]] = rows.to(DEV).to(DT)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    from protoasnet_amd.plan import Act, PlanBuilder, round_up

    inner, cout, cin2, want = CASES[name]
    torch.manual_seed(sum(map(ord, name)))
    n, t = 3, _frames()
    s = t * HO * WO
    m = n * s
    assert s % 32 and m % 32 and m > 3 * 32 * 16 * torch.cuda.get_device_properties(0).multi_processor_count
    hi, wi = 2 * HO - 1, 2 * WO - 1
    z = torch.randn(m, inner)
    g = torch.rand(n, inner) + 0.25
    conv, bn = nn.Conv3d(inner, cout, 1, bias=False), _norm(cout)
    # ---- reference: torch on the bf16-rounded operands, row by row (channels-last rows are the op's natural layout)
    zin = _rt(z) * g.repeat_interleave(s, 0)
    zin = _rt(zin * torch.sigmoid(zin))
    sc, bs = _fold(bn)
    ref = zin @ _rt(conv.weight.detach().view(cout, inner)).t() * sc + bs
    del zin
    if cin2 is None:
        side = torch.randn(m, cout)
        ref += _rt(side)
        conv2 = bn2 = None
    else:
        side = torch.randn(n * t * hi * wi, cin2)
        conv2, bn2 = nn.Conv3d(cin2, cout, 1, (1, 2, 2), bias=False), _norm(cout)
        sc2, bs2 = _fold(bn2)
        picked = _rt(side).view(n, t, hi, wi, cin2)[:, :, ::2, ::2].reshape(m, cin2)
        ref += picked @ _rt(conv2.weight.detach().view(cout, cin2)).t() * sc2 + bs2
        del picked
    ref = torch.relu_(ref)

    zs = _store(z, (n, t, HO, WO), round_up(inner, 8))
    ss = _store(side, (n, t, HO, WO) if cin2 is None else (n, t, hi, wi), round_up(cout if cin2 is None else cin2, 8))
    gt = torch.zeros(n, round_up(inner, 8), dtype=torch.float32, device=DEV)
    gt[:, :inner] = g.to(DEV)
    del z, side
    conv, bn = conv.to(DEV), bn.to(DEV)
    if cin2 is not None:
        conv2, bn2 = conv2.to(DEV), bn2.to(DEV)

    def run(clips):
        pb = PlanBuilder(torch.device(DEV), DT, DT)
        za = Act(clips, t, HO, WO, inner, zs.shape[-1], pb._new_buf(zs[:clips].numel() * 2, external=True))
        gbuf = pb._new_buf(gt[:clips].numel() * 4, external=True)
        if cin2 is None:
            sa = Act(clips, t, HO, WO, cout, ss.shape[-1], pb._new_buf(ss[:clips].numel() * 2, external=True))
            y = pb.conv(za, conv, bn, "relu", residual=sa, in_gate=gbuf, in_swish=True)
        else:
            sa = Act(clips, t, hi, wi, cin2, ss.shape[-1], pb._new_buf(ss[:clips].numel() * 2, external=True))
            y = pb.conv_short(za, conv, bn, "relu", sa, conv2, bn2, in_gate=gbuf, in_swish=True)
            assert y is not None, "the fused kernel must cover this pair"
        kernel = pb.meta[-1]["kernel"]
        plan = pb.finish(za, y)
        assert len(plan.ops) == 1
        plan.ptrs[sa.buf] = ss.data_ptr()
        plan.ptrs[gbuf] = gt.data_ptr()
        out = plan.run(zs[:clips])
        torch.cuda.synchronize()
        return out, kernel

    full, k_full = run(n)
    clip0, k_clip0 = run(1)
    return {"want": want, "kernels": (k_full, k_clip0), "cout": cout, "ref": ref, "full": full.cpu(), "clip0": clip0.cpu()}


@pytest.mark.parametrize("name", list(CASES))
def test_persist_steady_state_against_torch(name):
    c = _case(name)
    assert c["kernels"] == (c["want"], c["want"]), c["kernels"]
    out = c["full"].view(-1, c["full"].shape[-1])[:, : c["cout"]].float()
    scale = max(1.0, float(c["ref"].abs().max()))
    assert_close(out, c["ref"], 3e-2 * scale, 2e-2, f"{name}: >= 3 tiles per wave, ragged last tile, 3 odd clips")


@pytest.mark.parametrize("name", list(CASES))
def test_persist_rows_do_not_depend_on_the_walk(name):
    c = _case(name)
    assert c["kernels"] == (c["want"], c["want"]), c["kernels"]
    assert torch.equal(c["full"][:1], c["clip0"]), f"{name}: clip 0 of the full launch differs from the launch over clip 0 alone"


@pytest.mark.parametrize("name", list(CASES))
def test_persist_padded_channels_stay_zero(name):
    c = _case(name)
    assert c["kernels"] == (c["want"], c["want"]), c["kernels"]
    for out in (c["full"], c["clip0"]):
        if out.shape[-1] > c["cout"]:
            assert float(out[..., c["cout"]:].float().abs().max()) == 0.0, f"{name}: padded channels must stay zero"
    if name.endswith("_tail"):
        assert c["full"].shape[-1] > c["cout"]
