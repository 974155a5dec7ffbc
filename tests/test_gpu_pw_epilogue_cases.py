"""GPU: the epilogues of ``pwconv_ws_kernel`` (pwconv_ws.hip) and ``pwconv_xtile_kernel`` (pwconv_xtile.hip) on the shapes where they can go
wrong.  Both dispatch the activation once per tile / block (ReLU compiled in, everything else behind the run-time switch on a second copy of
the body) and hold no branch between the groups of an epilogue: the tail mask is a select against a per-lane channel count, lanes without a
channel piece hand their piece to a pad slot of the LDS tile, and every masked store is issued with an out-of-range offset.

**Inputs.**  Two clips of (2, 5, 7) = 70 positions: 140 rows, so every 64-position tile is ragged and the last one spans both clips.  Two rows
use another size and say why.  Every row asserts the instance it runs by ``pb.meta[-1]["kernel"]``, as the dense-conv ladder does.

**Reference and bound** are those of tests/conv_kernel_cases.py, taken from it by import (``conv64``, ``LIPSCHITZ``, ``ACT``, ``tk.rnd``,
``tk.BF16_STORE``): operands rounded to bf16, fp64 arithmetic at the kernels' rounding points, and per element

    bound = 2^-8 |ref|  +  L (2 K 2^-24 A  +  |scale| conv(flip, |w|))  +  (2^-21 + |u| 2^-24) |ref|   [last term: sigmoid / swish]

as derived there (neither kernel rounds the pre-activation sum a second time: IMAGE = 0).  Nothing the kernel under test returns enters
the bound.  Two rows feed a conv an operand that an earlier launch or conv of the same plan produced; the reference then starts from
exactly that operand, read back from the device (it is a bf16 tensor: the values ARE what the conv read):

* the chained pair's second conv reads the first conv's stored output;
* the squeeze-excite row's conv reads the stencil's output and computes its gate from the stencil's pool partial rows.  The reference
  computes the gate from the same rows in fp64; the kernel's fp32 mean / fc1 / fc2 differ from it by at most
  dg = 1/4 (sum|w2| e_h + 2 (cse + 1) 2^-24 A_2) + 2^-21 g with e_h = 2 (C + blocks + 1) 2^-24 A_1 (A_i = the sum of the magnitudes of
  the terms of the dot product: every fp32 addition rounds by 2^-24 of a partial sum that A_i bounds, the factor 2 is the margin; 1/4 =
  sigmoid's Lipschitz constant; 2^-21 g = the sigmoid itself, as in the ladder).  That relative error dg / g of the gate joins the ladder's
  eps of the transformed operand with swish's condition number: eps = (8 + 2 |v|) 2^-24 + (1 + |v|) dg / g, and ``flip`` follows from eps
  as in the ladder."""
import collections
import functools

import pytest
import torch
import torch.nn as nn

import conv_kernel_cases as ck
import train_kernel_cases as tk
from conftest import assert_close

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
NTHW = (2, 2, 5, 7)  # 2 clips x 70 positions
_WS_ALL = {"PASN_WS": "2"}  # every layer the weight-stationary kernel covers, not only its measured routes

Row = collections.namedtuple("Row", "id cin cout nthw s act res env expect")


def _r(id, cin, cout, expect, act="relu", res=False, env=None, nthw=NTHW, s=(1, 1, 1)):
    return Row(id, cin, cout, nthw, s, act, res, dict(env or {}), expect)


ROWS = [
    # 216 -> 96 + residual rides the chained pair in the default plans: the single launch needs the switch
    _r("ws_216_96_res", 216, 96, "pwconv_ws_kernel<14,1,false,true>", res=True, env=_WS_ALL),
    _r("ws_96_432", 96, 432, "pwconv_ws_kernel<6,2,false,false>"),
    # Cout = 54 in Cout_p = 56: the tail mask zeroes two channels.  With two channel tiles the geometry picks four position waves (128-row tiles),
    # which a clip of 70 positions does not hold: one position wave (PASN_WS_PT=1) keeps the common input, on 64-row tiles
    _r("ws_48_54_tail", 48, 54, "pwconv_ws_kernel<4,2,false,false>", env={"PASN_WS": "2", "PASN_WS_PT": "1"}),
    _r("xtile_48_108_tail", 48, 108, "pwconv_xtile_kernel<bf16,4,false>"),
    # strided gather: OUTPUT planes (2, 6, 10) from input (2, 11, 19).  (As input planes, (2, 6, 10) leave 30 output positions per clip, and the
    # kernel demands a clip of at least one 64-row tile.)  120 positions per clip: 240 rows, ragged, the second tile spans both clips
    _r("xtile_48_96_stride", 48, 96, "pwconv_xtile_kernel<bf16,4,false>", nthw=(2, 2, 11, 19), s=(1, 2, 2)),
    # the run-time arm (second copy of the tile body) through the same entry point
    _r("ws_96_432_none", 96, 432, "pwconv_ws_kernel<6,2,false,false>", act="none"),
    _r("ws_96_432_swish", 96, 432, "pwconv_ws_kernel<6,2,false,false>", act="swish"),
    _r("ws_48_54_tail_swish", 48, 54, "pwconv_ws_kernel<4,2,false,false>", act="swish", env={"PASN_WS": "2", "PASN_WS_PT": "1"}),  # swish(0) = 0 but sigmoid-free paths must not leak: masked after the activation
    _r("xtile_48_108_tail_none", 48, 108, "pwconv_xtile_kernel<bf16,4,false>", act="none"),
    _r("xtile_48_108_tail_swish", 48, 108, "pwconv_xtile_kernel<bf16,4,false>", act="swish"),
]
BY_ID = {r.id: r for r in ROWS}


def _bn(c, g):
    bn = nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5), bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3), bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn.eval()


def _conv(cin, cout, g, s=(1, 1, 1)):
    conv = nn.Conv3d(cin, cout, 1, s, 0, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 1, 1, 1, generator=g) * (1.5 / cin ** 0.5))
    return conv


def _folded(bn, cout):
    from protoasnet_amd.plan import fold_norm

    scale, bias = fold_norm(bn, None, cout, cout, torch.device("cpu"))
    return scale.to(F64).view(1, -1, 1, 1, 1), bias.to(F64).view(1, -1, 1, 1, 1)


def ref_bound(xt, flip, conv, bn, res, act):
    """ref, bound (N,Cout,To,Ho,Wo) in fp64 of act(norm(conv(xt)) + res): the ladder's formula (module docstring).  ``xt``: the operand the
    matrix cores read, fp64 values of bf16 numbers; ``flip``: how far a correct kernel's copy of it may lie, or None."""
    w = tk.rnd(conv.weight.detach(), BF16)
    s, p = tuple(conv.stride), (0, 0, 0)
    sc, bi = _folded(bn, conv.out_channels)
    u = sc * ck.conv64(xt, w, s, p) + bi
    A = sc.abs() * ck.conv64(xt.abs(), w.abs(), s, p) + bi.abs()
    if res is not None:
        u, A = u + res, A + res.abs()
    ref = ck.ACT[act](u)
    pre = 2 * ck.round_up(conv.in_channels, 8) * 2.0 ** -24 * A
    if flip is not None:
        pre = pre + sc.abs() * ck.conv64(flip, w.abs(), s, p)
    bound = tk.BF16_STORE * ref.abs() + ck.LIPSCHITZ[act] * pre
    if act in ("sigmoid", "swish"):
        bound = bound + (2.0 ** -21 + u.abs() * 2.0 ** -24) * ref.abs()
    return ref, bound


def check(label, out, cout, ref, bound):
    """``out`` [N][To][Ho][Wo][Cout_p] as launched into a tensor full of NaN: every element written, |out - ref| <= bound on the real channels
    (logged as err / bound against 1), exact zeros in the padded ones."""
    out = out.detach().cpu().to(F64)
    assert tuple(out.shape[:-1]) == (ref.shape[0],) + tuple(ref.shape[2:]) and out.shape[-1] == ck.round_up(cout, 8), tuple(out.shape)
    assert bool(torch.isfinite(out).all()), f"{label}: {int((~torch.isfinite(out)).sum())} elements unwritten or not finite"
    err = (out[..., :cout].permute(0, 4, 1, 2, 3) - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    print(f"{label}: max err / bound = {float(ratio.max()):.3f}, max err = {float(err.max()):.3g}, max |ref| = {float(ref.abs().max()):.3g}")
    assert_close(ratio, torch.zeros_like(ratio), 1.0, 0.0, f"{label} (err / bound)")
    if out.shape[-1] > cout:
        assert float(out[..., cout:].abs().max()) == 0.0, f"{label}: padded channels must be exact zeros"


# ------------------------------------------------------------------------------------------------- single launches
@functools.lru_cache(maxsize=None)
def single(row_id):
    """Modules, inputs and the reference of a row, drawn and computed once (the ReLU and the run-time rows of a shape share the seed)."""
    row = BY_ID[row_id]
    g = torch.Generator().manual_seed(7000 + row.cin * 7 + row.cout)
    n, t, h, w = row.nthw
    x = torch.randn(n, row.cin, t, h, w, generator=g)
    conv, bn = _conv(row.cin, row.cout, g, row.s), _bn(row.cout, g)
    out_thw = tuple((i - 1) // ss + 1 for i, ss in zip((t, h, w), row.s))
    res = torch.randn(n, row.cout, *out_thw, generator=g) if row.res else None
    ref, bound = ref_bound(tk.rnd(x, BF16), None, conv, bn, tk.rnd(res, BF16) if row.res else None, row.act)
    return dict(x=x, conv=conv, bn=bn, res=res, ref=ref, bound=bound, out_thw=out_thw)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_pointwise_epilogue_row(row):
    from protoasnet_amd.plan import Act, PlanBuilder

    T = single(row.id)
    n, t, h, w = row.nthw
    with ck.switches(row):
        pb = PlanBuilder(torch.device("cuda"), BF16, BF16)
        store = ck._channels_last(T["x"], ck.round_up(row.cin, 8), BF16, "cuda")
        x = Act(n, t, h, w, row.cin, store.shape[-1], pb._new_buf(store.numel() * 2, external=True))
        binds, ra = [], None
        if row.res:
            rs = ck._channels_last(T["res"], ck.round_up(row.cout, 8), BF16, "cuda")
            ra = Act(n, *T["out_thw"], row.cout, rs.shape[-1], pb._new_buf(rs.numel() * 2, external=True))
            binds.append((ra.buf, rs))
        y = pb.conv(x, T["conv"].to("cuda"), T["bn"].to("cuda"), row.act, residual=ra)
        name = pb.meta[-1]["kernel"]
        assert name == row.expect, f"{row.id}: the launch runs {name}, the row says {row.expect}"
        out = ck.launch(ck.Built(pb, x, y, name, store, binds))
    check(f"{name} {row.id}", out, row.cout, T["ref"], T["bound"])


# ------------------------------------------------------------------------------------------------- the chained pair
def _nan_out(pb, plan, act):
    """An output tensor full of NaN behind a plan buffer (made external before ``finish``)."""
    y = torch.full((act.N, act.T, act.H, act.W, act.Cp), float("nan"), dtype=BF16, device="cuda")
    plan.ptrs[act.buf] = y.data_ptr()
    return y


def _run(plan, store, binds):
    from protoasnet_amd import _lib

    for buf, t in binds:
        plan.ptrs[buf] = t.data_ptr()
    plan.ptrs[plan.in_buf] = store.data_ptr()
    for op in plan.ops:
        op(plan.ptrs, _lib.current_stream())
    torch.cuda.synchronize()


def _from_cl(y, c):
    return y.detach().cpu().to(F64)[..., :c].permute(0, 4, 1, 2, 3)


def test_chained_pair_216_96_216():
    """``pwconv_ws_kernel<14,1,false,true,6>``: project conv + residual + ReLU, its tile handed over in LDS to the expand conv + ReLU.  140
    rows in 64-row tiles: the tiles hold rows beyond M, whose pieces go through the hand-over all the same and are never stored."""
    from protoasnet_amd.plan import Act, PlanBuilder

    c0, c1, c2 = 216, 96, 216
    n, t, h, w = NTHW
    g = torch.Generator().manual_seed(7216)
    x, res = torch.randn(n, c0, t, h, w, generator=g), torch.randn(n, c1, t, h, w, generator=g)
    conv1, bn1, conv2, bn2 = _conv(c0, c1, g), _bn(c1, g), _conv(c1, c2, g), _bn(c2, g)
    with ck.switches(_r("pair", c0, c1, "")):
        pb = PlanBuilder(torch.device("cuda"), BF16, BF16)
        store, rs = ck._channels_last(x, c0, BF16, "cuda"), ck._channels_last(res, c1, BF16, "cuda")
        xa = Act(n, t, h, w, c0, c0, pb._new_buf(store.numel() * 2, external=True))
        ra = Act(n, t, h, w, c1, c1, pb._new_buf(rs.numel() * 2, external=True))
        pair = pb.conv_pair(xa, conv1.to("cuda"), bn1.to("cuda"), "relu", ra, conv2.to("cuda"), bn2.to("cuda"), "relu")
        assert pair is not None and pb.meta[-1]["kernel"] == "pwconv_ws_kernel<14,1,false,true,6>", pb.meta[-1]["kernel"]
        o1, o2 = pair
        pb.bufs[o1.buf].external = True
        plan = pb.finish(xa, o2)
        y1, y2 = _nan_out(pb, plan, o1), _nan_out(pb, plan, o2)
        plan.ptrs[plan.out_buf] = y2.data_ptr()
        _run(plan, store, [(ra.buf, rs)])
    ref1, bound1 = ref_bound(tk.rnd(x, BF16), None, conv1.cpu(), bn1.cpu(), tk.rnd(res, BF16), "relu")
    check("pair: block output", y1, c1, ref1, bound1)
    ref2, bound2 = ref_bound(_from_cl(y1, c1), None, conv2.cpu(), bn2.cpu(), None, "relu")  # from the block output the launch stored
    check("pair: expand output", y2, c2, ref2, bound2)


# ------------------------------------------------------------------------------------------------- gated, squeeze-excite prologue
def test_gated_project_conv_432_192_se_prologue():
    """``pwconv_ws_kernel<28,1,true,true>`` with the gate computed in its prologue: depthwise stencil (+ pool partial rows) -> project conv on
    x' = swish(x * gate) + residual + ReLU.  The gated instances share the epilogue of the plain ones."""
    from protoasnet_amd.plan import Act, PlanBuilder, se_operands

    c, cout, cse = 432, 192, 32
    n, t, h, w = NTHW
    g = torch.Generator().manual_seed(7432)
    x, res = torch.randn(n, c, t, h, w, generator=g), torch.randn(n, cout, t, h, w, generator=g)
    conv_b = nn.Conv3d(c, c, 3, 1, 1, groups=c, bias=False)
    fc1, fc2 = nn.Conv3d(c, cse, 1), nn.Conv3d(cse, c, 1)
    with torch.no_grad():
        conv_b.weight.copy_(torch.randn(c, 1, 3, 3, 3, generator=g) * 0.25)
        fc1.weight.copy_(torch.randn(cse, c, 1, 1, 1, generator=g) * (1.5 / c ** 0.5)), fc1.bias.copy_(torch.randn(cse, generator=g) * 0.3)
        fc2.weight.copy_(torch.randn(c, cse, 1, 1, 1, generator=g) * (1.5 / cse ** 0.5)), fc2.bias.copy_(torch.randn(c, generator=g) * 0.3)
    bn_b, conv_c, bn_c = _bn(c, g), _conv(c, cout, g), _bn(cout, g)
    with ck.switches(_r("se", c, cout, "", env=_WS_ALL)):
        pb = PlanBuilder(torch.device("cuda"), BF16, BF16)
        store, rs = ck._channels_last(x, c, BF16, "cuda"), ck._channels_last(res, cout, BF16, "cuda")
        xa = Act(n, t, h, w, c, c, pb._new_buf(store.numel() * 2, external=True))
        ra = Act(n, t, h, w, cout, cout, pb._new_buf(rs.numel() * 2, external=True))
        yb, pooled = pb.dwconv(xa, conv_b.to("cuda"), bn_b.to("cuda"), act="none", pool=True)
        out = pb.conv_se(yb, conv_c.to("cuda"), bn_c.to("cuda"), "relu", ra, pooled, fc1.to("cuda"), fc2.to("cuda"))
        assert out is not None and pb.meta[-1]["kernel"] == "pwconv_ws_kernel<28,1,true,true>[se]", pb.meta[-1]
        pool_buf, blocks, _ = pooled
        pb.bufs[yb.buf].external = pb.bufs[pool_buf].external = True
        plan = pb.finish(xa, out)
        ys, y = _nan_out(pb, plan, yb), _nan_out(pb, plan, out)
        pool = torch.zeros(n, blocks, yb.Cp, dtype=torch.float32, device="cuda")
        plan.ptrs[plan.out_buf] = y.data_ptr()
        _run(plan, store, [(ra.buf, rs), (pool_buf, pool)])
    # the gate, in fp64 from the partial rows the prologue read, and how far its fp32 evaluation may lie from that
    w1, b1, w2, b2 = (v.cpu().to(F64) for v in se_operands(fc1, fc2))
    part = pool.cpu().to(F64)[..., :c]                                  # [n][blocks][c]
    mean = part.sum(1) / (t * h * w)
    a1 = part.abs().sum(1) / (t * h * w) @ w1.abs().t() + b1.abs()      # [n][cse]
    hid = torch.relu(mean @ w1.t() + b1)
    e_h = 2 * (c + blocks + 1) * 2.0 ** -24 * a1
    z = hid @ w2.t() + b2
    a2 = hid @ w2.abs().t() + b2.abs()
    gate = torch.sigmoid(z)                                             # [n][c]
    dg = 0.25 * (e_h @ w2.abs().t() + 2 * (cse + 1) * 2.0 ** -24 * a2) + 2.0 ** -21 * gate
    xs = _from_cl(ys, c)                                                # the stencil's output as stored: what the conv read
    assert bool(torch.isfinite(xs).all())
    v = xs * gate[:, :, None, None, None]
    xt = v * torch.sigmoid(v)
    eps = (8 + 2 * v.abs()) * 2.0 ** -24 + (1 + v.abs()) * (dg / gate)[:, :, None, None, None]
    flip = (tk.rnd(xt * (1 + eps), BF16) - tk.rnd(xt * (1 - eps), BF16)).abs()
    ref, bound = ref_bound(tk.rnd(xt, BF16), flip, conv_c.cpu(), bn_c.cpu(), tk.rnd(res, BF16), "relu")
    check("gated project conv, gate in the prologue", y, cout, ref, bound)
