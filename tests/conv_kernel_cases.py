"""The dense-conv ladder (``pasn_conv3d_fwd``, ``conv_route`` in csrc/conv.hip) case by case, pure torch on the CPU: one table of layers,
each pinned to the kernel instance it runs, with inputs, an fp64 reference and a per-element error bound built from the reference alone.

Shared by tests/test_gpu_conv_cases.py, which runs the HIP kernels on these inputs, and tests/test_cpu_conv_kernel_cases.py, which checks
without a GPU that every row reaches the instance it names, that the table claims every instance the default plans launch, that the
reference is right and that the bound tells a correct kernel from a subtly wrong one.

**Reference.**  Every operand is rounded to the compute dtype first (``train_kernel_cases.rnd``): x, the weights, the residual.  The folded
norm (scale, bias) and the gate rows are fp32 tensors, which the kernels read as they are.  A transformed input x' = swish(x * gate) (or
swish(x) without a gate) is taken in fp64 and rounded once more to the compute dtype, as the kernels round it before the matrix cores.
Then, in fp64: u = scale * conv(x', w) + bias + residual, ref = act(u).  The conv is a sum over the taps of fp64 matrix products.

**Bound**, per output element, from the reference's own quantities (nothing the kernel returns enters it):

    bound = STORE * |ref|  +  L * (2 * K * 2^-24 * A  +  |scale| * conv(flip, |w|)  +  IMAGE * |pre|)  +  (2^-21 + |u| * 2^-24) * |ref|
                                                                                          [last term: sigmoid / swish]

* ``STORE``: the output's rounding, ``BF16_STORE`` = 2^-8 for bf16, 2^-23 for fp32.  2^-8 is bf16's unit roundoff (8 significand bits: half a
  spacing, relative to a value just above a power of two), so this term has NO margin: a correct kernel reaches 0.98 of the bound where
  |ref| sits just above 2 or 4 (profiles/conv_ladder_parity_observed.tsv); the fp32 rows stay below 0.08 of theirs.
* ``K = Cin_p * taps`` terms meet in one fp32 accumulator; A = |scale| * conv(|x'|, |w|) + |bias| + |residual| is the sum of their
  magnitudes.  bf16 products are exact in fp32, every addition rounds by 2^-24 of a partial sum that A bounds: K * 2^-24 * A, and the
  factor 2 is the margin (it also covers the fp32 products of the fp32 kernels and the epilogue's fused multiply-add).
* ``IMAGE * |pre|``, pre = scale * conv(x', w) + bias -- **a second store, by design, in three bf16 epilogues.**  They pass the finished tile
  through an LDS image in the compute dtype so that the residual read and the store are whole 16-byte pieces per lane: norm(conv) is
  rounded to bf16 THERE, the residual is added to the rounded sum, the activation follows and the result is rounded again.
  ``pwconv_persist_kernel<bf16,..,true>`` (pwconv.hip, "added in the copy-out loop on the rounded pre-activation sums"), the implicit-GEMM
  kernels with a residual (igemm_epilogue.h, "keep that rounding point") and ``gemm_conv_kernel<bf16,..>`` always (its block image holds T).
  The issue's formula has one store only; for these rows (``rounds_pre_sum``) IMAGE = ``BF16_STORE``, for every other row 0.  Without a
  residual under none / relu / abs the second rounding changes nothing (the image's value is already a bf16 number) and IMAGE stays 0.
* ``L``, the activation's Lipschitz constant, carries the error of u to act(u): 1 for none / relu / abs, 1/4 for sigmoid, 1.1 for swish
  (max |swish'| = 1.0998).  The issue's formula has no L; without it a swish case is bounded 10 % too tightly and a sigmoid case four
  times too loosely.
* The last term is the epilogue's sigmoid = v_rcp(1 + v_exp(-u * log2 e)): v_exp and v_rcp are within one ulp (2^-23) each, the addition
  and swish's product round by 2^-24 each: 6 * 2^-24 < 2^-21.  The product -u * log2 e is rounded before v_exp sees it, an absolute error
  of |u| log2 e 2^-24 in the exponent, i.e. a relative |u| * 2^-24 in exp(-u): hence |u| * 2^-24 on top of the constant 2^-21, which
  alone would not hold for |u| > 2.
* ``flip`` -- **the transformed operand on the other side of a rounding boundary.**  The kernel computes v = x * gate in fp32 (rounds by
  2^-24, which swish's relative condition number |1 + v (1 - sigmoid v)| <= 1 + |v| carries over) and swish(v) as above ((6 + |v|) * 2^-24):
  its x' before the rounding is x'(1 + d) with |d| <= eps(v) = (8 + 2 |v|) * 2^-24.  Rounding is monotone, so the kernel's rounded operand
  lies between rnd(x'(1 - eps)) and rnd(x'(1 + eps)).  For almost every operand these two are the same number, and the kernel's operand
  IS the reference's; where they differ, x' sits within eps of a rounding boundary and the kernel may legitimately hold the neighbour:
  flip = |rnd(x'(1 + eps)) - rnd(x'(1 - eps))|, one operand ulp for the few operands at risk and exactly zero for all the others.  The
  term charges |w| * flip for the operands at risk only, so it stays far below "one ulp on every term" (2^-7 * A): in bf16 about
  eps / 2^-8 ~ 2^-12 of the operands are at risk.  In fp32 eps is several ulps, every operand is "at risk", and the same expression is the
  plain first-order bound 2 eps |x'| |w|.

Padded output channels (``Cout .. Cout_p``) must read back as exact zeros, whatever the activation (sigmoid(0) = 0.5 must be masked), and
nothing of the output may be left unwritten: the GPU test hands the launch an output full of NaN.

**Table.**  ``expect`` is the full instance name as ``plan.conv_kernel_name`` prints it; ``env`` holds the routing switches a row needs to
reach that instance at a small shape (the row is built AND launched under them: the launch decides its route again).  Shapes are the
smallest that still go wrong: rows no multiple of the tile, clips shorter than a tile (or, where the kernel demands a clip of at least
one tile, shorter than two) so that a tile straddles two clips, channel counts with a partial last 8- / 16-channel chunk (54, 108, 45,
30, 180, 230), padded output channels also under sigmoid, a residual.  ``igemm_halo_kernel<5,2,0>`` needs 131 k rows (its MT = 2 tile is chosen only
where the grid still fills the chip twice) and ``conv3d_mfma_kernel<.,.,2>`` 262 k: three rows of that size, about two seconds each."""
import collections
import functools
import os

import torch
import torch.nn as nn

import train_kernel_cases as tk
from conftest import assert_close

F64 = torch.float64
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
LIPSCHITZ = {"none": 1.0, "relu": 1.0, "abs": 1.0, "sigmoid": 0.25, "swish": 1.1}
ACT = {"none": lambda v: v, "relu": torch.relu, "abs": torch.abs, "sigmoid": torch.sigmoid, "swish": lambda v: v * torch.sigmoid(v)}

Case = collections.namedtuple("Case", "id cin cout k s p nthw act res gate in_swish dtype env expect")

P0, S1, K1 = (0, 0, 0), (1, 1, 1), (1, 1, 1)


def _c(id, cin, cout, nthw, expect, act="relu", res=False, gate=False, in_swish=False, dtype="bf16", k=K1, s=S1, p=P0, env=None):
    return Case(id, cin, cout, k, s, p, nthw, act, res, gate, in_swish or gate, dtype, dict(env or {}), expect)


_NO_PW = {"PASN_WS": "0", "PASN_NO_PWTINY": "1", "PASN_NO_PWCONV": "1", "PASN_NO_XTILE": "1"}  # every pointwise rung above gemm_conv_kernel off
_GENERIC = dict(_NO_PW, PASN_NO_GEMM="1", PASN_NO_IGEMM="1")                                   # ... and the GEMM rungs: conv3d_mfma_kernel
_T3, _PT = dict(k=(3, 1, 1), p=(1, 0, 0)), dict(k=(1, 3, 3), p=(0, 1, 1))                       # the R(2+1)D temporal / spatial windows

CASES = [
    # ---- pwconv_ws_kernel<KS,MT,transform,residual> (bf16, 32 * PT * MT row tiles, a clip holds at least one tile) -------------------------
    _c("ws_54_24_res", 54, 24, (3, 2, 12, 11), "pwconv_ws_kernel<4,1,false,true>", res=True),                       # X3D stage-2 project; 256-row tiles, clips of 264
    _c("ws_108_48_res", 108, 48, (3, 2, 9, 8), "pwconv_ws_kernel<8,1,false,true>", res=True),                       # stage-3 project; 128-row tiles, clips of 144
    _c("ws_48_216", 48, 216, (3, 3, 5, 5), "pwconv_ws_kernel<4,2,false,false>"),                                    # expand, 7 channel tiles; 64-row tiles, clips of 75
    _c("ws_96_432", 96, 432, (2, 3, 5, 5), "pwconv_ws_kernel<6,2,false,false>"),                                    # 14 channel tiles in two groups
    _c("ws_432_192_gate_res", 432, 192, (3, 3, 5, 5), "pwconv_ws_kernel<28,1,true,true>", res=True, gate=True),     # stage-5 project, gated; 64-row tiles
    _c("ws_216_30_gate_sigmoid", 216, 30, (3, 3, 9, 11), "pwconv_ws_kernel<14,1,true,false>", act="sigmoid", gate=True, env={"PASN_WS": "2"}),
    _c("ws_108_45_swish_res", 108, 45, (3, 2, 9, 8), "pwconv_ws_kernel<8,1,true,true>", act="none", res=True, in_swish=True, env={"PASN_WS": "2"}),
    # ---- pwconv_persist_kernel<T,KS,NT,residual> (32-row tiles, any clip length) ----------------------------------------------------------
    _c("persist_54_24_gate_res", 54, 24, (3, 1, 5, 5), "pwconv_persist_kernel<bf16,4,1,true>", res=True, gate=True),
    _c("persist_108_48_gate_res", 108, 48, (3, 1, 5, 7), "pwconv_persist_kernel<bf16,8,2,true>", res=True, gate=True),
    _c("persist_128_30", 128, 30, (3, 2, 5, 5), "pwconv_persist_kernel<bf16,8,1,false>", act="abs"),                # head B's last occurrence conv
    _c("persist_54_30_sigmoid", 54, 30, (2, 1, 7, 5), "pwconv_persist_kernel<bf16,4,1,false>", act="sigmoid"),
    _c("persist_f32_24_54", 24, 54, (3, 1, 5, 7), "pwconv_persist_kernel<f32,4,2,false>", dtype="f32"),
    _c("persist_f32_54_24_gate_res", 54, 24, (3, 1, 5, 5), "pwconv_persist_kernel<f32,8,1,true>", res=True, gate=True, dtype="f32"),
    _c("persist_f32_24_108", 24, 108, (2, 1, 7, 5), "pwconv_persist_kernel<f32,4,4,false>", dtype="f32"),
    _c("persist_f32_30_45_sigmoid", 30, 45, (2, 1, 7, 5), "pwconv_persist_kernel<f32,4,2,false>", act="sigmoid", dtype="f32"),
    # ---- pwconv_tiny_kernel<T> (one wave per 32 x 32 output tile) --------------------------------------------------------------------
    _c("tiny_bf16_256_40", 256, 40, (3, 1, 5, 5), "pwconv_tiny_kernel<bf16>", act="none"),
    _c("tiny_bf16_270_45_sigmoid_res", 270, 45, (3, 1, 5, 5), "pwconv_tiny_kernel<bf16>", act="sigmoid", res=True),
    _c("tiny_f32_96_216", 96, 216, (3, 1, 5, 5), "pwconv_tiny_kernel<f32>", dtype="f32"),
    _c("tiny_f32_108_30_sigmoid_res", 108, 30, (3, 1, 5, 5), "pwconv_tiny_kernel<f32>", act="sigmoid", res=True, dtype="f32"),
    # ---- pwconv_xtile_kernel<T,KS,transform> (64-row tiles, a clip holds at least one) -------------------------------------------------
    _c("xtile_48_108", 48, 108, (3, 3, 5, 5), "pwconv_xtile_kernel<bf16,4,false>"),
    _c("xtile_96_192_stride", 96, 192, (3, 2, 13, 11), "pwconv_xtile_kernel<bf16,6,false>", act="none", s=(1, 2, 2)),  # strided shortcut, odd planes
    _c("xtile_108_48", 108, 48, (3, 3, 5, 5), "pwconv_xtile_kernel<bf16,8,false>", act="none"),
    _c("xtile_180_256", 180, 256, (2, 3, 5, 5), "pwconv_xtile_kernel<bf16,12,false>"),                              # head convs behind the X3D trunk
    _c("xtile_256_250_sigmoid", 256, 250, (2, 3, 5, 5), "pwconv_xtile_kernel<bf16,16,false>", act="sigmoid", env={"PASN_NO_PWTINY": "1"}),
    _c("xtile_216_96_res", 216, 96, (3, 3, 5, 5), "pwconv_xtile_kernel<bf16,14,false>", res=True, env={"PASN_WS": "0"}),       # not in a default plan
    _c("xtile_432_192_res", 432, 192, (3, 3, 5, 5), "pwconv_xtile_kernel<bf16,28,false>", res=True, env={"PASN_WS": "0", "PASN_NO_PWTINY": "1"}),
    _c("xtile_108_48_gate_res", 108, 48, (3, 3, 5, 5), "pwconv_xtile_kernel<bf16,8,true>", res=True, gate=True, env={"PASN_XTILE_GATED": "1"}),
    _c("xtile_f32_24_24_stride", 24, 24, (3, 2, 13, 11), "pwconv_xtile_kernel<f32,16,false>", act="none", dtype="f32", s=(1, 2, 2)),
    _c("xtile_f32_108_48_gate_res", 108, 48, (3, 3, 5, 5), "pwconv_xtile_kernel<f32,16,true>", res=True, gate=True, dtype="f32"),
    _c("xtile_f32_216_96_gate_res", 216, 96, (3, 3, 5, 5), "pwconv_xtile_kernel<f32,28,true>", res=True, gate=True, dtype="f32"),
    _c("xtile_f32_180_250_sigmoid", 180, 250, (2, 3, 5, 5), "pwconv_xtile_kernel<f32,28,false>", act="sigmoid", dtype="f32", env={"PASN_NO_PWTINY": "1"}),
    # ---- tconv_ws_kernel<KSF,residual> (bf16 (3,1,1) convs, T-marching; tiles of a frame's positions) --------------------------------------
    _c("tconv_45_64", 45, 64, (2, 3, 9, 11), "tconv_ws_kernel<3,false>", **_T3),                                    # R(2+1)D stem; frames of 99 positions
    _c("tconv_64_30_sigmoid", 64, 30, (2, 4, 9, 11), "tconv_ws_kernel<4,false>", act="sigmoid", **_T3),
    _c("tconv_144_64", 144, 64, (2, 3, 9, 11), "tconv_ws_kernel<9,false>", **_T3),
    _c("tconv_144_64_res", 144, 64, (2, 5, 9, 7), "tconv_ws_kernel<9,true>", res=True, **_T3),
    # ---- igemm_glds_kernel<NT,MT> / igemm_halo_kernel<NT,MT,mode> (bf16 windowed convs) --------------------------------------------------
    _c("igemm_64_230_stride", 64, 230, (2, 2, 9, 11), "igemm_glds_kernel<4,1>", s=(1, 2, 2), **_PT),
    _c("igemm_30_144_stride_res", 30, 144, (2, 2, 9, 11), "igemm_glds_kernel<5,1>", s=(1, 2, 2), res=True, **_PT),
    _c("igemm_45_30_stride_sigmoid", 45, 30, (2, 3, 9, 7), "igemm_glds_kernel<2,1>", act="sigmoid", s=(2, 1, 1), **_T3),
    _c("halo_64_64", 64, 64, (3, 1, 9, 11), "igemm_halo_kernel<2,1,0>", res=True, **_PT),                           # ResNet-18 basic block
    _c("halo_45_230", 45, 230, (2, 2, 9, 11), "igemm_halo_kernel<4,1,0>", **_PT),
    _c("halo_54_288_sigmoid", 54, 286, (2, 2, 9, 11), "igemm_halo_kernel<5,1,0>", act="sigmoid", **_PT),
    _c("halo_230_128_t", 230, 128, (2, 5, 5, 7), "igemm_halo_kernel<4,1,1>", res=True, **_T3),
    _c("halo_24_144_big", 24, 144, (2, 8, 131, 63), "igemm_halo_kernel<5,2,0>", **_PT),                             # MT = 2 needs >= 130817 rows
    # ---- gemm_conv_kernel<T,pointwise> (LDS-tiled GEMM; 64- and 128-column tiles) ----------------------------------------------------------
    _c("gemm_bf16_128_100", 128, 100, (3, 1, 5, 5), "gemm_conv_kernel<bf16,true>", act="sigmoid"),                  # clips of 25 positions: no X tile
    _c("gemm_bf16_108_45_gate_res", 108, 45, (3, 1, 5, 5), "gemm_conv_kernel<bf16,true>", res=True, gate=True, env=_NO_PW),
    _c("gemm_bf16_64_230_stride", 64, 230, (3, 1, 9, 7), "gemm_conv_kernel<bf16,false>", act="none", s=(1, 2, 2)),  # ResNet-18 downsample conv
    _c("gemm_f32_432_192_gate_res", 432, 192, (3, 1, 5, 5), "gemm_conv_kernel<f32,true>", res=True, gate=True, dtype="f32"),
    _c("gemm_f32_45_64_t", 45, 64, (2, 3, 5, 7), "gemm_conv_kernel<f32,false>", dtype="f32", **_T3),
    _c("gemm_f32_64_144_s", 64, 140, (2, 2, 7, 5), "gemm_conv_kernel<f32,false>", act="sigmoid", res=True, dtype="f32", **_PT),
    _c("gemm_f32_64_128_333", 64, 128, (2, 4, 9, 7), "gemm_conv_kernel<f32,false>", act="swish", dtype="f32", k=(3, 3, 3), s=(2, 2, 2), p=(1, 1, 1)),
    # ---- conv3d_mfma_kernel<T,NT,MT> (generic; no default plan reaches NT = 3 / 4 any more) -----------------------------------------------
    _c("generic_24_48_stride", 24, 48, (2, 2, 9, 9), "conv3d_mfma_kernel<bf16,2,1>", act="none", s=(1, 2, 2)),
    _c("generic_f32_24_48_stride", 24, 48, (2, 2, 9, 9), "conv3d_mfma_kernel<f32,2,1>", act="none", dtype="f32", s=(1, 2, 2)),
    _c("generic_16_30_t_sigmoid", 16, 30, (2, 3, 5, 7), "conv3d_mfma_kernel<bf16,1,1>", act="sigmoid", res=True, **_T3),
    _c("generic_432_192_nt3", 432, 192, (2, 1, 5, 5), "conv3d_mfma_kernel<bf16,3,1>", act="sigmoid", env=_GENERIC),  # many k-steps, 6 output tiles
    _c("generic_f32_432_192_nt3", 432, 192, (2, 1, 5, 5), "conv3d_mfma_kernel<f32,3,1>", act="sigmoid", dtype="f32", env=_GENERIC),
    _c("generic_216_216_nt4", 216, 216, (2, 2, 6, 6), "conv3d_mfma_kernel<bf16,4,1>", act="abs", env=_GENERIC),      # 7 output tiles: two chunks of NT = 4
    _c("generic_f32_216_216_nt4", 216, 216, (2, 2, 6, 6), "conv3d_mfma_kernel<f32,4,1>", act="abs", dtype="f32", env=_GENERIC),
    _c("generic_54_24_gate_res", 54, 24, (3, 1, 5, 5), "conv3d_mfma_kernel<bf16,1,1>", res=True, gate=True, env=_GENERIC),
    # MT = 2 (two position tiles per wave) is taken from 262144 rows on: a small-K temporal conv on two clips of 8 x 131 x 127
    _c("generic_12_40_t_big", 12, 40, (2, 8, 131, 127), "conv3d_mfma_kernel<bf16,2,2>", res=True, **_T3),
    _c("generic_f32_12_30_t_big", 12, 30, (2, 8, 131, 127), "conv3d_mfma_kernel<f32,1,2>", act="sigmoid", dtype="f32", **_T3),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def round_up(v, m):
    return (v + m - 1) // m * m


def out_extent(case):
    n, t, h, w = case.nthw
    return tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((t, h, w), case.k, case.s, case.p))


# ------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def tensors(case_id):
    """fp32 inputs of a row, drawn once: x (N,Cin,T,H,W), w, the norm's parameters, residual, gate rows (N,Cin)."""
    case = BY_ID[case_id]
    n, t, h, w = case.nthw
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    kk = case.cin * case.k[0] * case.k[1] * case.k[2]
    to, ho, wo = out_extent(case)
    return dict(x=torch.randn(n, case.cin, t, h, w, generator=g),
                w=torch.randn(case.cout, case.cin, *case.k, generator=g) * (1.5 / kk ** 0.5),
                gamma=torch.rand(case.cout, generator=g) + 0.5, beta=torch.randn(case.cout, generator=g) * 0.3,
                mean=torch.randn(case.cout, generator=g) * 0.3, var=torch.rand(case.cout, generator=g) + 0.5,
                res=torch.randn(n, case.cout, to, ho, wo, generator=g) if case.res else None,
                gate=torch.rand(n, case.cin, generator=g) + 0.25 if case.gate else None)


def modules(case):
    """The layer as torch modules (fp32 parameters): what ``PlanBuilder.conv`` takes."""
    T = tensors(case.id)
    conv = nn.Conv3d(case.cin, case.cout, case.k, case.s, case.p, bias=False)
    bn = nn.BatchNorm3d(case.cout)
    with torch.no_grad():
        conv.weight.copy_(T["w"])
        bn.weight.copy_(T["gamma"]), bn.bias.copy_(T["beta"]), bn.running_mean.copy_(T["mean"]), bn.running_var.copy_(T["var"])
    return conv, bn.eval()


# ------------------------------------------------------------------------------------------------- builder
Built = collections.namedtuple("Built", "pb x y name store binds")


def _channels_last(x, cp, dtype, device):
    n, c = x.shape[:2]
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=dtype, device=device)
    out[..., :c] = x.permute(0, 2, 3, 4, 1).to(device).to(dtype)
    return out


def build(case, device):
    """The row as a one-launch plan on ``device``, through ``PlanBuilder.conv`` only.  ``name`` is ``pb.meta[-1]["kernel"]``.  The caller
    holds the row's switches in force (``switches(case)``) around this AND around the launch."""
    from protoasnet_amd.plan import Act, PlanBuilder

    dtype, T = DT[case.dtype], tensors(case.id)
    conv, bn = modules(case)
    n, t, h, w = case.nthw
    pb = PlanBuilder(torch.device(device), dtype, dtype)
    cp = round_up(case.cin, 8)
    store = _channels_last(T["x"], cp, dtype, device)
    x = Act(n, t, h, w, case.cin, cp, pb._new_buf(store.numel() * store.element_size(), external=True))
    binds, ra, gbuf = [], None, None
    if case.res:
        rs = _channels_last(T["res"], round_up(case.cout, 8), dtype, device)
        ra = Act(n, *out_extent(case), case.cout, rs.shape[-1], pb._new_buf(rs.numel() * rs.element_size(), external=True))
        binds.append((ra.buf, rs))
    if case.gate:
        gt = torch.zeros(n, cp, dtype=torch.float32, device=device)
        gt[:, :case.cin] = T["gate"].to(device)
        gbuf = pb._new_buf(gt.numel() * 4, external=True)
        binds.append((gbuf, gt))
    y = pb.conv(x, conv.to(device), bn.to(device), case.act, residual=ra, in_gate=gbuf, in_swish=case.in_swish)
    return Built(pb, x, y, pb.meta[-1]["kernel"], store, binds)


def switches(case):
    """Context manager: the row's routing switches set, every other ``PASN_*`` variable of the environment cleared."""
    from protoasnet_amd import _lib

    kv = {k: None for k in os.environ if k.startswith("PASN_") and k != "PASN_PARITY_LOG"}
    kv.update(case.env)
    return _lib.tuning_env(**kv)


def launch(built):
    """Run the plan into an output full of NaN (an element the launch does not write stays NaN).  Returns [N][To][Ho][Wo][Cout_p]."""
    from protoasnet_amd import _lib

    plan = built.pb.finish(built.x, built.y)
    o = plan.out
    y = torch.full((o.N, o.T, o.H, o.W, o.Cp), float("nan"), dtype=plan.dtype, device=built.store.device)
    for buf, t in built.binds:
        plan.ptrs[buf] = t.data_ptr()
    plan.ptrs[plan.in_buf], plan.ptrs[plan.out_buf] = built.store.data_ptr(), y.data_ptr()
    for op in plan.ops:
        op(plan.ptrs, _lib.current_stream())
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------------------------- reference
def conv64(x, w, s, p, groups=1):
    """Exact dense conv in fp64: for every tap one matrix product [M][Cin] x [Cin][Cout].  x (N,Cin,T,H,W), w (Cout,Cin,kt,kh,kw).
    ``groups`` = Cin: the depthwise conv, w (C,1,kt,kh,kw), for every tap one product per channel."""
    n, cin, t, h, wd = x.shape
    cout, _, kt, kh, kw = w.shape
    assert groups == 1 or (groups == cin == cout and w.shape[1] == 1), "dense or depthwise"
    to, ho, wo = ((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((t, h, wd), (kt, kh, kw), s, p))
    xp = torch.nn.functional.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0])).permute(0, 2, 3, 4, 1)  # channels last
    out = torch.zeros(n * to * ho * wo, cout, dtype=F64)
    for a in range(kt):
        for b in range(kh):
            for c in range(kw):
                xs = xp[:, a:a + s[0] * (to - 1) + 1:s[0], b:b + s[1] * (ho - 1) + 1:s[1], c:c + s[2] * (wo - 1) + 1:s[2]]
                if groups != 1:
                    out += xs.reshape(-1, cin) * w[:, 0, a, b, c]
                    continue
                out += xs.reshape(-1, xs.shape[-1]) @ w[:, :, a, b, c].t()
    return out.view(n, to, ho, wo, cout).permute(0, 4, 1, 2, 3)


def folded(case):
    """(scale, bias) as the launch reads them: ``plan.fold_norm``'s fp32 values, in fp64."""
    from protoasnet_amd.plan import fold_norm

    _, bn = modules(case)
    scale, bias = fold_norm(bn, None, case.cout, case.cout, torch.device("cpu"))
    return scale.to(F64), bias.to(F64)


def transformed_input(case, gate_of_clip=None):
    """(x', flip): the operand the matrix cores read, fp64 values of the compute dtype, and how far a correct kernel's copy may be from it.
    ``gate_of_clip``: a (N,) index tensor, which clip's gate row each clip uses (the identity; a test's mutation passes another)."""
    dtype, T = DT[case.dtype], tensors(case.id)
    x = tk.rnd(T["x"], dtype)
    if not case.in_swish:
        return x, None
    v = x
    if case.gate:
        g = T["gate"].to(F64)
        if gate_of_clip is not None:
            g = g[gate_of_clip]
        v = x * g[:, :, None, None, None]
    xt = v * torch.sigmoid(v)
    eps = (8 + 2 * v.abs()) * 2.0 ** -24
    flip = (tk.rnd(xt * (1 + eps), dtype) - tk.rnd(xt * (1 - eps), dtype)).abs()
    return tk.rnd(xt, dtype), flip


def rounds_pre_sum(case):
    """The epilogue rounds norm(conv) to bf16 before the residual and the activation see it (module docstring, IMAGE)."""
    family = case.expect.split("<")[0]
    if case.dtype != "bf16" or not (case.res or case.act in ("sigmoid", "swish")):
        return False
    return family == "gemm_conv_kernel" or (case.res and family in ("pwconv_persist_kernel", "igemm_glds_kernel", "igemm_halo_kernel"))


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """ref, bound (N,Cout,To,Ho,Wo) fp64 and the quantities the bound is made of."""
    case = BY_ID[case_id]
    dtype, T = DT[case.dtype], tensors(case_id)
    xt, flip = transformed_input(case)
    w = tk.rnd(T["w"], dtype)
    scale, bias = folded(case)
    sc, bi = scale.view(1, -1, 1, 1, 1), bias.view(1, -1, 1, 1, 1)
    res = tk.rnd(T["res"], dtype) if case.res else None
    u = sc * conv64(xt, w, case.s, case.p) + bi
    A = sc.abs() * conv64(xt.abs(), w.abs(), case.s, case.p) + bi.abs()
    image = tk.BF16_STORE * u.abs() if rounds_pre_sum(case) else 0.0
    if res is not None:
        u, A = u + res, A + res.abs()
    ref = ACT[case.act](u)
    kk = round_up(case.cin, 8) * case.k[0] * case.k[1] * case.k[2]
    pre = 2 * kk * 2.0 ** -24 * A + image
    if flip is not None:
        pre = pre + sc.abs() * conv64(flip, w.abs(), case.s, case.p)
    store = tk.BF16_STORE if dtype == torch.bfloat16 else 2.0 ** -23
    bound = store * ref.abs() + LIPSCHITZ[case.act] * pre
    if case.act in ("sigmoid", "swish"):
        bound = bound + (2.0 ** -21 + u.abs() * 2.0 ** -24) * ref.abs()
    return dict(ref=ref, bound=bound, u=u, A=A, at_risk=0.0 if flip is None else float((flip > 0).double().mean()))


# ------------------------------------------------------------------------------------------------- comparison
def check(case, out, name=None):
    """``out``: the launch's whole output [N][To][Ho][Wo][Cout_p].  Every element written; |out - ref| <= bound on the real channels (logged
    through ``assert_close`` as the ratio err / bound against 1); exact zeros in the padded channels."""
    R = reference(case.id)
    out = out.detach().cpu().to(F64)
    n = case.nthw[0]
    assert tuple(out.shape) == (n,) + out_extent(case) + (round_up(case.cout, 8),), tuple(out.shape)
    assert bool(torch.isfinite(out).all()), f"{case.id}: {int((~torch.isfinite(out)).sum())} elements unwritten or not finite"
    got = out[..., :case.cout].permute(0, 4, 1, 2, 3)
    err = (got - R["ref"]).abs()
    ratio = err / R["bound"].clamp_min(1e-300)
    i = int(ratio.argmax())
    label = (f"{name or case.expect} {case.id} max_err={float(err.max()):.3g} worst: err={float(err.flatten()[i]):.3g} "
             f"bound={float(R['bound'].flatten()[i]):.3g} |ref|={float(R['ref'].flatten()[i].abs()):.3g} max|ref|={float(R['ref'].abs().max()):.3g} (err / bound)")
    assert_close(ratio, torch.zeros_like(ratio), 1.0, 0.0, label)
    if out.shape[-1] > case.cout:
        assert float(out[..., case.cout:].abs().max()) == 0.0, f"{case.id}: padded channels must be exact zeros"
    return float(ratio.max())
