"""The depthwise half of the forward pass (``pasn_dwconv3d_fwd``, ``pasn_dwconv3d_se_fwd``, ``pasn_x3d_expdw_fwd``; ``dw_route`` in
csrc/conv.hip) case by case, pure torch on the CPU: one table of small layers, each pinned to the kernel instance it runs, with inputs, an
fp64 reference and a per-element error bound built from the reference alone.  The dense ladder's twin (tests/conv_kernel_cases.py, whose
helpers it uses); ``x3d_edp_kernel`` (a whole block, three rounding stages) and the backward stencils are not in this table.

Shared by tests/test_gpu_dw_cases.py, which runs the HIP kernels on these inputs, and tests/test_cpu_dw_kernel_cases.py, which checks
without a GPU that every row reaches the instance it names, that the table claims every depthwise instance the default plans launch, that
the reference stays within one weight rounding of conv3d(groups = C) + eval-mode BatchNorm3d and that the bound tells a correct kernel from a
subtly wrong one.

**Reference.**  fp64 on the operands exactly as the launch reads them: x rounded to the compute dtype, the norm as ``plan.fold_norm``'s fp32
(scale, bias), the stencil weights as the fp32 taps of ``pack_dw_taps`` -- and then the family's **operand model** (``operand_model``), the
rounding the kernel applies to the taps before they meet x:

    family                                   model     pool sums taken from               read at (protoasnet_amd/csrc)
    dwconv3d_kernel<T>                       none      fp32 pre-activation                conv.hip:334 (fmaf on the fp32 taps), :341-342
    dwconv3d_strip_kernel<T,WT,KW,SW>        none      fp32 pre-activation                conv.hip:472, :494-495
    dwconv3d_march_kernel<SW,WT> (and <SW,se>)  none   fp32 pre-activation                dwmarch.hip:175, :205-206
    dwconv_t_kernel<T,kt>                    none      (writes no pool rows)              dwtemporal.hip:55-56
    dwconv3d_mfma_kernel<RPT,false,ACT>      w         fp32 pre-activation                blockdiag.h:53 (bf16_bits(w)), :142, :152
    x3d_expdw_kernel<KS,ACT,SS>              w         fp32 pre-activation                x3d_expdw.hip:82 -> blockdiag.h:53, :142, :152
    dwconv3d_tz_kernel<ACT,false>            w*scale   --                                 toeplitz.h:91, :99 (bf16_bits(w * sw)), :149
    dwconv3d_tz_kernel<0,true>               w         the ROUNDED bf16 outputs           toeplitz.h:99 (sw = 1), :156, :167-176 (fdot2 of the stored pairs)
    dwconv3d_tz_kernel<3,true>               w         fp32 pre-activation                toeplitz.h:159-163
    x3d_expdw_tz_kernel<1,ACT,POOL>          as dwconv3d_tz_kernel<ACT,POOL>              x3d_expdw_tz.hip:155, :199 -> toeplitz.h

``none``: the fp32 taps as they are (the VALU families convert x to fp32 and use fmaf, whatever the compute dtype); ``w``: the taps rounded
to bf16, round-to-nearest-even (``plan.stencil_operands`` documents the same values), the norm's scale in fp32 behind the accumulator;
``w*scale``: the fp32 product w * scale rounded to bf16, no scale behind the accumulator and the bias as its initial value.  Then

    pre = scale_eff * sum(w_eff * x) + bias,   ref = act(pre)          (scale_eff = 1 under ``w*scale``, the folded scale otherwise)

so that the reference differs from a correct kernel only by accumulation order and the output store.  On ``expand`` rows x is the
intermediate of the fused 1x1x1 conv, e = rnd_bf16(relu(u_e)): u_e = conv1x1(x, rnd(wa * scale_a)) + bias_a under the default fold (the
plan rounds the fp32 product once, ``PlanBuilder.expand_dw``), u_e = scale_a * conv1x1(x, rnd(wa)) + bias_a under ``PASN_EXPDW_FOLD=0``
(x3d_expdw.hip:216-221; x3d_expdw_tz.hip:111-118 rounds before the ReLU, which is the same value: both are monotone and keep the sign).

**Bound**, per output element, from the reference's own quantities:

    bound = STORE * |ref|  +  L * (2 * taps * 2^-24 * A  +  flip_term)  +  (2^-21 + |pre| * 2^-24) * |ref|     [last term: swish / sigmoid]

``STORE``, ``L`` and the last term are conv_kernel_cases.py's: every depthwise epilogue computes swish as v * sigmoidf_(v) with the same
sigmoidf_ = v_rcp(1 + v_exp(-v)) (common.h:432; act_vec, bd_epilogue blockdiag.h:156, tz_stencil_step toeplitz.h:165).  A = |scale_eff| *
conv(|x|, |w_eff|) + |bias| bounds every partial sum of the ``taps`` terms (+ the bias) that meet in one fp32 accumulator; the factor 2
is the margin, as there.  ``flip_term`` is zero except on ``expand`` rows: the kernel's pre-rounding u_e is within eps_e = 2 * K * 2^-24 *
A_e of the reference's (K = Cin + 1 terms meet in the expand accumulator: the real input channels -- the padded ones add exact zeros -- and
the bias), rounding and ReLU are monotone, so its e lies between rnd(relu(u_e - eps_e)) and rnd(relu(u_e + eps_e)); flip = the distance of
the two, zero for all but the few elements within eps_e of a rounding boundary (or of the kink), and the term is |scale_b| * conv(flip,
|w_b|).  ``reference`` reports the share of elements with flip > 0; the CPU test asserts it below 1 % on every expand row.

**Pool partial rows.**  The launch is handed ``pool_blocks`` rows full of NaN.  Both consumers -- ``pasn_se_gate_fwd`` (conv.hip:1091-1112,
se_gate_kernel :596-609) and the weight-stationary prologue (pwconv_ws.hip:248-264) -- read every one of the Cp channels of every row, so
every element must come back finite.  The per-(clip, channel) sum over the rows is compared with the fp64 sum of pre over all P output
positions under  sum_p (2 * taps * 2^-24 * A + flip_term)  +  (P - 1) * 2^-24 * sum_p |pre|  (an fp32 sum of P terms in any order).  Where
the kernel sums its ROUNDED outputs (table above) the reference sums rnd_bf16(pre), and an element's share of the bound is
rnd(pre + d) - rnd(pre - d) with d its L = 1 bound without STORE: zero unless pre lies within d of a rounding boundary.
A fused gate (``se`` rows) is compared with sigmoid(fc2(relu(fc1(mean)))) in fp64; its bound carries the pool bound through the two FCs,
1/4 * |W2| @ (|W1| @ d_mean), plus their own fp32 accumulation terms and the sigmoid's.

Padded channels must read back as exact zeros, and nothing of the output may be left unwritten (the GPU test's output is full of NaN).

**Observed** on an MI355X (profiles/dw_ladder_parity_observed.tsv), largest err / bound per family, output | pool sums | gate:
dwconv3d_kernel 0.987 | 0.010; dwconv3d_strip_kernel 0.995 | 0.027; dwconv3d_march_kernel 0.994 | 0.012 | 0.009; dwconv_t_kernel 0.993;
dwconv3d_mfma_kernel 0.994 | 0.018; dwconv3d_tz_kernel 0.995 | 0.447; x3d_expdw_kernel 0.994 | 0.161; x3d_expdw_tz_kernel 0.995 | 0.025.  The
outputs' 0.99 is the bf16 rows' STORE term, which has no margin (2^-8 |ref| is half a spacing just above a power of two; the fp32 rows stay
below 0.42, the largest on the (kt,1,1) windows, whose bound is little more than the fp32 store); the Toeplitz kernel's 0.447 is a row whose pool sums are taken from the rounded outputs.  No row needed a rounding point
beyond the table above.

**Table.**  ``expect`` is the full instance name as ``plan.dwconv_kernel_name`` and ``PlanBuilder.expand_dw`` / ``dwconv_se`` print it;
``env`` holds the routing switches (the row is built AND launched under them).  Shapes: N >= 2 everywhere; channel counts with a partial
8-channel group (20, 54) and a partial 16-channel tile (24, 56, 108); T = 9 under forced chunks of 4 / 8 (halos, a partial last chunk), T = 1,
T shorter than the window; planes no multiple of a region, band or strip (5 x 7, 9 x 13, 11 x 13, 14 x 9, 13 x 17 -> 7 x 9); planes at most 8
wide and wider ones for the matrix-core stencil; Toeplitz planes without a second band (5 high), with a cut one (9, 11, 13 high) and the
tallest (14 high, 9 wide); rows with several pool partial rows.  The strip kernel's other (WT, KW, SW) instantiations have no row:
only ``PASN_DW_WT`` reaches them, a development override that is compiled out of the product library."""
import collections
import functools

import torch
import torch.nn as nn

import train_kernel_cases as tk
from conftest import assert_close
from conv_kernel_cases import ACT, DT, F64, LIPSCHITZ, conv64, round_up, switches  # noqa: F401  (switches: used by the tests)

Case = collections.namedtuple("Case", "id c k s p nthw act pool se expand dtype env expect")

K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
S2 = (1, 2, 2)


def _c(id, c, nthw, expect, act="none", pool=False, se=None, expand=None, dtype="bf16", k=K3, s=S1, p=P1, env=None):
    return Case(id, c, k, s, p, nthw, act, pool or se is not None, se, expand, dtype, dict(env or {}), expect)


_VALU = {"PASN_DWMFMA": "0"}                              # no matrix-core stencil (Toeplitz included): the T-marching VALU stencil
_STRIP = {"PASN_DWMFMA": "0", "PASN_NO_DWMARCH": "1"}     # ... and not that one either: the strip kernel on a bf16 3x3x3 layer
_BD = {"PASN_DW_TZ": "0"}                                 # planes 9 .. 14 wide on the block-diagonal matrix-core stencil
_PLANE = dict(k=(1, 3, 3), p=(0, 1, 1))                   # a (1,3,3) window: no T-marching kernel covers it
_T5, _T3 = dict(k=(5, 1, 1), p=(2, 0, 0)), dict(k=(3, 1, 1), p=(1, 0, 0))


def _m(wt, tc):
    return dict(_VALU, PASN_DWM_WT=str(wt), PASN_DWM_TC=str(tc))


def _f(tc, upb, **kv):
    return dict(kv, PASN_DWMFMA_TC=str(tc), PASN_DWMFMA_UPB=str(upb))


CASES = [
    # ---- dwconv3d_kernel<T> (128 positions per block; windows the strip kernel has no instance for) ----------------------------------------
    _c("gen_f32_20_k355", 20, (2, 3, 5, 7), "dwconv3d_kernel<f32>", act="swish", dtype="f32", k=(3, 5, 5), p=(1, 2, 2)),
    _c("gen_f32_24_k155_pool", 24, (2, 2, 5, 7), "dwconv3d_kernel<f32>", act="relu", pool=True, dtype="f32", k=(1, 5, 5), p=(0, 2, 2)),
    _c("gen_bf16_56_k355_pool", 56, (2, 3, 9, 13), "dwconv3d_kernel<bf16>", pool=True, k=(3, 5, 5), p=(1, 2, 2)),          # 351 positions: 3 pool rows
    _c("gen_bf16_54_k133_s3", 54, (2, 1, 11, 13), "dwconv3d_kernel<bf16>", act="swish", k=(1, 3, 3), s=(1, 3, 3), p=(0, 1, 1)),
    # ---- dwconv3d_strip_kernel<T,WT,KW,SW>: WT by the layer (stride 2: 4; Wo % 7 == 0: 7; else 8).  PASN_DW_WT, which would reach the other
    # (WT, KW, SW), is a development override (tune_dev): compiled out of the product library, so these ten are all a plan can launch -----
    _c("strip_f32_8_3_1", 20, (2, 2, 9, 13), "dwconv3d_strip_kernel<f32,8,3,1>", act="swish", pool=True, dtype="f32"),
    _c("strip_f32_7_3_1", 54, (2, 3, 5, 7), "dwconv3d_strip_kernel<f32,7,3,1>", pool=True, dtype="f32"),
    _c("strip_f32_8_3_1_t1", 24, (2, 1, 11, 13), "dwconv3d_strip_kernel<f32,8,3,1>", act="relu", dtype="f32"),
    _c("strip_f32_4_3_2", 54, (2, 3, 13, 17), "dwconv3d_strip_kernel<f32,4,3,2>", pool=True, dtype="f32", s=S2),
    _c("strip_f32_4_3_2_even", 20, (2, 2, 14, 9), "dwconv3d_strip_kernel<f32,4,3,2>", act="swish", dtype="f32", s=S2),
    _c("strip_f32_8_1_1_pool", 24, (2, 6, 4, 4), "dwconv3d_strip_kernel<f32,8,1,1>", pool=True, dtype="f32", **_T5),       # (kt,1,1) with pool rows
    _c("strip_f32_7_1_1", 20, (2, 2, 5, 7), "dwconv3d_strip_kernel<f32,7,1,1>", act="relu", dtype="f32", env={"PASN_DW_TEMPORAL": "0"}, **_T5),
    _c("strip_f32_7_1_1_k331", 54, (2, 3, 5, 7), "dwconv3d_strip_kernel<f32,7,1,1>", act="swish", pool=True, dtype="f32", k=(3, 3, 1), p=(1, 1, 0)),
    _c("strip_f32_520", 520, (2, 2, 5, 5), "dwconv3d_strip_kernel<f32,8,3,1>", pool=True, dtype="f32"),                     # > 512 channels: 65 channel groups
    _c("strip_bf16_8_3_1", 54, (2, 3, 9, 13), "dwconv3d_strip_kernel<bf16,8,3,1>", act="swish", pool=True, env=_STRIP),
    _c("strip_bf16_7_3_1", 20, (2, 2, 5, 7), "dwconv3d_strip_kernel<bf16,7,3,1>", pool=True, **_PLANE),
    _c("strip_bf16_8_3_1_t1", 56, (2, 1, 11, 13), "dwconv3d_strip_kernel<bf16,8,3,1>", act="relu", env=_STRIP),
    _c("strip_bf16_4_3_2", 54, (2, 2, 13, 17), "dwconv3d_strip_kernel<bf16,4,3,2>", pool=True, s=S2, **_PLANE),
    _c("strip_bf16_4_3_2_even", 24, (2, 3, 14, 9), "dwconv3d_strip_kernel<bf16,4,3,2>", act="swish", pool=True, s=S2, env=_STRIP),
    _c("strip_bf16_8_1_1_pool", 24, (2, 6, 4, 4), "dwconv3d_strip_kernel<bf16,8,1,1>", pool=True, **_T5),
    _c("strip_bf16_7_1_1", 54, (2, 2, 5, 7), "dwconv3d_strip_kernel<bf16,7,1,1>", act="swish", env={"PASN_DW_TEMPORAL": "0"}, **_T3),
    _c("strip_bf16_8_1_1_k331", 20, (2, 3, 14, 9), "dwconv3d_strip_kernel<bf16,8,1,1>", pool=True, k=(3, 3, 1), p=(1, 1, 0)),
    _c("strip_bf16_520", 520, (2, 2, 5, 5), "dwconv3d_strip_kernel<bf16,8,3,1>", act="swish", pool=True, **_PLANE),
    # ---- dwconv3d_march_kernel<SW,WT> (bf16 3x3x3, T-marching VALU stencil; PASN_DWM_TC 4 / 8 / 16 on T = 9) ------------------------------
    _c("march_1_2_tc4", 56, (2, 9, 11, 13), "dwconv3d_march_kernel<1,2>", act="swish", pool=True, env=_m(2, 4)),
    _c("march_1_2_tc8", 20, (2, 9, 5, 7), "dwconv3d_march_kernel<1,2>", pool=True, env=_m(2, 8)),
    _c("march_1_2_tc16_t1", 54, (2, 1, 14, 9), "dwconv3d_march_kernel<1,2>", act="relu", pool=True, env=_m(2, 16)),
    _c("march_1_3_tc4", 24, (2, 9, 9, 13), "dwconv3d_march_kernel<1,3>", pool=True, env=_m(3, 4)),
    _c("march_1_3_tc8", 108, (2, 9, 5, 7), "dwconv3d_march_kernel<1,3>", act="swish", pool=True, env=_m(3, 8)),
    _c("march_1_3_tc16", 20, (2, 9, 11, 13), "dwconv3d_march_kernel<1,3>", pool=True, env=_m(3, 16)),
    _c("march_2_2_tc4", 54, (2, 9, 13, 17), "dwconv3d_march_kernel<2,2>", pool=True, s=S2, env={"PASN_DWM_TC": "4"}),
    _c("march_2_2_tc8", 108, (2, 9, 11, 13), "dwconv3d_march_kernel<2,2>", act="swish", pool=True, s=S2, env={"PASN_DWM_TC": "8"}),
    _c("march_2_2_tc16_t2", 24, (3, 2, 5, 7), "dwconv3d_march_kernel<2,2>", act="relu", s=S2, env={"PASN_DWM_TC": "16"}),
    _c("march_2_2_216", 216, (2, 4, 14, 14), "dwconv3d_march_kernel<2,2>", pool=True, s=S2),                               # stage 4's first block, its own split
    # ---- the fused stencil + gate launch (dwconv3d_march_kernel; the clip's last-arriving block computes the gate) -------------------------
    _c("se_2_2_54", 54, (2, 5, 13, 17), "dwconv3d_march_kernel<2,2>", se=8, s=S2, env={"PASN_DWM_TC": "4"}),
    _c("se_1_3_24", 24, (2, 9, 9, 13), "dwconv3d_march_kernel<1,3>", se=8, env=_m(3, 4)),
    _c("se_1_2_20", 20, (3, 2, 5, 7), "dwconv3d_march_kernel<1,2>", se=4, env=_m(2, 16)),
    _c("se_1_se_108", 108, (2, 3, 11, 13), "dwconv3d_march_kernel<1,se>", se=8, env={"PASN_DWMFMA_MAXW": "8"}),            # the plain launch is the Toeplitz kernel's
    # ---- dwconv3d_mfma_kernel<RPT,false,ACT> (block-diagonal matrix-core stencil; regions of 7 x 14 / 8 x 8 outputs) ---------------------
    _c("mfma_2_0_24", 24, (2, 5, 5, 7), "dwconv3d_mfma_kernel<2,false,0>", pool=True),
    _c("mfma_2_3_108_tc4", 108, (2, 9, 7, 7), "dwconv3d_mfma_kernel<2,false,3>", act="swish", pool=True, env=_f(4, 1)),
    _c("mfma_2_r_56", 56, (2, 3, 14, 8), "dwconv3d_mfma_kernel<2,false,-1>", act="relu", pool=True),                       # two row regions, the second cut
    _c("mfma_2_0_20_t1", 20, (2, 1, 7, 7), "dwconv3d_mfma_kernel<2,false,0>", pool=True, env=_f(16, 2)),
    _c("mfma_1_3_56_tc4", 56, (2, 9, 9, 13), "dwconv3d_mfma_kernel<1,false,3>", act="swish", pool=True, env=_f(4, 3, **_BD)),
    _c("mfma_1_0_54", 54, (2, 3, 11, 13), "dwconv3d_mfma_kernel<1,false,0>", pool=True, env=_BD),
    _c("mfma_1_r_108", 108, (2, 2, 14, 9), "dwconv3d_mfma_kernel<1,false,-1>", act="relu", env=_BD),
    _c("mfma_1_3_20_wide", 20, (2, 2, 5, 17), "dwconv3d_mfma_kernel<1,false,3>", act="swish"),                              # two column regions, the second 3 wide
    _c("mfma_1_0_24_upb", 24, (2, 9, 9, 17), "dwconv3d_mfma_kernel<1,false,0>", pool=True, env=_f(2, 1000)),
    # ---- dwconv3d_tz_kernel<ACT,POOL> (Toeplitz form, planes 9 .. 14 wide; PASN_DWMFMA_TC 1 / 3) -------------------------------------------
    _c("tz_3_f_24_tc3", 24, (2, 7, 9, 13), "dwconv3d_tz_kernel<3,false>", act="swish", env={"PASN_DWMFMA_TC": "3"}),
    _c("tz_0_t_56_tc3", 56, (2, 7, 14, 9), "dwconv3d_tz_kernel<0,true>", pool=True, env={"PASN_DWMFMA_TC": "3"}),
    _c("tz_3_t_20_tc1", 20, (2, 3, 5, 14), "dwconv3d_tz_kernel<3,true>", act="swish", pool=True, env={"PASN_DWMFMA_TC": "1"}),
    _c("tz_0_f_108_t1", 108, (2, 1, 11, 13), "dwconv3d_tz_kernel<0,false>"),
    _c("tz_0_t_54", 54, (2, 4, 9, 9), "dwconv3d_tz_kernel<0,true>", pool=True),
    _c("tz_3_f_56_tc1", 56, (2, 2, 13, 11), "dwconv3d_tz_kernel<3,false>", act="swish", env={"PASN_DWMFMA_TC": "1"}),
    # ---- dwconv_t_kernel<T,kt> ((kt,1,1) windows, a thread marches along T) ----------------------------------------------------------
    _c("t_bf16_5", 24, (2, 6, 5, 5), "dwconv_t_kernel<bf16,5>", act="relu", **_T5),
    _c("t_bf16_5_t1", 20, (2, 1, 4, 7), "dwconv_t_kernel<bf16,5>", act="swish", **_T5),
    _c("t_f32_5_t2", 20, (2, 2, 3, 3), "dwconv_t_kernel<f32,5>", act="swish", dtype="f32", **_T5),
    _c("t_bf16_3", 54, (2, 7, 5, 6), "dwconv_t_kernel<bf16,3>", act="relu", **_T3),
    _c("t_f32_3_t1", 24, (2, 1, 4, 7), "dwconv_t_kernel<f32,3>", dtype="f32", **_T3),
    # ---- x3d_expdw_kernel<KS,ACT,SS> (expand conv + block-diagonal stencil; regions of 3 x 14 / 6 x 14 outputs; both forms of norm_a) -------
    _c("xe_2_0_2", 54, (2, 5, 13, 17), "x3d_expdw_kernel<2,0,2>", pool=True, expand=24, s=S2, env={"PASN_EXPDW_TC": "2"}),
    _c("xe_2_3_2", 108, (3, 3, 13, 17), "x3d_expdw_kernel<2,3,2>", act="swish", expand=24, s=S2),
    _c("xe_2_r_2", 40, (2, 3, 7, 9), "x3d_expdw_kernel<2,-1,2>", act="relu", expand=16, s=S2),
    _c("xe_2_0_2_nofold", 54, (2, 1, 14, 9), "x3d_expdw_kernel<2,0,2>", pool=True, expand=24, s=S2, env={"PASN_EXPDW_FOLD": "0"}),
    _c("xe_2_3_2_nofold", 72, (2, 3, 11, 16), "x3d_expdw_kernel<2,3,2>", act="swish", expand=8, s=S2, env={"PASN_EXPDW_FOLD": "0"}),
    _c("xe_2_r_2_nofold", 20, (2, 2, 5, 7), "x3d_expdw_kernel<2,-1,2>", act="relu", pool=True, expand=24, s=S2, env={"PASN_EXPDW_FOLD": "0"}),
    _c("xe_2_0_1", 54, (2, 2, 9, 57), "x3d_expdw_kernel<2,0,1>", pool=True, expand=24, env={"PASN_EXPDW_TZ": "0"}),
    _c("xe_2_3_1", 40, (2, 3, 7, 59), "x3d_expdw_kernel<2,3,1>", act="swish", expand=16, env={"PASN_EXPDW_TZ": "0", "PASN_EXPDW_TC": "2"}),
    _c("xe_2_0_1_nofold", 24, (2, 3, 5, 57), "x3d_expdw_kernel<2,0,1>", pool=True, expand=8, env={"PASN_EXPDW_FOLD": "0", "PASN_EXPDW_TC": "2"}),
    _c("xe_2_3_1_nofold", 54, (2, 1, 9, 57), "x3d_expdw_kernel<2,3,1>", act="swish", expand=24, env={"PASN_EXPDW_FOLD": "0"}),
    # ---- x3d_expdw_tz_kernel<1,ACT,POOL> (expand conv + Toeplitz stencil, stride 1, planes >= 56 wide; regions of 8 x 28 outputs) ---------
    _c("xtz_3_f", 54, (2, 3, 9, 57), "x3d_expdw_tz_kernel<1,3,false>", act="swish", expand=24, env={"PASN_EXPDW_TC": "2"}),
    _c("xtz_0_t", 54, (2, 3, 9, 59), "x3d_expdw_tz_kernel<1,0,true>", pool=True, expand=24, env={"PASN_EXPDW_TC": "2"}),
    _c("xtz_3_t", 24, (2, 1, 9, 57), "x3d_expdw_tz_kernel<1,3,true>", act="swish", pool=True, expand=8),
    _c("xtz_0_f", 40, (2, 2, 5, 70), "x3d_expdw_tz_kernel<1,0,false>", expand=16),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

def family(case):
    return case.expect.split("<")[0]


def out_extent(case):
    n, t, h, w = case.nthw
    return tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((t, h, w), case.k, case.s, case.p))


def t_chunk(case):
    """The forced T chunk of the row (output frames), or None: the kernel's own split."""
    for key in ("PASN_DWM_TC", "PASN_DWMFMA_TC", "PASN_EXPDW_TC"):
        if key in case.env:
            return int(case.env[key])
    return None


def operand_model(case):
    """(weight model, pool sums taken from the rounded outputs): the table of the module docstring."""
    fam = family(case)
    if fam in ("dwconv3d_tz_kernel", "x3d_expdw_tz_kernel"):
        return ("w" if case.pool else "w*scale"), (case.pool and case.act == "none")
    if fam in ("dwconv3d_mfma_kernel", "x3d_expdw_kernel"):
        return "w", False
    assert fam in ("dwconv3d_kernel", "dwconv3d_strip_kernel", "dwconv3d_march_kernel", "dwconv_t_kernel"), fam
    return "none", False


# ------------------------------------------------------------------------------------------------- inputs
def _norm_params(c, g):
    return dict(gamma=torch.rand(c, generator=g) + 0.5, beta=torch.randn(c, generator=g) * 0.3, mean=torch.randn(c, generator=g) * 0.3,
                var=torch.rand(c, generator=g) + 0.5)


@functools.lru_cache(maxsize=None)
def tensors(case_id):
    """fp32 inputs of a row, drawn once: x (N,Cin,T,H,W), the stencil taps w (C,1,kt,kh,kw) and norm; wa (C,Cin) and norm_a of an
    ``expand`` row; the two FCs of an ``se`` row."""
    case = BY_ID[case_id]
    n, t, h, w = case.nthw
    g = torch.Generator().manual_seed(3000 + CASES.index(case))
    cin = case.expand or case.c
    taps = case.k[0] * case.k[1] * case.k[2]
    T = dict(x=torch.randn(n, cin, t, h, w, generator=g), w=torch.randn(case.c, 1, *case.k, generator=g) * (1.5 / taps ** 0.5), bn=_norm_params(case.c, g))
    if case.expand:
        T.update(wa=torch.randn(case.c, cin, generator=g) * (1.5 / cin ** 0.5), bn_a=_norm_params(case.c, g))
    if case.se:
        T.update(w1=torch.randn(case.se, case.c, generator=g) * 0.2, b1=torch.randn(case.se, generator=g) * 0.2,
                 w2=torch.randn(case.c, case.se, generator=g) * 0.2, b2=torch.randn(case.c, generator=g) * 0.2)
    return T


def _bn(c, q):
    bn = nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.copy_(q["gamma"]), bn.bias.copy_(q["beta"]), bn.running_mean.copy_(q["mean"]), bn.running_var.copy_(q["var"])
    return bn.eval()


def modules(case):
    """The row as torch modules (fp32 parameters): dict(conv, bn[, conv_a, bn_a][, fc1, fc2]), what the ``PlanBuilder`` methods take."""
    T = tensors(case.id)
    conv = nn.Conv3d(case.c, case.c, case.k, case.s, case.p, groups=case.c, bias=False)
    with torch.no_grad():
        conv.weight.copy_(T["w"])
    m = dict(conv=conv, bn=_bn(case.c, T["bn"]))
    if case.expand:
        m["conv_a"] = nn.Conv3d(case.expand, case.c, 1, bias=False)
        with torch.no_grad():
            m["conv_a"].weight.copy_(T["wa"].view(case.c, case.expand, 1, 1, 1))
        m["bn_a"] = _bn(case.c, T["bn_a"])
    if case.se:
        m["fc1"], m["fc2"] = nn.Conv3d(case.c, case.se, 1), nn.Conv3d(case.se, case.c, 1)
        with torch.no_grad():
            m["fc1"].weight.copy_(T["w1"].view(case.se, case.c, 1, 1, 1)), m["fc1"].bias.copy_(T["b1"])
            m["fc2"].weight.copy_(T["w2"].view(case.c, case.se, 1, 1, 1)), m["fc2"].bias.copy_(T["b2"])
    return m


# ------------------------------------------------------------------------------------------------- builder
Built = collections.namedtuple("Built", "pb x y name kind store pool_buf pool_blocks gate_buf")
Ran = collections.namedtuple("Ran", "out pool gate")


def _channels_last(x, cp, dtype, device):
    n, c = x.shape[:2]
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=dtype, device=device)
    out[..., :c] = x.permute(0, 2, 3, 4, 1).to(device).to(dtype)
    return out


def build(case, device):
    """The row as a one-launch plan on ``device``, through ``PlanBuilder.dwconv`` / ``.dwconv_se`` / ``.expand_dw`` only.  ``name`` and
    ``kind`` are those of ``pb.meta[-1]``.  The caller holds the row's switches in force (``switches(case)``) around this AND the launch."""
    from protoasnet_amd.plan import ALIGN, Act, PlanBuilder

    dtype, T = DT[case.dtype], tensors(case.id)
    m = {k: v.to(device) for k, v in modules(case).items()}
    n, t, h, w = case.nthw
    pb = PlanBuilder(torch.device(device), dtype, dtype)
    cin = case.expand or case.c
    cp = round_up(cin, 8)
    store = _channels_last(T["x"], cp, dtype, device)
    x = Act(n, t, h, w, cin, cp, pb._new_buf(store.numel() * store.element_size(), external=True))
    pool_buf, pool_blocks, gate_buf = None, 0, None
    if case.expand:
        got = pb.expand_dw(x, m["conv_a"], m["bn_a"], m["conv"], m["bn"], case.act, pool=case.pool)
        assert got is not None, f"{case.id}: the fused expand + stencil launch does not cover the row"
        y, pooled = got if case.pool else (got, None)
    elif case.se:
        y, gate_buf = pb.dwconv_se(x, m["conv"], m["bn"], m["fc1"], m["fc2"])
        assert isinstance(gate_buf, int) and len(pb.ops) == 1 and pb.meta[-1]["kind"] == "dwconv+se", f"{case.id}: not the fused stencil + gate launch"
        pool_buf, pool_blocks = gate_buf - 1, int(pb.lib.pasn_dwconv3d_se_pool_blocks(_desc_of(pb), pb.code))
        assert pb.bufs[pool_buf].nbytes == round_up(n * pool_blocks * y.Cp * 4, ALIGN), "the partial rows' buffer precedes the gate's"
        pooled = None
    else:
        got = pb.dwconv(x, m["conv"], m["bn"], case.act, pool=case.pool)
        y, pooled = got if case.pool else (got, None)
    if pooled is not None:
        pool_buf, pool_blocks = pooled[0], pooled[1]
    return Built(pb, x, y, pb.meta[-1]["kernel"], pb.meta[-1]["kind"], store, pool_buf, pool_blocks, gate_buf)


def _desc_of(pb):
    """The conv descriptor the fused stencil + gate launch keeps (``PlanBuilder.dwconv_se``)."""
    import ctypes

    from protoasnet_amd._lib import ConvDesc

    d = [k for k in pb.keep if isinstance(k, ConvDesc)]
    assert len(d) == 1
    return ctypes.byref(d[0])


def _arena_view(plan, buf, shape):
    off = plan.ptrs[buf] - plan.arena.data_ptr()
    count = 4
    for v in shape:
        count *= v
    return plan.arena[off:off + count].view(torch.float32).view(*shape)


def launch(built, twice=False):
    """Run the plan into an output, pool partial rows and a gate full of NaN (what the launch does not write stays NaN).  Returns ``Ran`` (out
    [N][To][Ho][Wo][Cp], pool [N][pool_blocks][Cp] or None, gate [N][Cp] or None); with ``twice`` a second ``Ran`` of the same launch
    repeated with nothing cleared in between, and the arrival counters as they read after either launch."""
    from protoasnet_amd import _lib

    plan = built.pb.finish(built.x, built.y)
    assert len(plan.ops) == 1
    o = plan.out
    y = torch.full((o.N, o.T, o.H, o.W, o.Cp), float("nan"), dtype=plan.dtype, device=built.store.device)
    plan.arena.fill_(0xFF)  # every fp32 of the arena (pool partial rows, gate) is a NaN
    plan.ptrs[plan.in_buf], plan.ptrs[plan.out_buf] = built.store.data_ptr(), y.data_ptr()

    def once():
        plan.ops[0](plan.ptrs, _lib.current_stream())
        torch.cuda.synchronize()
        pool = _arena_view(plan, built.pool_buf, (o.N, built.pool_blocks, o.Cp)).clone() if built.pool_buf is not None else None
        gate = _arena_view(plan, built.gate_buf, (o.N, o.Cp)).clone() if built.gate_buf is not None else None
        return Ran(y.clone(), pool, gate), (plan.se_counters.clone() if plan.se_counters is not None else None)

    first, c1 = once()
    if not twice:
        return first
    second, c2 = once()
    return first, second, (c1, c2)


# ------------------------------------------------------------------------------------------------- reference
def folded(bn_params, c):
    """(scale, bias) as the launch reads them: ``plan.fold_norm``'s fp32 values."""
    from protoasnet_amd.plan import fold_norm

    return fold_norm(_bn(c, bn_params), None, c, c, torch.device("cpu"))


def expand_fold(case):
    return case.env.get("PASN_EXPDW_FOLD", "1") != "0"


def stencil_input(case):
    """(x, flip) (N,C,T,H,W) fp64: what the stencil reads -- the input rounded to the compute dtype, or the intermediate e of the fused expand
    conv -- and how far a correct kernel's copy may be from it (None: not at all).  Also the share of elements with flip > 0."""
    dtype, T = DT[case.dtype], tensors(case.id)
    x = tk.rnd(T["x"], dtype)
    if not case.expand:
        return x, None
    sa, ba = folded(T["bn_a"], case.c)
    if expand_fold(case):  # the fp32 product W * scale rounded once (PlanBuilder.expand_dw), the bias the accumulator's initial value
        wa, post = tk.rnd(T["wa"] * sa.view(-1, 1), dtype), torch.ones(case.c, dtype=F64)
    else:
        wa, post = tk.rnd(T["wa"], dtype), sa.to(F64)
    post, ba = post.view(1, -1, 1, 1, 1), ba.to(F64).view(1, -1, 1, 1, 1)
    u = post * torch.einsum("ncthw,mc->nmthw", x, wa) + ba
    A = post.abs() * torch.einsum("ncthw,mc->nmthw", x.abs(), wa.abs()) + ba.abs()
    eps = 2 * (case.expand + 1) * 2.0 ** -24 * A
    e = tk.rnd(torch.relu(u), dtype)
    flip = (tk.rnd(torch.relu(u + eps), dtype) - tk.rnd(torch.relu(u - eps), dtype)).abs()
    return e, flip


def effective_taps(case):
    """(w_eff (C,1,kt,kh,kw), scale_eff, bias (C,)) fp64 under the row's operand model."""
    T = tensors(case.id)
    scale, bias = folded(T["bn"], case.c)
    model, _ = operand_model(case)
    w = T["w"].float()
    if model == "w":
        w = w.to(torch.bfloat16)
    elif model == "w*scale":
        w, scale = (w * scale.view(-1, 1, 1, 1, 1)).to(torch.bfloat16), torch.ones_like(scale)
    return w.to(F64), scale.to(F64), bias.to(F64)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """ref, bound (N,C,To,Ho,Wo) fp64, the pool sums and the gate with their bounds, and the quantities the bounds are made of."""
    case = BY_ID[case_id]
    dtype, T = DT[case.dtype], tensors(case_id)
    x, flip = stencil_input(case)
    w, scale, bias = effective_taps(case)
    sc, bi = scale.view(1, -1, 1, 1, 1), bias.view(1, -1, 1, 1, 1)
    pre = sc * conv64(x, w, case.s, case.p, groups=case.c) + bi
    A = sc.abs() * conv64(x.abs(), w.abs(), case.s, case.p, groups=case.c) + bi.abs()
    taps = case.k[0] * case.k[1] * case.k[2]
    d = 2 * taps * 2.0 ** -24 * A
    if flip is not None:
        d = d + sc.abs() * conv64(flip, w.abs(), case.s, case.p, groups=case.c)
    ref = ACT[case.act](pre)
    store = tk.BF16_STORE if dtype == torch.bfloat16 else 2.0 ** -23
    bound = store * ref.abs() + LIPSCHITZ[case.act] * d
    if case.act in ("sigmoid", "swish"):
        bound = bound + (2.0 ** -21 + pre.abs() * 2.0 ** -24) * ref.abs()
    R = dict(ref=ref, bound=bound, pre=pre, A=A, at_risk=0.0 if flip is None else float((flip > 0).double().mean()))
    if case.pool:
        P = pre[0, 0].numel()
        summed, share = pre, d
        if operand_model(case)[1]:  # the kernel sums its stored bf16 outputs
            summed, share = tk.rnd(pre, torch.bfloat16), tk.rnd(pre + d, torch.bfloat16) - tk.rnd(pre - d, torch.bfloat16)
        R["pool"] = summed.sum(dim=(2, 3, 4))
        R["pool_bound"] = share.sum(dim=(2, 3, 4)) + (P - 1) * 2.0 ** -24 * summed.abs().sum(dim=(2, 3, 4))
    if case.se:
        P = pre[0, 0].numel()
        w1, b1, w2, b2 = (T[k].to(F64) for k in ("w1", "b1", "w2", "b2"))
        mean = R["pool"] / P
        d_mean = R["pool_bound"] / P + 2 * 2.0 ** -24 * mean.abs()  # 1 / P rounded to fp32, and the product
        hid = torch.relu(mean @ w1.t() + b1)
        d_hid = d_mean @ w1.abs().t() + 2 * (case.c + 1) * 2.0 ** -24 * (mean.abs() @ w1.abs().t() + b1.abs())
        s = hid @ w2.t() + b2
        d_s = d_hid @ w2.abs().t() + 2 * (case.se + 1) * 2.0 ** -24 * (hid @ w2.abs().t() + b2.abs())
        R["gate"] = torch.sigmoid(s)
        R["gate_bound"] = 0.25 * d_s + (2.0 ** -21 + s.abs() * 2.0 ** -24) * R["gate"] + 2.0 ** -24 * R["gate"]
    return R


# ------------------------------------------------------------------------------------------------- comparison
def _ratio(got, want, bound, label):
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    assert_close(ratio, torch.zeros_like(ratio), 1.0, 0.0, f"{label} max_err={float(err.max()):.3g} worst: err={float(err.flatten()[i]):.3g} "
                 f"bound={float(bound.flatten()[i]):.3g} |ref|={float(want.flatten()[i].abs()):.3g} max|ref|={float(want.abs().max()):.3g} (err / bound)")
    return float(ratio.max())


def check(case, ran, name=None):
    """``ran``: the launch's ``Ran``.  The output: its shape, every element written, |out - ref| <= bound on the real channels (logged through
    ``assert_close`` as the ratio err / bound against 1), exact zeros in the padded channels.  The pool partial rows: every element finite,
    their per-(clip, channel) sums within the pool bound.  The gate: within its bound, zero in the padded channels.  Returns the largest ratio."""
    R = reference(case.id)
    n, c, cp = case.nthw[0], case.c, round_up(case.c, 8)
    tag = f"{name or case.expect} {case.id}"
    out = ran.out.detach().cpu().to(F64)
    assert tuple(out.shape) == (n,) + out_extent(case) + (cp,), tuple(out.shape)
    assert bool(torch.isfinite(out).all()), f"{case.id}: {int((~torch.isfinite(out)).sum())} elements unwritten or not finite"
    worst = _ratio(out[..., :c].permute(0, 4, 1, 2, 3), R["ref"], R["bound"], tag)
    if cp > c:
        assert float(out[..., c:].abs().max()) == 0.0, f"{case.id}: padded channels must be exact zeros"
    assert (ran.pool is not None) == case.pool, f"{case.id}: pool partial rows"
    if case.pool:
        pool = ran.pool.detach().cpu().to(F64)
        assert pool.dim() == 3 and pool.shape[0] == n and pool.shape[2] == cp and pool.shape[1] >= 1, tuple(pool.shape)
        assert bool(torch.isfinite(pool).all()), f"{case.id}: {int((~torch.isfinite(pool)).sum())} elements of the pool partial rows unwritten or not finite"
        worst = max(worst, _ratio(pool.sum(dim=1)[:, :c], R["pool"], R["pool_bound"], tag + " pool sums"))
    assert (ran.gate is not None) == (case.se is not None), f"{case.id}: gate"
    if case.se:
        gate = ran.gate.detach().cpu().to(F64)
        assert tuple(gate.shape) == (n, cp) and bool(torch.isfinite(gate).all()), f"{case.id}: gate unwritten or not finite"
        worst = max(worst, _ratio(gate[:, :c], R["gate"], R["gate_bound"], tag + " gate"))
        if cp > c:
            assert float(gate[:, c:].abs().max()) == 0.0, f"{case.id}: the gate's padded channels must be exact zeros"
    return worst
