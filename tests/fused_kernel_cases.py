"""The launches that fuse more than one layer (``PlanBuilder.conv_short`` / ``conv_se`` / ``conv_pair`` / ``x3d_edp`` / ``se_gate``) case by
case, pure torch on the CPU: the fourth table beside tests/conv_kernel_cases.py, tests/dw_kernel_cases.py and tests/stem_kernel_cases.py,
whose helpers it imports (``conv64``, ``ACT``, ``LIPSCHITZ``, ``round_up``, ``switches``, ``tk.rnd``, ``tk.BF16_STORE``).  One row per
instantiation the product library can launch, each pinned to the instance ``pb.meta[-1]["kernel"]`` names -- a name the library decodes from
the geometry the launch itself reads (``pasn_conv3d_se_variant`` and its five siblings, include/protoasnet_amd.h) -- with inputs, an fp64
reference and a per-element bound built from the reference alone.

Shared by tests/test_gpu_fused_cases.py, which runs the HIP kernels on these inputs, and tests/test_cpu_fused_kernel_cases.py, which checks
without a GPU that every row reaches the instance it names, that the four tables together claim every launch of the default plans, that
the reference is right and that the bound tells a correct kernel from a subtly wrong one.

**Forms** (``Case.form``) and the rounding points the reference follows, read from protoasnet_amd/csrc (all bf16; every folded norm is
``plan.fold_norm``'s fp32 (scale, bias), applied in fp32 BEHIND the accumulator -- none of these launches folds a scale into its weights):

    short     pwconv_persist_kernel<bf16,KS,NT,false,KS2>   y = relu(s1 (w1 . x') + s2 (w2 . x2[strided]) + (b1 + b2)): TWO accumulators (pwconv.hip:283,
              :303), o = acc * s1 + b (:333), o = fmaf(acc2, s2, o) (:338), activation, ONE store (:357; RCOPY is off without a residual).  scale2 is
              applied behind the shortcut's own accumulator, not folded; the bias is the fp32 sum the plan makes (plan.py, conv_short).
              x' = swish(x * gate) rounded to bf16 per k-step (:272-278).
    se        pwconv_ws_kernel<KS,MT,true,RES>[se]          gate = sigmoid(fc2(relu(fc1(mean)))) in fp32 from the stencil's pool partial rows
              (pwconv_ws.hip:248-303: rows summed in order, * 1/positions, fmaf chains + a shuffle tree); x' = swish(x * gate) rounded to bf16 in
              place (:192-198); v = acc * s + b (:385), + residual (:390), activation, one store (:396).
    pair      pwconv_ws_kernel<KS,1,XF,true,KS2>            the same first conv; its bf16 outputs (:396) are stored AND handed over in LDS (:401) as
              the second conv's operand: y2 = relu(acc2 * s2 + b2) (:435-440).
              pwconv_xpair_kernel<KS1,KS2,XF>               the same two stages (pwconv_xpair.hip:126-129 transform, :208-209 store + hand-over, :263).
    pair_se   pwconv_ws_kernel<KS,1,true,true,KS2>[se]      ``se`` + ``pair``.
    pe, pe_se x3d_pe_kernel<28,12,SE,MT>                    ``pair`` / ``pair_se`` with streamed weights: gate x3d_pe.hip:50-130 (pwconv_ws's prologue,
              thread for thread), transform :204-208, both convs xb_pointwise.h:68 (scale, bias), :74 (residual), :78 (ReLU, store, :83 hand-over).
              Without the gate the first conv reads its input as it is (pe_geom: in_swish comes with the gate only).
    edp       x3d_edp_kernel<12,28,NEXT>                    e = rnd(relu(acc * s_a + b_a)) (x3d_edp.hip:198-201; zeros outside the clip, :203);
              d = rnd(swish(S * s_d + b_d)) on the bf16 taps of ``plan.stencil_operands`` (:265-270); y = rnd(relu(acc * s_c + b_c + x)) (:338-343);
              the chained expand conv reads y's bf16 image (:345) through xb_pointwise.  Neither e nor d is ever stored.
    gate      se_gate_kernel (stand-alone)                  conv.hip:585-: ``pasn_se_gate_fwd`` runs se_gate_fast_kernel for Cse % 4 == 0 and se_gate_kernel
              otherwise; ``meta`` calls both "se_gate_kernel".  tests/dw_kernel_cases.py's ``se`` rows bound the gate FUSED into the stencil launch
              (kind ``dwconv+se``), not this launch: it is claimed here, one row per kernel.

**Reference.**  fp64 on the operands exactly as each stage reads them.  Nothing the kernel under test returns enters the bound, with the one
exception the project already uses (tests/test_gpu_pw_epilogue_cases.py): where a stage's input is a tensor that the same plan STORED in global
memory, the reference for that stage starts from that tensor as read back from the device --

* the second conv of a pair / of ``x3d_pe`` / the chained expand conv of ``x3d_edp`` starts from the stored y1 (which is itself bounded from the
  inputs);
* an ``se`` stage starts from the stencil launch's stored output and recomputes the gate in fp64 from the stored pool partial rows (the
  stencil launch is tests/dw_kernel_cases.py's subject, not this table's; its outputs must be finite).  The kernel's fp32 gate differs from
  that by at most dg = 1/4 (sum|w2| e_h + 2 (cse + 1) 2^-24 A_2) + (2^-21 + |z| 2^-24) g with e_h = 2 (C + blocks + 1) 2^-24 A_1, and the
  transformed operand's eps = (8 + 2 |v|) 2^-24 + (1 + |v|) dg / g gives ``flip`` as in the dense ladder (derivation: test_gpu_pw_epilogue_cases).

**Bound** per element: the ladder's

    bound = 2^-8 |ref|  +  L (2 K 2^-24 A  +  |scale| conv(flip, |w|))        (every output activation here is ReLU: L = 1, no sigmoid term)

``short``: one stage, K = both padded K extents, A = |s1| conv(|x'|, |w1|) + |s2| conv(|x2|, |w2|) + |b1 + b2|.  ``edp`` carries the flip
interval of dw_kernel_cases's ``expand`` rows through two unstored stages: e lies between rnd(relu(u_e -+ eps_e)), eps_e = 2 (Cin + 1)
2^-24 A_e; the stencil's pre-activation is then uncertain by d_pre = |s_d| conv(flip_e, |w_d|) + 2 * 27 * 2^-24 A_d, and d lies between
rnd(swish(pre) -+ dd), dd = 1.1 d_pre + (2^-21 + |pre| 2^-24) |swish(pre)| (Lipschitz form: swish is not monotone); flip_d enters the project
conv's bound.  ``reference`` reports the share of operands with non-zero flip per stage (``at_risk``).  Caps, asserted by the CPU test:

* below 2e-3 where the launch reads a gate tensor as it is (the other tables' cap; the single-stage rows);
* below 2 % where the launch computes the gate itself: dg / g is about 2e-5 at 432 channels (the factor 2 (C + blocks + 1) 2^-24 of e_h), so
  eps ~ 4e-5 against bf16's half spacing 2^-8.  That holds only for a gate whose dot products do not cancel: dg grows with the SUM OF
  MAGNITUDES of their terms, the gate's dependence on the clip with their sum.  With zero-mean FC weights the share was 80 % at 432 channels
  and the bound ten bf16 spacings wide (as loose as the tolerance this table replaces), so the SE rows draw clips of different brightness,
  taps with a positive sum, positive pooled means and FC weights, and a negative fc2 bias: gates of 0.2 .. 0.75 that differ by 0.06 .. 0.11
  between a row's first and last clip, and a bound of 1.0 .. 1.4 times the store term;
* ``edp`` rows: flip_e below 3.5 %, flip_d below 50 %.  Every flipped e moves the pre-activation of its 27 neighbours by about one spacing of
  d, so d's share is roughly 27 times e's whatever the inputs; what the inputs decide is how much each flip weighs.  With a zero-mean draw
  (A / |u| ~ 10 in both pointwise convs) the bound was 0.035 |ref| at the median, nine spacings.  The rows therefore use a post-ReLU block input
  and expand / project weights around a positive mean (A / |u| near 1), and in every eighth channel of both convs a running mean at the
  channel's typical conv value, so that both ReLUs still clip: the bound is then 1.3 .. 1.5 times the store term at the median.

Both sets of inputs were chosen on the CPU from the reference and the fp32 emulation alone; with them the bound fails every fault of the CPU
test's list (its part (c)) on every row.

Padded output channels must read back as exact zeros; every output -- y1 of a pair and the block output of ``block+expand`` included -- is
launched into a tensor full of NaN and must come back finite; the pool partial rows are handed to the stencil launch full of NaN.

**Observed** on an MI355X (profiles/fused_ladder_parity_observed.tsv), largest err / bound per family, first output | second output:
pwconv_persist_kernel 0.970; pwconv_ws_kernel[se] 0.991 | 0.978; pwconv_ws_kernel (pair) 0.970 | 0.984; pwconv_xpair_kernel 0.986 | 0.984;
x3d_pe_kernel 0.939 | 0.981; x3d_edp_kernel 0.896 | 0.970; the stand-alone gate 0.053.  The 0.9 .. 0.99 is the bf16 store term, which has no
margin (as on the other ladders); no row needed a rounding point beyond the list above, and no row exceeded 1.

**Table.**  Shapes are the smallest that still go wrong: N >= 2, rows no multiple of the tile, clips shorter than two tiles so that a tile
straddles two clips ((2,2,5,7): 70 positions against 64-row tiles; (3,1,5,7): 35 against x3d_pe's 32-row share; (3,1,9,11) -> 5 x 6: 30 against
pwconv_persist's 32-row tiles, odd planes under stride (1,2,2)), partial 8- and 16-channel chunks (54, 108, 210, 430 inner channels, shortcut
inputs of 20 and 40, middle widths 45 and 90 / 170) and padded outputs (20, 45, 100, 210, 420, 190).  ``x3d_pe_kernel`` needs Cout1_p % 16 == 0
(pe_geom): 180 middle channels pad to 184 and are NOT covered, so the odd row uses 430 -> 170 -> 420.  Three rows are large because the path
exists only there: ``edp_tpb2`` (N = 3, T = 172: 258 tiles, two per block) and ``pe_r33`` / ``pe_se_r33`` (8232 rows: R = 33, a second 32-row
sub-tile of one row).  **Not reachable at any shape:** two tiles per block in ``x3d_pe_kernel``.  pe_geom takes tpb = 2 above 32 768 rows,
where R = 128; its LDS layout (x3d_pe.hip:264-270) passes 160 KiB from R = 116 on at the only instantiated widths (Cin_p 417..448, Cout1_p
176 / 192), so every layer above 29 440 rows is declined and the tile loop never runs twice.  (Should that limit ever move: the loop keeps the
second gate row only if the block's FIRST tile touched the next clip, x3d_pe.hip:184-189 -- a later tile that straddles would read a row
nobody wrote.)"""
import collections
import functools

import torch
import torch.nn as nn

import train_kernel_cases as tk
from conftest import assert_close
from conv_kernel_cases import ACT, F64, LIPSCHITZ, conv64, round_up, switches  # noqa: F401  (switches: used by the tests)

BF16 = torch.bfloat16
S1, P0, S2 = (1, 1, 1), (0, 0, 0), (1, 2, 2)

Case = collections.namedtuple("Case", "id form c0 c1 c2 cx cse nthw gate res env expect")


def _c(id, form, c0, c1, nthw, expect, c2=0, cx=0, cse=0, gate=False, res=True, env=None):
    return Case(id, form, c0, c1, c2, cx, cse, nthw, gate, res, dict(env or {}), expect)


_WS_ALL = {"PASN_WS": "2"}
_WSPAIR_ALL = {"PASN_WSPAIR": "2"}
_XPAIR = {"PASN_WSPAIR": "0", "PASN_XPAIR_ALL": "1"}
_TC1 = {"PASN_DWMFMA_TC": "1"}  # the stencil launch ahead of an SE row: one frame per T chunk = one pool partial row per frame
A, B = (2, 2, 5, 7), (3, 1, 5, 7)


def _xp(ks1, ks2, c0, c1, c2):
    return [_c(f"xpair_{ks1}_{ks2}" + ("_gate" if g else ""), "pair", c0, c1, A, f"pwconv_xpair_kernel<{ks1},{ks2},{'true' if g else 'false'}>",
               c2=c2, gate=g, env=_XPAIR) for g in (False, True)]


CASES = [
    # ---- conv+shortcut: pwconv_persist_kernel<bf16,KS,NT,false,KS2>; shortcut input planes 9 x 11 -> 5 x 6 under stride (1,2,2) ---------------
    _c("short_4_1_2", "short", 54, 20, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,4,1,false,2>", cx=20, res=False),
    _c("short_4_1_2_gate", "short", 54, 24, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,4,1,false,2>", cx=20, gate=True, res=False),
    _c("short_8_2_2", "short", 108, 45, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,8,2,false,2>", cx=20, res=False),
    _c("short_8_2_2_gate", "short", 108, 48, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,8,2,false,2>", cx=24, gate=True, res=False),
    _c("short_8_2_4", "short", 108, 48, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,8,2,false,4>", cx=40, res=False),
    _c("short_8_2_4_gate", "short", 108, 45, (3, 1, 9, 11), "pwconv_persist_kernel<bf16,8,2,false,4>", cx=40, gate=True, res=False),
    # ---- conv+se: pwconv_ws_kernel<KS,MT,true,RES>[se]; the two production instances, then PASN_WS=2 ----------------------------------------
    _c("se_28_1", "se", 432, 192, A, "pwconv_ws_kernel<28,1,true,true>[se]", cse=32, env=_TC1),
    _c("se_14_1", "se", 210, 90, A, "pwconv_ws_kernel<14,1,true,true>[se]", cse=16, env=_TC1),
    _c("se_8_1", "se", 108, 45, (2, 3, 5, 9), "pwconv_ws_kernel<8,1,true,true>[se]", cse=8, env=dict(_WS_ALL, **_TC1)),      # 128-row tiles, clips of 135
    _c("se_14_1_nores", "se", 216, 30, A, "pwconv_ws_kernel<14,1,true,false>[se]", cse=16, res=False, env=dict(_WS_ALL, **_TC1)),
    _c("se_4_2", "se", 54, 156, A, "pwconv_ws_kernel<4,2,true,true>[se]", cse=8, env=dict(_WS_ALL, **_TC1)),                  # five channel tiles: MT = 2
    # ---- conv_pair: pwconv_ws_kernel<KS,1,XF,true,KS2> ------------------------------------------------------------------------------------
    _c("wspair_14_6", "pair", 210, 90, A, "pwconv_ws_kernel<14,1,false,true,6>", c2=210),
    _c("wspair_14_6_gate", "pair", 210, 90, A, "pwconv_ws_kernel<14,1,true,true,6>", c2=210, gate=True, env=_WSPAIR_ALL),
    _c("wspair_8_4", "pair", 108, 45, A, "pwconv_ws_kernel<8,1,false,true,4>", c2=100, env=_WSPAIR_ALL),
    _c("wspair_8_4_gate", "pair", 108, 45, A, "pwconv_ws_kernel<8,1,true,true,4>", c2=100, gate=True, env=_WSPAIR_ALL),
    # ---- conv_pair: pwconv_xpair_kernel<KS1,KS2,XF>; KS2 * 16 == ceil(Cout1_p / 32) * 32: 45 -> 4, 90 -> 6 ------------------------------------
    *_xp(8, 4, 108, 45, 100), *_xp(8, 6, 108, 90, 210), *_xp(14, 4, 210, 45, 100), *_xp(14, 6, 210, 90, 210),
    # ---- conv_pair+se: pwconv_ws_kernel<KS,1,true,true,KS2>[se] -------------------------------------------------------------------------------
    _c("wspair_se_14_6", "pair_se", 210, 90, A, "pwconv_ws_kernel<14,1,true,true,6>[se]", c2=210, cse=16, env=_TC1),
    _c("wspair_se_8_4", "pair_se", 108, 45, A, "pwconv_ws_kernel<8,1,true,true,4>[se]", c2=100, cse=8, env=dict(_WSPAIR_ALL, **_TC1)),
    # ---- x3d_pe_kernel<28,12,SE,MT> -----------------------------------------------------------------------------------------------------------
    _c("pe_4", "pe", 432, 192, B, "x3d_pe_kernel<28,12,false,4>", c2=432),
    _c("pe_2", "pe", 430, 170, B, "x3d_pe_kernel<28,12,false,2>", c2=420, env={"PASN_PE_MT": "2"}),
    _c("pe_se_4", "pe_se", 430, 170, A, "x3d_pe_kernel<28,12,true,4>", c2=420, cse=32, env=_TC1),
    _c("pe_se_2", "pe_se", 432, 192, A, "x3d_pe_kernel<28,12,true,2>", c2=432, cse=16, env=dict(_TC1, PASN_PE_MT="2")),
    _c("pe_r33", "pe", 432, 192, (6, 28, 7, 7), "x3d_pe_kernel<28,12,false,2>", c2=432, env={"PASN_PE_MT": "2"}),             # 8232 rows: R = 33
    _c("pe_se_r33", "pe_se", 432, 192, (6, 28, 7, 7), "x3d_pe_kernel<28,12,true,4>", c2=432, cse=32),                        # ... with the gate: the one-row sub-tile's clip
    # ---- x3d_edp_kernel<12,28,NEXT>: block width c0 (185 .. 192), inner width c1 (425 .. 432), next expand width c2 ---------------------------
    _c("edp_t1", "edp", 192, 432, (3, 1, 7, 7), "x3d_edp_kernel<12,28,false>"),
    _c("edp_t2_next", "edp", 190, 430, (2, 2, 7, 7), "x3d_edp_kernel<12,28,true>", c2=420),
    _c("edp_t3", "edp", 190, 430, (2, 3, 7, 7), "x3d_edp_kernel<12,28,false>"),
    _c("edp_t3_next", "edp", 192, 432, (2, 3, 7, 7), "x3d_edp_kernel<12,28,true>", c2=432),
    _c("edp_tpb2", "edp", 192, 432, (3, 172, 7, 7), "x3d_edp_kernel<12,28,true>", c2=432),                                  # 258 tiles, 25284 rows
    # ---- the stand-alone gate launch: se_gate_fast_kernel (Cse % 4 == 0) and se_gate_kernel, both "se_gate_kernel" in meta ----------------------
    _c("gate_fast", "gate", 216, 0, A, "se_gate_kernel", cse=16, res=False, env=_TC1),
    _c("gate_generic", "gate", 54, 0, A, "se_gate_kernel", cse=6, res=False, env=_TC1),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

KIND = {"short": "conv+shortcut", "se": "conv+se", "pair": "conv_pair", "pair_se": "conv_pair+se", "pe": "conv_pair", "pe_se": "conv_pair+se", "gate": "se_gate"}
SE_FORMS = ("se", "pair_se", "pe_se", "gate")


def kind(case):
    return KIND.get(case.form) or ("block+expand" if case.c2 else "block")


def family(case):
    return case.expect.split("<")[0] + ("[se]" if case.form in ("se", "pair_se", "pe_se") else "")


def out_thw(case):
    n, t, h, w = case.nthw
    return (t, (h - 1) // 2 + 1, (w - 1) // 2 + 1) if case.form == "short" else (t, h, w)


def outputs(case):
    """[(name, channels)] of the tensors the row's last launch writes, in stage order."""
    if case.form == "gate":
        return []
    first = case.c0 if case.form == "edp" else case.c1
    return [("y1", first)] + ([("y2", case.c2)] if case.c2 else [])


# ------------------------------------------------------------------------------------------------- inputs
def _norm_params(c, g):
    return dict(gamma=torch.rand(c, generator=g) + 0.5, beta=torch.randn(c, generator=g) * 0.3, mean=torch.randn(c, generator=g) * 0.3,
                var=torch.rand(c, generator=g) + 0.5)


def _apply_bn(v, q):
    return (v - q["mean"].view(1, -1, 1, 1, 1)) * (q["gamma"] / (q["var"] + 1e-5).sqrt()).view(1, -1, 1, 1, 1) + q["beta"].view(1, -1, 1, 1, 1)


def _pw(cout, cin, g):
    return torch.randn(cout, cin, 1, 1, 1, generator=g) * (1.5 / cin ** 0.5)


@functools.lru_cache(maxsize=None)
def tensors(case_id):
    """fp32 inputs of a row, drawn once."""
    case = BY_ID[case_id]
    n, t, h, w = case.nthw
    g = torch.Generator().manual_seed(5000 + CASES.index(case))
    to, ho, wo = out_thw(case)
    T = {}
    if case.form == "edp":
        # Inputs that keep the two unstored stages' flip intervals narrow (module docstring, Bound): a post-ReLU block input and expand / project
        # weights drawn around a positive mean, so that A / |u| stays near 1 in seven channels of eight; in every eighth channel of both
        # convs the norm's running mean is the channel's typical conv value, so that its pre-activations straddle zero and both ReLUs clip.
        T["x"] = torch.relu(torch.randn(n, case.c0, t, h, w, generator=g))
        T.update(wa=torch.randn(case.c1, case.c0, 1, 1, 1, generator=g) * 0.06 + 0.08, bn_a=_norm_params(case.c1, g),
                 wb=torch.randn(case.c1, 1, 3, 3, 3, generator=g) * 0.25, bn_b=_norm_params(case.c1, g),
                 w1=torch.randn(case.c0, case.c1, 1, 1, 1, generator=g) * 0.05 + 0.03, bn1=_norm_params(case.c0, g))
        F = torch.nn.functional
        probe = T["x"][:1, :, :2]
        ca = F.conv3d(probe, T["wa"])
        T["bn_a"]["mean"][::8] = ca.mean(dim=(0, 2, 3, 4))[::8]
        dd = _apply_bn(F.conv3d(torch.relu(_apply_bn(ca, T["bn_a"])), T["wb"], padding=1, groups=case.c1), T["bn_b"])
        T["bn1"]["mean"][::8] = F.conv3d(dd * torch.sigmoid(dd), T["w1"]).mean(dim=(0, 2, 3, 4))[::8]
        if case.c2:
            T.update(w2=_pw(case.c2, case.c0, g), bn2=_norm_params(case.c2, g))
        return T
    T["x"] = torch.randn(n, case.c0, to, ho, wo, generator=g)
    if case.form in SE_FORMS:
        # A gate that differs from clip to clip by several per cent while its fp32 evaluation stays close to the fp64 one (dg, module docstring):
        # dg grows with the SUM OF MAGNITUDES of the two dot products' terms, the gate's dependence on the clip with their SUM, so the terms share a
        # sign -- clips of different brightness (a per-clip offset on x), taps with a positive sum, pooled means and FC weights above zero, and a
        # negative fc2 bias that centres the gate near one half.
        T["x"] = T["x"] + 0.4 * torch.arange(n).view(n, 1, 1, 1, 1) / (n - 1)
        T.update(wb=torch.randn(case.c0, 1, 3, 3, 3, generator=g) * 0.25 + 0.1, bn_b=_norm_params(case.c0, g),
                 fc1_w=torch.rand(case.cse, case.c0, generator=g) * (2.0 / case.c0), fc1_b=torch.randn(case.cse, generator=g) * 0.1,
                 fc2_w=torch.rand(case.c0, case.cse, generator=g) * (1.0 / case.cse), fc2_b=torch.randn(case.c0, generator=g) * 0.3 - 0.7)
        T["bn_b"].update(beta=torch.rand(case.c0, generator=g) * 0.5 + 0.5, mean=torch.randn(case.c0, generator=g) * 0.1)
    if case.form == "gate":
        return T
    T.update(w1=_pw(case.c1, case.c0, g), bn1=_norm_params(case.c1, g))
    if case.res:
        T["res"] = torch.randn(n, case.c1, to, ho, wo, generator=g)
    if case.gate:
        T["gate"] = torch.rand(n, case.c0, generator=g) + 0.25
    if case.form == "short":
        T.update(x2=torch.randn(n, case.cx, t, h, w, generator=g), w2=_pw(case.c1, case.cx, g), bn2=_norm_params(case.c1, g))
    elif case.c2:
        T.update(w2=_pw(case.c2, case.c1, g), bn2=_norm_params(case.c2, g))
    return T


def _bn(q):
    bn = nn.BatchNorm3d(q["gamma"].numel())
    with torch.no_grad():
        bn.weight.copy_(q["gamma"]), bn.bias.copy_(q["beta"]), bn.running_mean.copy_(q["mean"]), bn.running_var.copy_(q["var"])
    return bn.eval()


def _conv(w, stride=S1, groups=1, pad=0):
    conv = nn.Conv3d(w.shape[1] * groups, w.shape[0], tuple(w.shape[2:]), stride, pad, groups=groups, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    return conv


def modules(case):
    """The row as torch modules (fp32 parameters): what the ``PlanBuilder`` methods take."""
    T = tensors(case.id)
    m = {}
    if "wb" in T:
        m["conv_b"], m["bn_b"] = _conv(T["wb"], groups=T["wb"].shape[0], pad=1), _bn(T["bn_b"])
    if "wa" in T:
        m["conv_a"], m["bn_a"] = _conv(T["wa"]), _bn(T["bn_a"])
    if "w1" in T:
        m["conv1"], m["bn1"] = _conv(T["w1"]), _bn(T["bn1"])
    if "w2" in T:
        m["conv2"], m["bn2"] = _conv(T["w2"], S2 if case.form == "short" else S1), _bn(T["bn2"])
    if "fc1_w" in T:
        m["fc1"], m["fc2"] = nn.Conv3d(case.c0, case.cse, 1), nn.Conv3d(case.cse, case.c0, 1)
        with torch.no_grad():
            m["fc1"].weight.copy_(T["fc1_w"].view(case.cse, case.c0, 1, 1, 1)), m["fc1"].bias.copy_(T["fc1_b"])
            m["fc2"].weight.copy_(T["fc2_w"].view(case.c0, case.cse, 1, 1, 1)), m["fc2"].bias.copy_(T["fc2_b"])
    return m


# ------------------------------------------------------------------------------------------------- builder
Built = collections.namedtuple("Built", "pb first last name kind binds acts pool gate_buf")


def _channels_last(x, cp, dtype, device):
    n, c = x.shape[:2]
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=dtype, device=device)
    out[..., :c] = x.permute(0, 2, 3, 4, 1).to(device).to(dtype)
    return out


def build(case, device):
    """The row as a plan on ``device`` through the ``PlanBuilder`` methods the trunks use: the stencil launch that writes the pool partial rows
    (SE forms), then the launch under test, which is ``pb.meta[-1]``.  ``acts``: {name: Act} of the tensors ``launch`` captures (``ys``: the
    stencil's output; ``y1`` / ``y2``); ``pool``: (buffer, partial rows per clip).  The caller holds the row's switches in force around this
    AND around the launch."""
    from protoasnet_amd.plan import Act, PlanBuilder

    T = tensors(case.id)
    m = {k: v.to(device) for k, v in modules(case).items()}
    n = case.nthw[0]
    pb = PlanBuilder(torch.device(device), BF16, BF16)
    binds = []

    def ext(t5):
        store = _channels_last(t5, round_up(t5.shape[1], 8), BF16, device)
        a = Act(n, *t5.shape[2:], t5.shape[1], store.shape[-1], pb._new_buf(store.numel() * 2, external=True))
        binds.append((a.buf, store))
        return a

    xa = ext(T["x"])
    ra = ext(T["res"]) if "res" in T else None
    gbuf = None
    if case.gate:
        gt = torch.zeros(n, xa.Cp, dtype=torch.float32, device=device)
        gt[:, :case.c0] = T["gate"].to(device)
        gbuf = pb._new_buf(gt.numel() * 4, external=True)
        binds.append((gbuf, gt))
    acts, pool, gate_buf, src, pooled = {}, None, None, xa, None
    if case.form in SE_FORMS:
        src, pooled = pb.dwconv(xa, m["conv_b"], m["bn_b"], act="none", pool=True)
        acts["ys"], pool = src, (pooled[0], pooled[1])
    se = (pooled, m["fc1"], m["fc2"]) if pooled is not None else None
    if case.form == "short":
        y = pb.conv_short(xa, m["conv1"], m["bn1"], "relu", ext(T["x2"]), m["conv2"], m["bn2"], in_gate=gbuf, in_swish=case.gate)
        assert y is not None, f"{case.id}: the fused shortcut launch does not cover the row"
        acts["y1"] = y
    elif case.form == "se":
        y = pb.conv_se(src, m["conv1"], m["bn1"], "relu", ra, pooled, m["fc1"], m["fc2"])
        assert y is not None, f"{case.id}: the gate-in-prologue launch does not cover the row"
        acts["y1"] = y
    elif case.form in ("pair", "pair_se", "pe", "pe_se"):
        pair = pb.conv_pair(src, m["conv1"], m["bn1"], "relu", ra, m["conv2"], m["bn2"], "relu", in_gate=gbuf, in_swish=case.gate or se is not None, se=se)
        assert pair is not None, f"{case.id}: no chained launch covers the row"
        acts["y1"], acts["y2"] = pair
    elif case.form == "edp":
        out = pb.x3d_edp(xa, m["conv_a"], m["bn_a"], m["conv_b"], m["bn_b"], m["conv1"], m["bn1"], m.get("conv2"), m.get("bn2"))
        assert out is not None, f"{case.id}: the whole-block launch does not cover the row"
        acts["y1"] = out[0]
        if out[1] is not None:
            acts["y2"] = out[1]
    else:
        gate_buf = pb.se_gate(pooled, m["fc1"], m["fc2"])
    last = acts.get("y2") or acts.get("y1") or acts["ys"]
    return Built(pb, xa, last, pb.meta[-1]["kernel"], pb.meta[-1]["kind"], binds, acts, pool, gate_buf)


def launch(built):
    """Run the plan with every captured tensor, the pool partial rows and the gate full of NaN (what a launch does not write stays NaN).
    Returns {name: tensor on the CPU}: ``ys`` / ``y1`` / ``y2`` [N][T][H][W][Cp] bf16, ``pool`` [N][blocks][Cp] and ``gate`` [N][Cp] fp32."""
    from protoasnet_amd import _lib

    pb, dev = built.pb, built.binds[0][1].device
    held = {}
    for name, a in built.acts.items():
        pb.bufs[a.buf].external = True
        held[name] = (a.buf, torch.full((a.N, a.T, a.H, a.W, a.Cp), float("nan"), dtype=BF16, device=dev))
    n, cp = built.first.N, built.first.Cp
    if built.pool is not None:
        pb.bufs[built.pool[0]].external = True
        held["pool"] = (built.pool[0], torch.full((n, built.pool[1], cp), float("nan"), dtype=torch.float32, device=dev))
    if built.gate_buf is not None:
        pb.bufs[built.gate_buf].external = True
        held["gate"] = (built.gate_buf, torch.full((n, cp), float("nan"), dtype=torch.float32, device=dev))
    plan = pb.finish(built.first, built.last)
    plan.arena.fill_(0xFF)
    for buf, t in list(built.binds) + list(held.values()):
        plan.ptrs[buf] = t.data_ptr()
    for op in plan.ops:
        op(plan.ptrs, _lib.current_stream())
    torch.cuda.synchronize()
    return {k: v[1].cpu() for k, v in held.items()}


# ------------------------------------------------------------------------------------------------- reference
def _fold(q):
    """(scale, bias) as the launch reads them: ``plan.fold_norm``'s fp32 values (returned in fp32)."""
    from protoasnet_amd.plan import fold_norm

    c = q["gamma"].numel()
    return fold_norm(_bn(q), None, c, c, torch.device("cpu"))


def _v(t):
    return t.to(F64).view(1, -1, 1, 1, 1)


def from_cl(y, c):
    """[N][T][H][W][Cp] as launched -> (N,C,T,H,W) fp64."""
    return y.detach().cpu().to(F64)[..., :c].permute(0, 4, 1, 2, 3)


def stage(terms, bias, res, kterms):
    """relu(sum_i scale_i * conv(x_i, w_i) + bias + res) in fp64 with the ladder's bound.  ``terms``: [(x fp64 values of bf16 numbers, flip or
    None, w fp32, scale fp32, stride)]; every term has its own fp32 accumulator or shares one: 2 K 2^-24 A with K = ``kterms`` covers both."""
    u, A, fl, risk = _v(bias), _v(bias).abs(), 0.0, 0.0
    for x, flip, w, scale, s in terms:
        w = tk.rnd(w, BF16)
        u = u + _v(scale) * conv64(x, w, s, P0)
        A = A + _v(scale).abs() * conv64(x.abs(), w.abs(), s, P0)
        if flip is not None:
            fl = fl + _v(scale).abs() * conv64(flip, w.abs(), s, P0)
            risk = max(risk, float((flip > 0).double().mean()))
    if res is not None:
        u, A = u + res, A + res.abs()
    ref = torch.relu(u)
    bound = tk.BF16_STORE * ref.abs() + LIPSCHITZ["relu"] * (2 * kterms * 2.0 ** -24 * A + fl)
    return dict(ref=ref, bound=bound, u=u, A=A, at_risk=risk)


def swished(xs, gate=None, dg=None):
    """(x', flip) of x' = swish(xs * gate): the ladder's transformed operand (conv_kernel_cases.transformed_input), ``dg`` = how far the
    kernel's own fp32 gate may lie from ``gate`` (N,C), or None for a gate tensor the kernel reads as it is."""
    v = xs if gate is None else xs * gate[:, :, None, None, None]
    xt = v * torch.sigmoid(v)
    eps = (8 + 2 * v.abs()) * 2.0 ** -24
    if dg is not None:
        eps = eps + (1 + v.abs()) * (dg / gate)[:, :, None, None, None]
    flip = (tk.rnd(xt * (1 + eps), BF16) - tk.rnd(xt * (1 - eps), BF16)).abs()
    return tk.rnd(xt, BF16), flip


def gate_ref(case, pool):
    """(gate, dg) (N,C) fp64 from the pool partial rows [N][blocks][Cp] as stored: sigmoid(fc2(relu(fc1(mean)))) and the fp32 evaluation's distance."""
    T = tensors(case.id)
    c, cse, P = case.c0, case.cse, case.nthw[1] * case.nthw[2] * case.nthw[3]
    w1, b1, w2, b2 = (T[k].to(F64) for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b"))
    part = pool.detach().cpu().to(F64)[..., :c]
    blocks = part.shape[1]
    mean = part.sum(1) / P
    a1 = part.abs().sum(1) / P @ w1.abs().t() + b1.abs()
    hid = torch.relu(mean @ w1.t() + b1)
    e_h = 2 * (c + blocks + 1) * 2.0 ** -24 * a1
    z = hid @ w2.t() + b2
    a2 = hid @ w2.abs().t() + b2.abs()
    gate = torch.sigmoid(z)
    dg = 0.25 * (e_h @ w2.abs().t() + 2 * (cse + 1) * 2.0 ** -24 * a2) + (2.0 ** -21 + z.abs() * 2.0 ** -24) * gate
    return gate, dg


def _edp_first(case):
    """The block output of an ``edp`` row from the inputs alone: two unstored stages, their flip intervals carried forward (module docstring)."""
    T = tensors(case.id)
    x = tk.rnd(T["x"], BF16)
    (sa, ba), (sd, bd), (sc, bc) = _fold(T["bn_a"]), _fold(T["bn_b"]), _fold(T["bn1"])
    wa = tk.rnd(T["wa"], BF16)
    u_e = _v(sa) * conv64(x, wa, S1, P0) + _v(ba)
    A_e = _v(sa).abs() * conv64(x.abs(), wa.abs(), S1, P0) + _v(ba).abs()
    eps_e = 2 * (case.c0 + 1) * 2.0 ** -24 * A_e
    e = tk.rnd(torch.relu(u_e), BF16)
    flip_e = (tk.rnd(torch.relu(u_e + eps_e), BF16) - tk.rnd(torch.relu(u_e - eps_e), BF16)).abs()
    wd = T["wb"].to(BF16).to(F64)  # plan.stencil_operands: the taps rounded to bf16
    one, c = (1, 1, 1), case.c1
    pre = _v(sd) * conv64(e, wd, S1, one, groups=c) + _v(bd)
    A_d = _v(sd).abs() * conv64(e.abs(), wd.abs(), S1, one, groups=c) + _v(bd).abs()
    d_pre = _v(sd).abs() * conv64(flip_e, wd.abs(), S1, one, groups=c) + 2 * 27 * 2.0 ** -24 * A_d
    sw = pre * torch.sigmoid(pre)
    dd = LIPSCHITZ["swish"] * d_pre + (2.0 ** -21 + pre.abs() * 2.0 ** -24) * sw.abs()
    d = tk.rnd(sw, BF16)
    flip_d = (tk.rnd(sw + dd, BF16) - tk.rnd(sw - dd, BF16)).abs()
    R = stage([(d, flip_d, T["w1"], sc, S1)], bc, x, round_up(case.c1, 8))
    R["at_risk_e"], R["at_risk"] = float((flip_e > 0).double().mean()), float((flip_d > 0).double().mean())
    return R


@functools.lru_cache(maxsize=None)
def first_from_inputs(case_id):
    """The first stage of the rows whose first stage reads nothing an earlier launch stored (``short``, ``pair``, ``pe``, ``edp``), once per row."""
    case = BY_ID[case_id]
    T = tensors(case_id)
    if case.form == "edp":
        return _edp_first(case)
    x = tk.rnd(T["x"], BF16)
    xt, flip = swished(x, T["gate"].to(F64)) if case.gate else (x, None)
    s1, b1 = _fold(T["bn1"])
    if case.form == "short":
        s2, b2 = _fold(T["bn2"])
        return stage([(xt, flip, T["w1"], s1, S1), (tk.rnd(T["x2"], BF16), None, T["w2"], s2, S2)], b1 + b2, None,
                     round_up(case.c0, 8) + round_up(case.cx, 8))
    return stage([(xt, flip, T["w1"], s1, S1)], b1, tk.rnd(T["res"], BF16), round_up(case.c0, 8))


def reference(case, stored):
    """{output name: dict(ref, bound, ..., at_risk)} (N,C,T,H,W) fp64.  ``stored``: what ``launch`` returned (or the CPU test's emulation of it):
    the stages that read a stored tensor start from it (module docstring)."""
    T = tensors(case.id)
    R = {}
    if case.form in SE_FORMS:
        for k in ("ys", "pool"):
            assert bool(torch.isfinite(stored[k].float()).all()), f"{case.id}: the stencil launch left {k} unwritten or not finite"
        gate, dg = gate_ref(case, stored["pool"])
        if case.form == "gate":
            return {"gate": dict(ref=gate, bound=dg + 2.0 ** -24 * gate, at_risk=0.0)}
        xt, flip = swished(from_cl(stored["ys"], case.c0), gate, dg)
        s1, b1 = _fold(T["bn1"])
        R["y1"] = stage([(xt, flip, T["w1"], s1, S1)], b1, tk.rnd(T["res"], BF16) if case.res else None, round_up(case.c0, 8))
    else:
        R["y1"] = first_from_inputs(case.id)
    if case.c2:
        c_mid = case.c0 if case.form == "edp" else case.c1
        y1 = from_cl(stored["y1"], c_mid)
        assert bool(torch.isfinite(y1).all()), f"{case.id}: y1 unwritten or not finite"
        s2, b2 = _fold(T["bn2"])
        R["y2"] = stage([(y1, None, T["w2"], s2, S1)], b2, None, round_up(c_mid, 8))
    return R


# ------------------------------------------------------------------------------------------------- comparison
def _ratio(got, want, bound, label):
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    assert_close(ratio, torch.zeros_like(ratio), 1.0, 0.0, f"{label} max_err={float(err.max()):.3g} worst: err={float(err.flatten()[i]):.3g} "
                 f"bound={float(bound.flatten()[i]):.3g} |ref|={float(want.flatten()[i].abs()):.3g} max|ref|={float(want.abs().max()):.3g} (err / bound)")
    return float(ratio.max())


def check(case, outs, name=None):
    """``outs``: what ``launch`` returned.  Every captured tensor written and finite; every output of the launch under test within the bound on
    the real channels (logged through ``assert_close`` as err / bound against 1) and exactly zero in the padded ones.  Returns the largest ratio."""
    tag = f"{name or case.expect} {case.id}"
    n = case.nthw[0]
    for k, t in outs.items():
        assert bool(torch.isfinite(t.float()).all()), f"{case.id}: {int((~torch.isfinite(t.float())).sum())} elements of {k} unwritten or not finite"
    R = reference(case, outs)
    worst = 0.0
    if case.form == "gate":
        gate = outs["gate"].to(F64)
        assert tuple(gate.shape) == (n, round_up(case.c0, 8)), tuple(gate.shape)
        worst = _ratio(gate[:, :case.c0], R["gate"]["ref"], R["gate"]["bound"], tag + " gate")
        if gate.shape[1] > case.c0:
            assert float(gate[:, case.c0:].abs().max()) == 0.0, f"{case.id}: the gate's padded channels must be exact zeros"
        return worst
    for k, c in outputs(case):
        out = outs[k].to(F64)
        assert tuple(out.shape) == (n,) + out_thw(case) + (round_up(c, 8),), (k, tuple(out.shape))
        worst = max(worst, _ratio(from_cl(out, c), R[k]["ref"], R[k]["bound"], f"{tag} {k}"))
        if out.shape[-1] > c:
            assert float(out[..., c:].abs().max()) == 0.0, f"{case.id}: padded channels of {k} must be exact zeros"
    return worst
