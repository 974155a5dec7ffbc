"""The kernels that read the raw clip (``pasn_first_conv_fwd`` / ``_gray_fwd``, ``pasn_first_conv_mfma_fwd``, ``pasn_x3d_stem_fwd`` /
``_gray_fwd``, ``pasn_x3d_stem_mfma_fwd``) case by case, pure torch on the CPU: one table of small first layers, each pinned to the kernel
instance it runs, with inputs, an fp64 reference and a per-element error bound built from the reference alone.  The third ladder, next to
tests/conv_kernel_cases.py and tests/dw_kernel_cases.py, whose helpers it uses.

Shared by tests/test_gpu_stem_cases.py, which runs the HIP kernels on these inputs, and tests/test_cpu_stem_kernel_cases.py, which checks
without a GPU that every row reaches the instance it names, that the table claims every first-layer instance of the default plans and every
name ``PlanBuilder.first_conv`` / ``x3d_stem`` can print over a sweep of dtypes, windows and switches, that the reference agrees with
conv3d + eval-mode BatchNorm3d and that the bound tells a correct kernel from a subtly wrong one.

**Reference.**  fp64 on the operands exactly as each launch reads them.  The weights come from the plan's own packers
(``plan.pack_first_valu``, ``pack_first_mfma``, ``pack_stem_mfma``, ``pack_dw_taps``; a grey clip's taps summed over the three input
channels in fp32 first, as ``PlanBuilder.first_conv`` / ``x3d_stem`` sum them), the norm from ``plan.fold_norm``.  Every loaded value goes
through x' = fp32(x * a + b), ONE fused rounding ((a, b) = ``pb.in_affine`` on a grey clip, (1, 0) on a three-channel one); zero padding,
spatial and temporal, pads the NORMALISED tensor.  Then the family's **operand model**:

    family                        x as the taps see it   weights                                  between the two convs              read at (protoasnet_amd/csrc)
    first_conv_kernel<TIN,TOUT,COP>   x'                 fp32 taps                                --                                 conv.hip:50 (fmaf(x, in_a, in_b)), :55-58, :68
    first_conv_mfma_kernel<TIN,NT,KS> rnd_bf16(x')       rnd_bf16 of pack_first_mfma              --                                 first_conv_mfma.hip:92, :100 (store4 to the bf16 patch), :137; plan.py first_conv (.to(bfloat16))
    x3d_stem_kernel<TIN,T,24[,grey]>  x'                 fp32 w_xy, fp32 w_t                      e = rnd_T(conv_xy), zero frames    stem.hip:73, :90, :102 ((T)acc into the ring), :118, :128
                                                                                                  outside the clip                   (frames >= T: acc stays 0, :66)
    x3d_stem_mfma_kernel<TIN,CIN>     rnd_bf16(x')       rnd_bf16(fp32 product w_t * w_xy)        none: one linear map, K = 5*Cin*9  stem_mfma.hip:110-111, :156; plan.py pack_stem_mfma

    pre = scale * sum + bias,   ref = act(pre)                       (act: none or relu; the stems always relu)

The pair rows (``first_conv_kernel<u8,.,24>+dwconv_t_kernel<.,5>``: a three-channel uint8 clip off the matrix-core arm, for which
``x3d_stem_kernel`` has no instance) run the two unfused launches end to end against the x3d_stem_kernel model: the first launch stores
e in T, the second reads it with fp32 taps (dwtemporal.hip:55-56) -- the same values, which is what stem.hip's header promises.

**Bound**, per output element, from the reference's own quantities (nothing the kernel returns enters it):

    bound = STORE * |ref|  +  2 * K * 2^-24 * A  +  flip_term

``STORE`` = ``BF16_STORE`` = 2^-8 for bf16 outputs (no margin, as in the other ladders), 2^-23 for fp32 outputs.  K terms, the bias included,
meet in one fp32 accumulator (Cin*kh*kw + 1; the matrix-core stem 5*Cin*9 + 1; the VALU stem's temporal accumulator 5 + 1) and A = |scale| *
conv(|x|, |w|) + |bias| on the operands of the table bounds every partial sum; the factor 2 is the margin of the other ladders; L = 1 (only
none and relu occur).  ``flip_term`` is the dense ladder's device for an operand on the other side of a rounding boundary:

* the load-time normalisation: the kernel's x' is the fused fmaf; the reference rounds the fp64 value once more.  An operand within 2^-23
  of a rounding boundary of its dtype (bf16 on the matrix-core families, fp32 on the VALU ones) may legitimately be the neighbour: flip =
  |rnd(x'(1 + 2^-23)) - rnd(x'(1 - 2^-23))|, charged as |scale| * conv(flip, |w|).  Exactly zero where (a, b) = (1, 0).
* the VALU stem's intermediate, the expand rows' treatment of dw_kernel_cases.py: the kernel's conv_xy sum is within eps_e = 2 * K_xy * 2^-24
  * A_e (+ conv(flip, |w_xy|) on a normalising row) of the reference's, K_xy = Cin*9 + 1, so its e lies between rnd_T(e - eps_e) and
  rnd_T(e + eps_e); flip_e = the distance of the two and the term is |scale| * sum_k |w_t[k]| * flip_e[t - 2 + k].  ``reference`` reports
  the share of intermediate elements with flip_e > 0; the CPU test asserts it below 5 % on every bf16 stem row.  For T = f32 every element is
  "at risk" and the same expression is the plain first-order bound: those rows are exempt.

Padded output channels must read back as exact zeros, and nothing of the output may be left unwritten (the GPU test's output is full of NaN).

**Observed** on an MI355X (profiles/stem_ladder_parity_observed.tsv), largest err / bound per family, bf16 | fp32 outputs:
first_conv_kernel 0.994 | 0.222; first_conv_mfma_kernel 0.995; x3d_stem_kernel 0.991 | 0.064 (the pair rows 0.946 | 0.025);
x3d_stem_mfma_kernel 0.991.  The bf16 rows' 0.90 .. 0.995 is the STORE term, which has no margin; the fp32 rows' largest ratios are the 3x3
grey windows, whose bound (ten terms) is little more than the fp32 store.  No row needed a rounding point beyond the table above.

**Table.**  ``expect`` is the instance name as ``pb.meta[-1]["kernel"]`` prints it (a pair row: the two names joined with ``+``); ``env``
holds the routing switches (the row is built AND launched under them).  ``x``: the clip's dtype (``u8`` rows draw integers 0 .. 255, and so
does every row that normalises); ``norm``: a grey row whose ``in_affine`` is (1 / (255 * 0.171), -0.099 / 0.171) -- the non-zero b separates
"pad the normalised tensor with zeros" from "normalise a padded zero"; the other grey rows keep (1, 0).  N = 2 on every row.  Shapes:

* ``first_conv_kernel`` (a thread per output position, 256 per block): odd planes 13 x 15 and 17 x 19 (fewer and more than 256 positions, a
  ragged last block, right / bottom windows cut differently from left / top), T = 1 and 2, windows 7x7 p3, 3x3 p1, 5x5 p2, Cout 6, 12, 20,
  30, 45, 64 (the real channels end inside an 8-group; every COP).  bf16 rows reach it through ``PASN_NO_FC_MFMA=1``, a width no multiple
  of 4, or a window the matrix-core kernel has no instance for (the (1,5,5) rows at W = 16: before the probe and the launcher read one list
  of instances these built the matrix-core arm and raised at launch).
* ``first_conv_mfma_kernel`` (block = 4 output rows x 64 columns, two 32-column tiles per wave): (2,18,24): Ho = 9, a last row tile of one
  row, an empty second column tile; (1,10,72): Wo = 36, a ragged second tile; (1,8,132): Wo = 66, two column blocks, the second two columns
  wide; (3,7,4): Wo = 2, a patch mostly outside the image.  Cout 20, 24, 33, 45, 64; windows 7x7 p3 (slot 1) and 3x3 p1 (slot 3).
* ``x3d_stem_kernel`` (a thread marches along T with a five-frame ring): (7,9,11); (1,6,6): every temporal neighbour outside the clip;
  (2,5,7): T shorter than the window; (3,30,36): 540 positions per launch, more than one block and a ragged one.
* ``x3d_stem_mfma_kernel`` (block = 4 rows x 56 owned columns of a 64-wide tile, ring of 6 frame slots): (7,18,24); (1,16,16); (3,10,132):
  Wo = 66 = 56 + 10; (2,8,116): Wo = 58 = 56 + 2; (5,6,228): Wo = 114, three column tiles; (6,9,20) and (13,9,20): T at and beyond two
  turns of the ring, odd Ho.

Instances without a row: none of the four .hip files holds an instance that no ``PlanBuilder`` call can reach -- ``first_conv_kernel`` has
every (TIN, TOUT, COP) of {f32, bf16, u8} x {f32, bf16} x {8, 16, 24, 32, 48, 64} (conv.hip:814-819, :87-92; the table runs all 36, grey
and three-channel clips alternating: ``[grey]`` is a run-time branch on ``d.Cin``, not an instance), ``first_conv_mfma_kernel`` 3 x {1, 2} x
{11, 5, 4, 2} (first_conv_mfma.hip ``PASN_FCM_INSTANCES``), ``x3d_stem_kernel`` the ten of ``stem_dispatch`` (stem.hip:163-168) and
``x3d_stem_mfma_kernel`` 3 x {1, 3} (stem_mfma.hip:216-231).  A Cout_p of 40 or 56 has no ``first_conv_kernel`` instance and no row: no trunk
of this package has such a first layer, and the launch says so (conv.hip:94)."""
import collections
import functools

import torch
import torch.nn as nn

import train_kernel_cases as tk
from conftest import assert_close
from conv_kernel_cases import ACT, DT, F64, conv64, round_up, switches  # noqa: F401  (switches: used by the tests)

XDT = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}
AFFINE = (1.0 / (255.0 * 0.171), -0.099 / 0.171)   # the grey pipeline's normalisation: x' = (x / 255 - mean) / std
S2 = (1, 2, 2)

Case = collections.namedtuple("Case", "id kind cin cout k p nthw act x dtype norm env expect")

_NOFC, _NOSM = {"PASN_NO_FC_MFMA": "1"}, {"PASN_NO_STEM_MFMA": "1"}
K7, K3, K5 = dict(k=(7, 7), p=(3, 3)), dict(k=(3, 3), p=(1, 1)), dict(k=(5, 5), p=(2, 2))


def _fc(id, cin, cout, thw, expect, x="f32", dtype="f32", act="relu", norm=False, k=(7, 7), p=(3, 3), env=None):
    assert not norm or cin == 1
    return Case(id, "first", cin, cout, k, p, (2,) + thw, act, x, dtype, norm, dict(env or {}), expect + ("[grey]" if cin == 1 else ""))


def _st(id, cin, cout, thw, expect, x="f32", dtype="f32", norm=False, env=None):
    assert not norm or cin == 1
    return Case(id, "stem", cin, cout, (3, 3), (1, 1), (2,) + thw, "relu", x, dtype, norm, dict(env or {}), expect)


A, B, C_, D = (1, 13, 15), (2, 13, 15), (1, 17, 19), (2, 17, 19)           # first_conv_kernel planes
MA, MB, MC, MD = (2, 18, 24), (1, 10, 72), (1, 8, 132), (3, 7, 4)          # first_conv_mfma_kernel planes
SA, SB, SC, SD = (7, 9, 11), (1, 6, 6), (2, 5, 7), (3, 30, 36)             # x3d_stem_kernel planes

CASES = [
    # ---- first_conv_kernel<TIN,TOUT,COP>: every (TIN, TOUT, COP); grey and three-channel clips, the three windows, T = 1 / 2 ---------------
    _fc("fc_f32_f32_8", 3, 6, A, "first_conv_kernel<f32,f32,8>", **K3),
    _fc("fc_f32_f32_16_grey", 1, 12, D, "first_conv_kernel<f32,f32,16>", act="none", **K5),
    _fc("fc_f32_f32_24", 3, 20, B, "first_conv_kernel<f32,f32,24>", act="none", **K3),
    _fc("fc_f32_f32_24_grey", 1, 20, C_, "first_conv_kernel<f32,f32,24>", norm=True),
    _fc("fc_f32_f32_32_grey", 1, 30, A, "first_conv_kernel<f32,f32,32>", norm=True, **K3),
    _fc("fc_f32_f32_48", 3, 45, D, "first_conv_kernel<f32,f32,48>"),                                   # R(2+1)D stem, fp32
    _fc("fc_f32_f32_48_grey", 1, 45, B, "first_conv_kernel<f32,f32,48>", **K5),
    _fc("fc_f32_f32_64", 3, 64, C_, "first_conv_kernel<f32,f32,64>"),                                  # ResNet-18 conv1, fp32
    _fc("fc_f32_bf16_8_grey", 1, 6, B, "first_conv_kernel<f32,bf16,8>", dtype="bf16", norm=True),
    _fc("fc_f32_bf16_16", 3, 12, C_, "first_conv_kernel<f32,bf16,16>", dtype="bf16", **K3),
    _fc("fc_f32_bf16_24", 3, 20, D, "first_conv_kernel<f32,bf16,24>", dtype="bf16", **K5),
    _fc("fc_f32_bf16_24_grey", 1, 20, A, "first_conv_kernel<f32,bf16,24>", dtype="bf16", act="none", **K3),
    _fc("fc_f32_bf16_32", 3, 30, B, "first_conv_kernel<f32,bf16,32>", dtype="bf16", act="none"),
    _fc("fc_f32_bf16_48", 3, 45, (2, 20, 24), "first_conv_kernel<f32,bf16,48>", dtype="bf16", env=_NOFC),
    _fc("fc_f32_bf16_48_grey", 1, 45, C_, "first_conv_kernel<f32,bf16,48>", dtype="bf16", norm=True),
    _fc("fc_f32_bf16_64_grey", 1, 64, D, "first_conv_kernel<f32,bf16,64>", dtype="bf16", **K3),
    _fc("fc_bf16_f32_8", 3, 6, C_, "first_conv_kernel<bf16,f32,8>", x="bf16", **K5),
    _fc("fc_bf16_f32_16_grey", 1, 12, A, "first_conv_kernel<bf16,f32,16>", x="bf16", norm=True),
    _fc("fc_bf16_f32_24", 3, 20, D, "first_conv_kernel<bf16,f32,24>", x="bf16"),
    _fc("fc_bf16_f32_24_grey", 1, 20, B, "first_conv_kernel<bf16,f32,24>", x="bf16", **K3),
    _fc("fc_bf16_f32_32", 3, 30, C_, "first_conv_kernel<bf16,f32,32>", x="bf16", act="none", **K3),
    _fc("fc_bf16_f32_48", 3, 45, A, "first_conv_kernel<bf16,f32,48>", x="bf16", **K3),
    _fc("fc_bf16_f32_48_grey", 1, 45, D, "first_conv_kernel<bf16,f32,48>", x="bf16", norm=True, **K5),
    _fc("fc_bf16_f32_64_grey", 1, 64, B, "first_conv_kernel<bf16,f32,64>", x="bf16"),
    _fc("fc_bf16_bf16_8_grey", 1, 6, D, "first_conv_kernel<bf16,bf16,8>", x="bf16", dtype="bf16", **K3),
    _fc("fc_bf16_bf16_16", 3, 12, B, "first_conv_kernel<bf16,bf16,16>", x="bf16", dtype="bf16"),
    _fc("fc_bf16_bf16_24", 3, 20, (1, 14, 16), "first_conv_kernel<bf16,bf16,24>", x="bf16", dtype="bf16", **K5),        # (1,5,5), W % 4 == 0, no switch
    _fc("fc_bf16_bf16_24_grey", 1, 20, (2, 14, 16), "first_conv_kernel<bf16,bf16,24>", x="bf16", dtype="bf16", norm=True, **K5),  # ... grey
    _fc("fc_bf16_bf16_32_grey", 1, 30, C_, "first_conv_kernel<bf16,bf16,32>", x="bf16", dtype="bf16", norm=True),
    _fc("fc_bf16_bf16_48", 3, 45, C_, "first_conv_kernel<bf16,bf16,48>", x="bf16", dtype="bf16"),                     # R(2+1)D stem at an odd width
    _fc("fc_bf16_bf16_48_grey", 1, 45, (1, 14, 16), "first_conv_kernel<bf16,bf16,48>", x="bf16", dtype="bf16", act="none", env=_NOFC, **K3),
    _fc("fc_bf16_bf16_64", 3, 64, A, "first_conv_kernel<bf16,bf16,64>", x="bf16", dtype="bf16", **K3),
    _fc("fc_u8_f32_8_grey", 1, 6, C_, "first_conv_kernel<u8,f32,8>", x="u8", norm=True, **K3),
    _fc("fc_u8_f32_16", 3, 12, A, "first_conv_kernel<u8,f32,16>", x="u8"),
    _fc("fc_u8_f32_24", 3, 20, B, "first_conv_kernel<u8,f32,24>", x="u8", **K5),
    _fc("fc_u8_f32_24_grey", 1, 20, D, "first_conv_kernel<u8,f32,24>", x="u8", norm=True, **K3),
    _fc("fc_u8_f32_32", 3, 30, D, "first_conv_kernel<u8,f32,32>", x="u8", **K3),
    _fc("fc_u8_f32_48", 3, 45, C_, "first_conv_kernel<u8,f32,48>", x="u8", act="none", **K3),
    _fc("fc_u8_f32_48_grey", 1, 45, A, "first_conv_kernel<u8,f32,48>", x="u8", norm=True),
    _fc("fc_u8_f32_64_grey", 1, 64, B, "first_conv_kernel<u8,f32,64>", x="u8", **K5),                                 # (1, 0): raw grey levels
    _fc("fc_u8_bf16_8", 3, 6, D, "first_conv_kernel<u8,bf16,8>", x="u8", dtype="bf16"),
    _fc("fc_u8_bf16_16_grey", 1, 12, B, "first_conv_kernel<u8,bf16,16>", x="u8", dtype="bf16", norm=True, **K3),
    _fc("fc_u8_bf16_24", 3, 20, C_, "first_conv_kernel<u8,bf16,24>", x="u8", dtype="bf16", **K3),
    _fc("fc_u8_bf16_24_grey", 1, 20, (1, 14, 16), "first_conv_kernel<u8,bf16,24>", x="u8", dtype="bf16", norm=True, **K5),   # (1,5,5), W % 4 == 0
    _fc("fc_u8_bf16_32_grey", 1, 30, D, "first_conv_kernel<u8,bf16,32>", x="u8", dtype="bf16", act="none"),
    _fc("fc_u8_bf16_48", 3, 45, (2, 14, 16), "first_conv_kernel<u8,bf16,48>", x="u8", dtype="bf16", **K5),             # (1,5,5), W % 4 == 0, NT = 2
    _fc("fc_u8_bf16_48_grey", 1, 45, B, "first_conv_kernel<u8,bf16,48>", x="u8", dtype="bf16", norm=True),
    _fc("fc_u8_bf16_64", 3, 64, (1, 18, 24), "first_conv_kernel<u8,bf16,64>", x="u8", dtype="bf16", env=_NOFC),
    # ---- first_conv_mfma_kernel<TIN,NT,KS> (bf16 out, W % 4 == 0): every (TIN, NT, KS); KS 11 / 5 three channels, 4 / 2 grey ---------------
    _fc("fcm_f32_2_11", 3, 45, MA, "first_conv_mfma_kernel<f32,2,11>", dtype="bf16"),                                 # R(2+1)D stem
    _fc("fcm_f32_1_11", 3, 24, MC, "first_conv_mfma_kernel<f32,1,11>", dtype="bf16", act="none"),
    _fc("fcm_f32_2_5", 3, 33, MB, "first_conv_mfma_kernel<f32,2,5>", dtype="bf16", **K3),
    _fc("fcm_f32_1_5", 3, 20, MD, "first_conv_mfma_kernel<f32,1,5>", dtype="bf16", act="none", **K3),
    _fc("fcm_f32_2_4", 1, 64, MB, "first_conv_mfma_kernel<f32,2,4>", dtype="bf16", norm=True),
    _fc("fcm_f32_1_4", 1, 20, MD, "first_conv_mfma_kernel<f32,1,4>", dtype="bf16"),
    _fc("fcm_f32_2_2", 1, 45, MC, "first_conv_mfma_kernel<f32,2,2>", dtype="bf16", norm=True, **K3),
    _fc("fcm_f32_1_2", 1, 24, MA, "first_conv_mfma_kernel<f32,1,2>", dtype="bf16", act="none", **K3),
    _fc("fcm_bf16_2_11", 3, 64, MC, "first_conv_mfma_kernel<bf16,2,11>", x="bf16", dtype="bf16"),                     # ResNet-18 conv1
    _fc("fcm_bf16_1_11", 3, 20, MB, "first_conv_mfma_kernel<bf16,1,11>", x="bf16", dtype="bf16"),
    _fc("fcm_bf16_2_5", 3, 45, MD, "first_conv_mfma_kernel<bf16,2,5>", x="bf16", dtype="bf16", act="none", **K3),
    _fc("fcm_bf16_1_5", 3, 24, MA, "first_conv_mfma_kernel<bf16,1,5>", x="bf16", dtype="bf16", act="none", **K3),     # X3D conv_xy, the training tape's
    _fc("fcm_bf16_2_4", 1, 33, MA, "first_conv_mfma_kernel<bf16,2,4>", x="bf16", dtype="bf16"),
    _fc("fcm_bf16_1_4", 1, 24, MC, "first_conv_mfma_kernel<bf16,1,4>", x="bf16", dtype="bf16", norm=True),
    _fc("fcm_bf16_2_2", 1, 64, MD, "first_conv_mfma_kernel<bf16,2,2>", x="bf16", dtype="bf16", norm=True, **K3),
    _fc("fcm_bf16_1_2", 1, 20, MB, "first_conv_mfma_kernel<bf16,1,2>", x="bf16", dtype="bf16", **K3),
    _fc("fcm_u8_2_11", 3, 33, MD, "first_conv_mfma_kernel<u8,2,11>", x="u8", dtype="bf16"),
    _fc("fcm_u8_1_11", 3, 24, MA, "first_conv_mfma_kernel<u8,1,11>", x="u8", dtype="bf16"),
    _fc("fcm_u8_2_5", 3, 64, MC, "first_conv_mfma_kernel<u8,2,5>", x="u8", dtype="bf16", **K3),
    _fc("fcm_u8_1_5", 3, 20, MB, "first_conv_mfma_kernel<u8,1,5>", x="u8", dtype="bf16", act="none", **K3),
    _fc("fcm_u8_2_4", 1, 45, MA, "first_conv_mfma_kernel<u8,2,4>", x="u8", dtype="bf16", norm=True),
    _fc("fcm_u8_1_4", 1, 24, MB, "first_conv_mfma_kernel<u8,1,4>", x="u8", dtype="bf16", norm=True, act="none"),
    _fc("fcm_u8_2_2", 1, 33, MA, "first_conv_mfma_kernel<u8,2,2>", x="u8", dtype="bf16", **K3),                       # (1, 0): raw grey levels
    _fc("fcm_u8_1_2", 1, 20, MC, "first_conv_mfma_kernel<u8,1,2>", x="u8", dtype="bf16", norm=True, **K3),
    # ---- x3d_stem_kernel<TIN,T,24[,grey]>: the ten of stem_dispatch; bf16 rows by a width no multiple of 4 or PASN_NO_STEM_MFMA=1 ---------
    _st("st_f32_f32", 3, 24, SA, "x3d_stem_kernel<f32,f32,24>"),
    _st("st_f32_f32_grey", 1, 20, SD, "x3d_stem_kernel<f32,f32,24,grey>", norm=True),
    _st("st_f32_bf16", 3, 20, SD, "x3d_stem_kernel<f32,bf16,24>", dtype="bf16", env=_NOSM),
    _st("st_f32_bf16_t1", 3, 24, SB, "x3d_stem_kernel<f32,bf16,24>", dtype="bf16"),
    _st("st_f32_bf16_grey", 1, 24, SC, "x3d_stem_kernel<f32,bf16,24,grey>", dtype="bf16"),
    _st("st_bf16_f32", 3, 20, SC, "x3d_stem_kernel<bf16,f32,24>", x="bf16"),
    _st("st_bf16_f32_grey", 1, 24, SB, "x3d_stem_kernel<bf16,f32,24,grey>", x="bf16", norm=True),
    _st("st_bf16_bf16", 3, 24, SA, "x3d_stem_kernel<bf16,bf16,24>", x="bf16", dtype="bf16"),
    _st("st_bf16_bf16_t2", 3, 20, SC, "x3d_stem_kernel<bf16,bf16,24>", x="bf16", dtype="bf16"),
    _st("st_bf16_bf16_grey", 1, 20, SD, "x3d_stem_kernel<bf16,bf16,24,grey>", x="bf16", dtype="bf16", norm=True, env=_NOSM),
    _st("st_u8_f32_grey", 1, 24, SA, "x3d_stem_kernel<u8,f32,24,grey>", x="u8", norm=True),
    _st("st_u8_f32_grey_raw", 1, 20, SC, "x3d_stem_kernel<u8,f32,24,grey>", x="u8"),
    _st("st_u8_bf16_grey", 1, 20, SA, "x3d_stem_kernel<u8,bf16,24,grey>", x="u8", dtype="bf16", norm=True),
    _st("st_u8_bf16_grey_t1", 1, 24, SB, "x3d_stem_kernel<u8,bf16,24,grey>", x="u8", dtype="bf16", norm=True),
    # ---- a three-channel uint8 clip off the matrix-core arm: x3d_stem_kernel has no instance, the plan takes the two unfused launches ----
    _st("pair_u8_f32", 3, 24, SA, "first_conv_kernel<u8,f32,24>+dwconv_t_kernel<f32,5>", x="u8"),
    _st("pair_u8_bf16", 3, 20, SC, "first_conv_kernel<u8,bf16,24>+dwconv_t_kernel<bf16,5>", x="u8", dtype="bf16"),
    # ---- x3d_stem_mfma_kernel<TIN,CIN> (bf16 out, W % 4 == 0): the six of the launcher ---------------------------------------------------
    _st("sm_f32_3", 3, 24, (7, 18, 24), "x3d_stem_mfma_kernel<f32,3>", dtype="bf16"),
    _st("sm_f32_3_ring2", 3, 20, (13, 9, 20), "x3d_stem_mfma_kernel<f32,3>", dtype="bf16"),
    _st("sm_f32_1", 1, 20, (3, 10, 132), "x3d_stem_mfma_kernel<f32,1>", dtype="bf16", norm=True),
    _st("sm_bf16_3", 3, 20, (2, 8, 116), "x3d_stem_mfma_kernel<bf16,3>", x="bf16", dtype="bf16"),                     # the benchmark's instance
    _st("sm_bf16_3_t1", 3, 24, (1, 16, 16), "x3d_stem_mfma_kernel<bf16,3>", x="bf16", dtype="bf16"),
    _st("sm_bf16_3_ring", 3, 24, (6, 9, 20), "x3d_stem_mfma_kernel<bf16,3>", x="bf16", dtype="bf16"),
    _st("sm_bf16_1", 1, 24, (5, 6, 228), "x3d_stem_mfma_kernel<bf16,1>", x="bf16", dtype="bf16"),
    _st("sm_u8_3", 3, 24, (3, 10, 132), "x3d_stem_mfma_kernel<u8,3>", x="u8", dtype="bf16"),
    _st("sm_u8_3_wide", 3, 20, (5, 6, 228), "x3d_stem_mfma_kernel<u8,3>", x="u8", dtype="bf16"),
    _st("sm_u8_1", 1, 24, (7, 18, 24), "x3d_stem_mfma_kernel<u8,1>", x="u8", dtype="bf16", norm=True),                # the echo pipeline's instance
    _st("sm_u8_1_ring2", 1, 20, (13, 9, 20), "x3d_stem_mfma_kernel<u8,1>", x="u8", dtype="bf16", norm=True),
    _st("sm_u8_1_t1", 1, 20, (1, 16, 16), "x3d_stem_mfma_kernel<u8,1>", x="u8", dtype="bf16", norm=True),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def family(case):
    """The kernel whose operand model the row is held to (a pair row: ``x3d_stem_kernel``, whose values the two launches must give)."""
    return "x3d_stem_kernel" if "+" in case.expect else case.expect.split("<")[0]


def is_pair(case):
    return "+" in case.expect


def out_extent(case):
    n, t, h, w = case.nthw
    return (t, (h + 2 * case.p[0] - case.k[0]) // 2 + 1, (w + 2 * case.p[1] - case.k[1]) // 2 + 1)


def affine(case):
    """(a, b) as the launch gets them: fp32 values of ``pb.in_affine``."""
    a, b = AFFINE if case.norm else (1.0, 0.0)
    return float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(b, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------- inputs
def _norm_params(c, g):
    return dict(gamma=torch.rand(c, generator=g) + 0.5, beta=torch.randn(c, generator=g) * 0.3, mean=torch.randn(c, generator=g) * 0.3,
                var=torch.rand(c, generator=g) + 0.5)


@functools.lru_cache(maxsize=None)
def tensors(case_id):
    """Inputs of a row, drawn once: the clip x (N,Cin,T,H,W) in its own dtype (integers 0 .. 255 on uint8 and on normalising rows, randn
    otherwise), the fp32 conv weights w (Cout,3,1,kh,kw) (three input channels always: a grey row's plan sums them), a stem's temporal
    taps wt (Cout,1,5,1,1), and the norm."""
    case = BY_ID[case_id]
    n, t, h, w = case.nthw
    g = torch.Generator().manual_seed(5000 + CASES.index(case))
    if case.x == "u8" or case.norm:
        x = torch.randint(0, 256, (n, case.cin, t, h, w), generator=g).to(XDT[case.x])
    else:
        x = torch.randn(n, case.cin, t, h, w, generator=g).to(XDT[case.x])
    T = dict(x=x, w=torch.randn(case.cout, 3, 1, *case.k, generator=g) * (1.5 / (3 * case.k[0] * case.k[1]) ** 0.5), bn=_norm_params(case.cout, g))
    if case.kind == "stem":
        T["wt"] = torch.randn(case.cout, 1, 5, 1, 1, generator=g) * (1.5 / 5 ** 0.5)
    return T


def _bn(c, q):
    bn = nn.BatchNorm3d(c)
    with torch.no_grad():
        bn.weight.copy_(q["gamma"]), bn.bias.copy_(q["beta"]), bn.running_mean.copy_(q["mean"]), bn.running_var.copy_(q["var"])
    return bn.eval()


def modules(case):
    """The row as torch modules (fp32 parameters): dict(conv, bn[, conv_t]), what ``PlanBuilder.first_conv`` / ``x3d_stem`` take."""
    T = tensors(case.id)
    conv = nn.Conv3d(3, case.cout, (1,) + case.k, S2, (0,) + case.p, bias=False)
    with torch.no_grad():
        conv.weight.copy_(T["w"])
    m = dict(conv=conv, bn=_bn(case.cout, T["bn"]))
    if case.kind == "stem":
        m["conv_t"] = nn.Conv3d(case.cout, case.cout, (5, 1, 1), 1, (2, 0, 0), groups=case.cout, bias=False)
        with torch.no_grad():
            m["conv_t"].weight.copy_(T["wt"])
    return m


# ------------------------------------------------------------------------------------------------- builder
Built = collections.namedtuple("Built", "pb x y name kinds store")


def build(case, device):
    """The row as a plan on ``device`` through ``PlanBuilder.input`` + ``.first_conv`` / ``.x3d_stem`` only: one launch, two on a pair row.
    ``name``: the ``kernel`` of ``pb.meta``, joined with ``+``.  The caller holds the row's switches in force (``switches(case)``) around
    this AND the launch."""
    from protoasnet_amd.plan import PlanBuilder

    m = {k: v.to(device) for k, v in modules(case).items()}
    pb = PlanBuilder(torch.device(device), DT[case.dtype], XDT[case.x])
    if case.norm:
        pb.in_affine = AFFINE
    x = pb.input((case.nthw[0], case.cin) + case.nthw[1:])
    if case.kind == "stem":
        y = pb.x3d_stem(x, m["conv"], m["conv_t"], m["bn"])
    else:
        y = pb.first_conv(x, m["conv"], m["bn"], case.act)
    store = tensors(case.id)["x"].to(device).contiguous()
    return Built(pb, x, y, "+".join(r["kernel"] for r in pb.meta), tuple(r["kind"] for r in pb.meta), store)


def launch(built):
    """Run the plan into an output full of NaN (an element the launch does not write stays NaN).  Returns [N][To][Ho][Wo][Cout_p]."""
    from protoasnet_amd import _lib

    plan = built.pb.finish(built.x, built.y)
    o = plan.out
    y = torch.full((o.N, o.T, o.H, o.W, o.Cp), float("nan"), dtype=plan.dtype, device=built.store.device)
    plan.arena.fill_(0xFF)  # a pair row's intermediate starts as NaN too
    plan.ptrs[plan.in_buf], plan.ptrs[plan.out_buf] = built.store.data_ptr(), y.data_ptr()
    for op in plan.ops:
        op(plan.ptrs, _lib.current_stream())
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------------------------- reference
def mfma_family(case):
    return family(case) in ("first_conv_mfma_kernel", "x3d_stem_mfma_kernel")


def loaded_input(case, signed=False):
    """(x, flip) (N,Cin,T,H,W) fp64: the clip as the taps see it -- x' = fp32(x * a + b), rounded to bf16 on the matrix-core families -- and
    how far a correct kernel's copy may be from it (None where (a, b) = (1, 0): not at all).  ``signed``: a test's mutation, uint8 read as
    int8."""
    raw = tensors(case.id)["x"]
    if signed:
        raw = raw.view(torch.int8)
    a, b = affine(case)
    xp = (raw.to(F64) * a + b).to(torch.float32)
    op = torch.bfloat16 if mfma_family(case) else torch.float32
    if (a, b) == (1.0, 0.0):
        return tk.rnd(xp, op), None
    x64 = xp.to(F64)
    flip = (tk.rnd(x64 * (1 + 2.0 ** -23), op) - tk.rnd(x64 * (1 - 2.0 ** -23), op)).abs()
    return tk.rnd(xp, op), flip


def _summed(case, w):
    """(Cout, Ci, kh, kw) fp32 as the plan hands it to its packers: a grey clip's taps summed over the three input channels."""
    w = w.detach().float()[:, :, 0]
    return w.sum(dim=1, keepdim=True) if case.cin == 1 else w


def _desc(case, m):
    from protoasnet_amd.plan import Act, PlanBuilder

    n, t, h, w = case.nthw
    x = Act(n, t, h, w, case.cin, case.cin, -1, planar=True)
    k, p = (1,) + case.k, (0,) + case.p
    return PlanBuilder._probe_desc(x, PlanBuilder._geom(x, case.cout, k, S2, p), k, S2, p, case.act)


def effective_weights(case):
    """dict of fp64 operands under the row's operand model, unpacked from the plan's own packers: ``w`` (Cout, Cin, kt, kh, kw) -- kt = 5
    on the matrix-core stem, the combined map --, ``wt`` (Cout, 1, 5, 1, 1) on the VALU stem, ``scale`` / ``bias`` (Cout,)."""
    import ctypes

    from protoasnet_amd import _lib, plan

    T, m, cpu = tensors(case.id), modules(case), torch.device("cpu")
    c, cp, cin, (kh, kw) = case.cout, round_up(case.cout, 8), case.cin, case.k
    wsrc = _summed(case, m["conv"].weight)
    scale, bias = plan.fold_norm(m["bn"], None, c, cp, cpu)
    assert float(scale[c:].abs().max() if cp > c else 0) == 0.0 and float(bias[c:].abs().max() if cp > c else 0) == 0.0
    W = dict(scale=scale[:c].to(F64), bias=bias[:c].to(F64))
    fam = family(case)
    if fam == "first_conv_mfma_kernel":
        with switches(case):
            slot = int(_lib.lib().pasn_first_conv_mfma_slot(ctypes.byref(_desc(case, m)), _lib.dtype_code(XDT[case.x]), _lib.dtype_code(DT[case.dtype])))
        assert slot >= 0, f"{case.id}: the matrix-core first conv does not cover the row"
        wq = plan.pack_first_mfma(wsrc, slot, cp, cpu).to(torch.bfloat16)                 # [(ci, r) padded][32 NT][8]
        assert float(wq[:, :, :slot].abs().max() if slot else 0) == 0.0 and float(wq[:, :, slot + kw:].abs().max() if slot + kw < 8 else 0) == 0.0
        W["w"] = wq[:cin * kh, :c, slot:slot + kw].reshape(cin, kh, c, kw).permute(2, 0, 1, 3).unsqueeze(2).to(F64)
    elif fam == "x3d_stem_mfma_kernel":
        wq = plan.pack_stem_mfma(wsrc, m["conv_t"].weight.detach().float().reshape(c, 5), cpu).to(torch.bfloat16)   # [2 ksteps][32][8]
        wr = wq.view(wq.shape[0], 32, 2, 4).permute(0, 2, 1, 3).reshape(2 * wq.shape[0], 32, 4)                      # [(kt, ci, r) padded][32][4]
        assert float(wr[:, :, 0].abs().max()) == 0.0 and float(wr[5 * cin * 3:].abs().max() if wr.shape[0] > 15 * cin else 0) == 0.0
        W["w"] = wr[:5 * cin * 3, :c, 1:4].reshape(5, cin, 3, c, 3).permute(3, 1, 0, 2, 4).to(F64)                   # (co, ci, kt, r, s)
    else:
        wp = plan.pack_first_valu(wsrc, cp, cpu)                                          # [(ci, r, s)][cp]
        assert float(wp[:, c:].abs().max() if cp > c else 0) == 0.0
        W["w"] = wp[:, :c].reshape(cin, kh, kw, c).permute(3, 0, 1, 2).unsqueeze(2).to(F64)
        if fam == "x3d_stem_kernel":
            wt = plan.pack_dw_taps(m["conv_t"].weight, cp, cpu)                           # [5][cp]
            W["wt"] = wt[:, :c].t().reshape(c, 1, 5, 1, 1).to(F64)
    return W


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """ref, bound (N,Cout,To,Ho,Wo) fp64 and the quantities the bound is made of; ``at_risk``: the share of the VALU stem's intermediate
    elements with flip_e > 0."""
    case = BY_ID[case_id]
    dtype, fam = DT[case.dtype], family(case)
    x, flip = loaded_input(case)
    W = effective_weights(case)
    w, sc, bi = W["w"], W["scale"].view(1, -1, 1, 1, 1), W["bias"].view(1, -1, 1, 1, 1)
    R = dict(at_risk=0.0)
    if fam == "x3d_stem_kernel":
        s, p = S2, (0,) + case.p
        e64, A_e = conv64(x, w, s, p), conv64(x.abs(), w.abs(), s, p)
        eps = 2 * (case.cin * 9 + 1) * 2.0 ** -24 * A_e
        if flip is not None:
            eps = eps + conv64(flip, w.abs(), s, p)
        e, flip_e = tk.rnd(e64, dtype), (tk.rnd(e64 + eps, dtype) - tk.rnd(e64 - eps, dtype)).abs()
        R.update(e=e, at_risk=float((flip_e > 0).double().mean()))
        wt, one, pt = W["wt"], (1, 1, 1), (2, 0, 0)
        pre = sc * conv64(e, wt, one, pt, groups=case.cout) + bi
        A = sc.abs() * conv64(e.abs(), wt.abs(), one, pt, groups=case.cout) + bi.abs()
        K, flip_term = 5 + 1, sc.abs() * conv64(flip_e, wt.abs(), one, pt, groups=case.cout)
    else:
        s, p = S2, ((2,) if fam == "x3d_stem_mfma_kernel" else (0,)) + case.p
        pre = sc * conv64(x, w, s, p) + bi
        A = sc.abs() * conv64(x.abs(), w.abs(), s, p) + bi.abs()
        K = case.cin * w.shape[2] * case.k[0] * case.k[1] + 1
        flip_term = sc.abs() * conv64(flip, w.abs(), s, p) if flip is not None else 0.0
    ref = ACT[case.act](pre)
    store = tk.BF16_STORE if dtype == torch.bfloat16 else 2.0 ** -23
    R.update(ref=ref, pre=pre, A=A, K=K, bound=store * ref.abs() + 2 * K * 2.0 ** -24 * A + flip_term)
    return R


# ------------------------------------------------------------------------------------------------- comparison
def check(case, out, name=None):
    """``out``: the launch's whole output [N][To][Ho][Wo][Cout_p].  Its shape; every element written; |out - ref| <= bound on the real
    channels (logged through ``assert_close`` as the ratio err / bound against 1); exact zeros in the padded channels.  Returns the
    largest ratio."""
    R = reference(case.id)
    out = out.detach().cpu().to(F64)
    assert tuple(out.shape) == (case.nthw[0],) + out_extent(case) + (round_up(case.cout, 8),), tuple(out.shape)
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
