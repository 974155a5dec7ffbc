"""Trunk compiler: turns a parameter-holding module tree into a replayable list of fused HIP launches.

``HipTrunk.forward`` (eval mode) = ``Plan.run``: the first call for a given (input shape, dtype) walks
``build_plan`` once, which

* folds every eval-mode norm layer into a per-channel fp32 (scale, bias) epilogue,
* packs conv weights into the MFMA fragment-friendly layout of ``pasn_conv3d_fwd``,
* assigns every intermediate activation an offset inside ONE arena by live-range analysis
  (a buffer's bytes are reused as soon as its last consumer has been recorded), so the working set
  of a trunk stays a few of its largest layers instead of the sum of all of them,
* records one closure per launch with all pointers resolved.

Each operand format the kernels define is packed by ONE module-level function: ``pack_conv_weight`` (dense [rows][taps][kc]),
``fragment_major`` / ``fragment_view`` (its MFMA fragment order, ``frag_steps`` per dtype; the training pass refreshes through the same
view), ``se_operands`` (squeeze-excite fc pair), ``pack_dw_taps`` (depthwise [taps][Cp]), ``stencil_operands`` (matrix-core stencil), ``pack_first_valu`` /
``pack_first_mfma`` / ``pack_stem_mfma`` (the first layer's taps: VALU rows, matrix-core K order, the stem's combined map).
A ``PlanBuilder`` method that may answer "not covered" probes first and allocates after: it asks the library with ``_geom`` (output
extents, no buffer) and ``_probe_desc`` (a descriptor nobody keeps), and only a launch that will be recorded reserves buffers
(``_alloc``) and appends to ``keep`` -- a declined launch leaves no trace in the arena plan.  ``conv_kernel_name`` /
``dwconv_kernel_name`` / ``fused_kernel_name`` / ``x3d_pe_kernel_name`` / ``x3d_edp_kernel_name`` decode the library's variant codes into the
instance names of ``meta``: no name is a formula of the shapes here.

Replaying is then a tight loop of ctypes calls on torch's current stream -- no allocation (bar the
output tensor), no host sync, capturable into a hipGraph.  Packed weights are refreshed automatically
when a parameter changes (``load_state_dict``, optimizer step, ``.to()``).
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import ConvDesc

ALIGN = 256


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _triple(v, lead) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(a) for a in v)
    return v if len(v) == 3 else (lead,) + v


class Act:
    """Symbolic channels-last activation [N][T][H][W][Cp] (or the planar network input)."""

    __slots__ = ("N", "T", "H", "W", "C", "Cp", "buf", "planar")

    def __init__(self, N, T, H, W, C, Cp, buf, planar=False):
        self.N, self.T, self.H, self.W, self.C, self.Cp, self.buf, self.planar = N, T, H, W, C, Cp, buf, planar

    @property
    def positions(self) -> int:
        return self.T * self.H * self.W


class _Buf:
    __slots__ = ("nbytes", "first", "last", "offset", "external")

    def __init__(self, nbytes, first, external=False):
        self.nbytes, self.first, self.last, self.offset, self.external = nbytes, first, first, -1, external


def fold_norm(norm: Optional[nn.Module], conv_bias: Optional[torch.Tensor], cout: int, rows: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm (and/or a conv bias) as fp32 per-channel (scale, bias), zero padded to ``rows``."""
    scale = torch.ones(cout, dtype=torch.float32, device=device)
    bias = torch.zeros(cout, dtype=torch.float32, device=device)
    if conv_bias is not None:
        bias = conv_bias.detach().float().clone()
    if norm is not None:
        inv = (norm.running_var.detach().float() + norm.eps).rsqrt()
        g = norm.weight.detach().float() if norm.weight is not None else torch.ones_like(inv)
        b = norm.bias.detach().float() if norm.bias is not None else torch.zeros_like(inv)
        scale = g * inv
        bias = b + (bias - norm.running_mean.detach().float()) * scale
    s = torch.zeros(rows, dtype=torch.float32, device=device)
    o = torch.zeros(rows, dtype=torch.float32, device=device)
    s[:cout] = scale
    o[:cout] = bias
    return s.contiguous(), o.contiguous()


def pack_conv_weight(w: torch.Tensor, cin_p: int, dtype: torch.dtype) -> Tuple[torch.Tensor, int, int]:
    """(Cout, Cin, [kt,] kh, kw) -> [rows][taps][kc] in ``dtype``; returns (packed, kc, rows)."""
    w = w.detach()
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin = w.shape[0], w.shape[1]
    taps = w.shape[2] * w.shape[3] * w.shape[4]
    kc = round_up(cin_p, frag_steps(dtype)[0])
    rows = round_up(round_up(cout, 8), 128)
    packed = torch.zeros(rows, taps, kc, dtype=torch.float32, device=w.device)
    packed[:cout, :, :cin] = w.float().permute(0, 2, 3, 4, 1).reshape(cout, taps, cin)
    return packed.to(dtype).contiguous(), kc, rows


def stencil_operands(w: torch.Tensor, c: int, cp: int) -> torch.Tensor:
    """Depthwise 3x3x3 weights (C,1,3,3,3) as the matrix-core stencil's block-diagonal A operands (``pasn_x3d_edp_fwd``'s ``w_dw``):
    int16 [ceil(cp / 16)][2][64 lanes][8], entry e = kt * 5 + j (half e >> 3, slot e & 7) = bf16 bits of the lane's one possibly nonzero
    element of A[kt][pair j] -- lane (m = lane & 15, q = lane >> 4) supplies k = 8 q .. 8 q + 7 = tap 2 j + (q >> 1) of the pair, channels
    8 (q & 1) ..: only channel m can be nonzero, and only when m's half matches.  Same values (round-to-nearest-even) as the prologue of
    ``dwconv3d_mfma_kernel`` builds (csrc/dwmfma.hip)."""
    dev = w.device
    w27 = w.detach().float().reshape(c, 27)
    ct = (cp + 15) // 16
    lane = torch.arange(64, device=dev)
    m, q = lane & 15, lane >> 4
    ch = torch.arange(ct, device=dev)[:, None] * 16 + m[None, :]                         # [ct][64]
    tap = 2 * torch.arange(5, device=dev)[None, :] + (q >> 1)[:, None]                   # [64][5]
    live = (tap < 9)[None, :, None, :] & ((m >> 3) == (q & 1))[None, :, None, None] & (ch < c)[:, :, None, None]
    idx = torch.arange(3, device=dev)[None, :, None] * 9 + tap.clamp(max=8)[:, None, :]  # [64][3][5]
    vals = w27[ch.clamp(max=c - 1)[:, :, None, None], idx[None]]                         # [ct][64][3][5]
    bits = vals.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    bits = torch.where(live, bits, torch.zeros_like(bits))
    out = torch.zeros(ct, 64, 16, dtype=torch.int32, device=dev)
    out[:, :, :15] = bits.reshape(ct, 64, 15)
    # [tile][half][lane][8]: one half of a tile = 1 KiB = one LDS-DMA instruction of the kernel
    return out.view(ct, 64, 2, 8).permute(0, 2, 1, 3).to(torch.int16).contiguous()


def frag_steps(dtype: torch.dtype) -> Tuple[int, int]:
    """(K elements per MFMA step, elements per lane and half step) of the fragment-major weight layout."""
    return (16, 8) if dtype == torch.bfloat16 else (8, 4)


def fragment_view(wp: torch.Tensor) -> torch.Tensor:
    """Packed weights [rows][taps][kc] as the strided view [rows / 32][K / kstep][2][32][ch] (K = taps * kc) that IS the fragment-major order."""
    kstep, ch = frag_steps(wp.dtype)
    return wp.view(wp.shape[0] // 32, 32, wp[0].numel() // kstep, 2, ch).permute(0, 2, 3, 1, 4)


def fragment_major(wp: torch.Tensor) -> torch.Tensor:
    """Packed weights stored fragment-major (descriptor ``w_frag = 1``): the kernels that read their weights as MFMA fragments load one
    contiguous 1 KB run per wave and fragment instead of a 32-row gather (the gather saturated the CU's address unit)."""
    return fragment_view(wp).contiguous()


def se_operands(fc1: nn.Module, fc2: nn.Module) -> List[torch.Tensor]:
    """Squeeze-excite operands of every gate-computing launch: fp32 [w1 [cse][c], b1 [cse], w2 [c][cse], b2 [c]]."""
    cse, c = fc1.out_channels, fc1.in_channels
    return [fc1.weight.detach().float().reshape(cse, c).contiguous(), fc1.bias.detach().float().contiguous(),
            fc2.weight.detach().float().reshape(c, cse).contiguous(), fc2.bias.detach().float().contiguous()]


def pack_dw_taps(w: torch.Tensor, cp: int, device, flip: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise weights (C, 1, kt, kh, kw) -> fp32 [taps][cp], zero padded channels.  ``flip``: taps reversed (the stencil of the input
    gradient).  ``out``: a persistent destination of that shape, whose padding is zero already (the training pass refreshes in place)."""
    c, taps = w.shape[0], w[0].numel()
    wp = out if out is not None else torch.zeros(taps, cp, dtype=torch.float32, device=device)
    t = w.detach().float().reshape(c, taps)
    wp[:, :c] = (t.flip(1) if flip else t).t()
    return wp


def pack_first_mfma(w: torch.Tensor, slot: int, cp: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """First-conv weights (C, Ci, kh, kw) in the matrix-core stem's K order: fp32 [nq][bn][8] -- rows (ci, r) padded to an even count,
    ``cp`` padded to 32 channels, 8-wide window slots with tap s in slot ``slot`` + s (``pasn_first_conv_mfma_slot``).  The kernel reads
    the bf16 cast.  ``out`` as in ``pack_dw_taps``."""
    c, ci, kh, kw = w.shape
    rows, nq, bn = ci * kh, 2 * ((ci * kh + 1) // 2), 32 * ((cp + 31) // 32)
    wq = out if out is not None else torch.zeros(nq, bn, 8, dtype=torch.float32, device=device)
    wq[:rows, :c, slot:slot + kw] = w.permute(1, 2, 0, 3).reshape(rows, c, kw)
    return wq


def pack_stem_mfma(wxy: torch.Tensor, wt: torch.Tensor, device) -> torch.Tensor:
    """X3D stem weights in the matrix-core stem's K order: both convs as one map, the fp32 product W'[co][kt][ci][r][s] = wt[co][kt] *
    wxy[co][ci][r][s] (``wxy`` (C, Ci, 3, 3), ``wt`` (C, 5)) as fp32 [2 * ksteps][32][8] -- K rows R = (kt, ci, r) in pairs, 4-wide window
    slots with tap s in slot 1 + s, 32 channels.  The kernel reads the bf16 cast."""
    c, ci = wxy.shape[0], wxy.shape[1]
    rows = 5 * ci * 3
    ksteps = (rows + 3) // 4
    comb = wt[:, :, None, None, None] * wxy[:, None]                         # [co][kt][ci][r][s]
    wr = torch.zeros(4 * ksteps, 32, 4, dtype=torch.float32, device=device)
    wr[:rows, :c, 1:4] = comb.permute(1, 2, 3, 0, 4).reshape(rows, c, 3)
    return wr.view(2 * ksteps, 2, 32, 4).permute(0, 2, 1, 3).reshape(2 * ksteps, 32, 8)


def pack_first_valu(w: torch.Tensor, cp: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """First-conv weights (C, Ci, kh, kw) -> fp32 [(ci, r, s)][cp], zero padded channels (the VALU first-conv and X3D stem kernels).
    ``out`` as in ``pack_dw_taps``."""
    c, ci, kh, kw = w.shape
    wp = out if out is not None else torch.zeros(ci * kh * kw, cp, dtype=torch.float32, device=device)
    wp[:, :c] = w.permute(1, 2, 3, 0).reshape(ci * kh * kw, c)
    return wp


def same_extent(a: Act, b: Act) -> bool:
    """A residual covers exactly the positions and padded channels of the tensor it is added to."""
    return (a.N, a.T, a.H, a.W, a.Cp) == (b.N, b.T, b.H, b.W, b.Cp)


# ---- kernel instance names: the codes of pasn_conv3d_variant / pasn_dwconv3d_variant, tested in the order conv.hip assigns them ---------
CONV_TCONV_WS, CONV_PW_WS, CONV_PW_TINY, CONV_PW_PERSIST, CONV_PW_XTILE, CONV_IGEMM, CONV_GEMM = 9000, 7000, 2002, 1000, 2500, 6000, 2000
DW_TEMPORAL, DW_TZ, DW_MFMA, DW_MARCH = 70000, 60000, 50000, 3000


def conv_kernel_name(v: int, tname: str, gate: bool, in_swish: bool, res: bool) -> str:
    tf = lambda b: "true" if b else "false"
    if v >= CONV_TCONV_WS:
        return f"tconv_ws_kernel<{v - CONV_TCONV_WS},{tf(res)}>"
    if v >= CONV_PW_WS:
        return f"pwconv_ws_kernel<{(v - CONV_PW_WS) // 10},{v % 10},{tf(gate or in_swish)},{tf(res)}>"
    if v == CONV_PW_TINY:
        return f"pwconv_tiny_kernel<{tname}>"
    if CONV_PW_PERSIST <= v < CONV_GEMM:
        return f"pwconv_persist_kernel<{tname},{(v - CONV_PW_PERSIST) // 10},{v % 10},{tf(res)}>"
    if CONV_PW_XTILE <= v < CONV_IGEMM:
        return f"pwconv_xtile_kernel<{tname},{(v - CONV_PW_XTILE) // 2},{tf(gate or v % 2 == 1)}>"
    if v >= CONV_IGEMM:  # igemm.hip / igemm_halo.hip: mode * 100 + MT * 10 + NT
        mode, mt, nt = (v - CONV_IGEMM) // 100, (v // 10) % 10, v % 10
        return f"igemm_halo_kernel<{nt},{mt},{mode - 1}>" if mode else f"igemm_glds_kernel<{nt},{mt}>"
    if v >= CONV_GEMM:
        return f"gemm_conv_kernel<{tname},{tf(v == CONV_GEMM)}>"
    return f"conv3d_mfma_kernel<{tname},{v // 10},{v % 10}>"


def dwconv_kernel_name(dv: int, tname: str, act: str, pool: bool, wo: int) -> str:
    actc = _lib.ACT[act]
    if dv >= DW_TEMPORAL:  # (never with pool partial rows: pasn_dwconv3d_pool_variant answers the strip kernel's code for a (kt,1,1) layer)
        return f"dwconv_t_kernel<{tname},{dv - DW_TEMPORAL}>"
    if dv >= DW_TZ:
        return f"dwconv3d_tz_kernel<{actc},{'true' if pool else 'false'}>"
    if dv >= DW_MFMA:  # the instance as the profiler prints it: <rows per position tile, ablation build, compiled-in activation>
        return f"dwconv3d_mfma_kernel<{2 if wo <= 8 else 1},false,{actc if actc in (_lib.ACT['none'], _lib.ACT['swish']) else -1}>"
    if dv >= DW_MARCH:
        return f"dwconv3d_march_kernel<{dv % 10},{dv // 10 % 100}>"
    if dv:
        return f"dwconv3d_strip_kernel<{tname},{dv // 100},{dv // 10 % 10},{dv % 10}>"
    return f"dwconv3d_kernel<{tname}>"


def fused_kernel_name(v: int, tname: str, transform: bool = False, res: bool = False, se: bool = False) -> str:
    """Instance names of the fused multi-stage launches, decoded from the library's codes (include/protoasnet_amd.h): ``pasn_conv3d_se_variant``
    (>= 7000, with ``se``), ``pasn_conv3d_pair_instance`` / ``pasn_conv3d_pair_se_variant`` (>= 10000), ``pasn_conv3d_short_variant`` (< 1000)."""
    tf = lambda b: "true" if b else "false"
    assert v > 0, "the launch is covered (its _supported probe said so) but its variant probe names no instance"
    if v >= 10000:
        ks1, ks2 = v // 100 % 100, v % 100
        if v // 10000 == 1:
            return f"pwconv_xpair_kernel<{ks1},{ks2},{tf(transform)}>"
        return f"pwconv_ws_kernel<{ks1},1,{tf(transform or se)},true,{ks2}>" + ("[se]" if se else "")
    if v >= CONV_PW_WS:
        return conv_kernel_name(v, tname, True, True, res) + "[se]"
    return f"pwconv_persist_kernel<{tname},{v // 100},{v // 10 % 10},false,{v % 10}>"


def x3d_pe_kernel_name(v: int, se: bool) -> str:
    """``pasn_x3d_pe_variant``'s code KSC * 1000 + KSA * 10 + MT."""
    assert v > 0
    return f"x3d_pe_kernel<{v // 1000},{v // 10 % 100},{'true' if se else 'false'},{v % 10}>"


def x3d_edp_kernel_name(v: int, nxt: bool) -> str:
    """``pasn_x3d_edp_variant``'s code KSA * 100 + KSC."""
    assert v > 0
    return f"x3d_edp_kernel<{v // 100},{v % 100},{'true' if nxt else 'false'}>"


class PlanBuilder:
    def __init__(self, device: torch.device, dtype: torch.dtype, in_dtype: torch.dtype, in_affine: Tuple[float, float] = (1.0, 0.0)):
        self.device, self.dtype, self.in_dtype = device, dtype, in_dtype
        self.in_affine = (float(in_affine[0]), float(in_affine[1]))  # x' = x * a + b on a grey (1-channel) input clip
        self.es = 2 if dtype == torch.bfloat16 else 4
        self.code = _lib.dtype_code(dtype)
        self.bufs: List[_Buf] = []
        self.ops: List[Callable[[List[int], int], None]] = []
        self.keep: List[object] = []  # packed weights / descriptors kept alive with the plan
        self.meta: List[dict] = []  # per launch: kernel instance name, algorithmic bytes and flops (DESIGN.md "Measurement")
        self.lib = _lib.lib()
        self.tname = "bf16" if dtype == torch.bfloat16 else "f32"
        # arrival counters of the fused SE-gate launches, one [N] slice per launch, packed so that Plan.run clears them with ONE fill before
        # the first launch (a launch that was aborted, or a replay that raced on a second stream, would otherwise leave a counter non-zero
        # and every later gate of that layer stale: a Plan is single-stream, and self-healing)
        self.se_counters: Optional[torch.Tensor] = None
        self.se_counters_used = 0

    # ---- buffers ---------------------------------------------------------------------------------
    def _new_buf(self, nbytes: int, external: bool = False) -> int:
        self.bufs.append(_Buf(round_up(max(nbytes, 1), ALIGN), len(self.ops), external))
        return len(self.bufs) - 1

    def _use(self, *buf_ids) -> None:
        for b in buf_ids:
            if b is not None:
                self.bufs[b].last = len(self.ops)

    def input(self, shape) -> Act:
        if len(shape) == 4:
            n, c, h, w = shape
            t = 1
        else:
            n, c, t, h, w = shape
        in_es = self._in_es()
        return Act(n, t, h, w, c, c, self._new_buf(n * c * t * h * w * in_es, external=True), planar=True)

    def _in_es(self) -> int:
        return {torch.bfloat16: 2, torch.uint8: 1}.get(self.in_dtype, 4)

    def _in_name(self) -> str:
        return {torch.bfloat16: "bf16", torch.uint8: "u8"}.get(self.in_dtype, "f32")

    # Probe first, allocate after: a method that may answer "not covered" asks the library with _geom() + _probe_desc(), which touch
    # neither ``bufs`` nor ``keep``, and reserves its outputs (_alloc) and keeps its descriptors only once the launch is certain.
    @staticmethod
    def _geom(x: Act, cout: int, k, s, p) -> Act:
        """Extents of a window sweep's output; no buffer yet (``buf`` = -1)."""
        to = (x.T + 2 * p[0] - k[0]) // s[0] + 1
        ho = (x.H + 2 * p[1] - k[1]) // s[1] + 1
        wo = (x.W + 2 * p[2] - k[2]) // s[2] + 1
        return Act(x.N, to, ho, wo, cout, round_up(cout, 8), -1)

    def _alloc(self, y: Act) -> Act:
        y.buf = self._new_buf(y.N * y.positions * y.Cp * self.es)
        return y

    def _out_act(self, x: Act, cout: int, k, s, p) -> Act:
        return self._alloc(self._geom(x, cout, k, s, p))

    @staticmethod
    def _probe_desc(x: Act, y: Act, k, s, p, act: str, in_swish=False, w_kc=0, w_rows=0, w_frag=0) -> ConvDesc:
        return ConvDesc(
            N=x.N, Ti=x.T, Hi=x.H, Wi=x.W, Cin=x.C, Cin_p=x.Cp, To=y.T, Ho=y.H, Wo=y.W, Cout=y.C, Cout_p=y.Cp,
            kt=k[0], kh=k[1], kw=k[2], st=s[0], sh=s[1], sw=s[2], pt=p[0], ph=p[1], pw=p[2],
            act=_lib.ACT[act], in_swish=int(bool(in_swish)), w_kc=w_kc, w_rows=w_rows, w_frag=w_frag,
        )

    def _desc(self, x: Act, y: Act, k, s, p, act: str, in_swish=False, w_kc=0, w_rows=0) -> ConvDesc:
        d = self._probe_desc(x, y, k, s, p, act, in_swish, w_kc, w_rows)
        self.keep.append(d)
        return d

    # ---- algorithmic work of one launch (true channel counts, every tensor moved once) -----------------
    @staticmethod
    def _touched(x: Act, y: Act, k, s) -> int:
        """Input positions a window sweep really needs (a 1x1 stride-2 conv reads a quarter of its input)."""
        t = x.T if k[0] >= s[0] else y.T * k[0]
        h = x.H if k[1] >= s[1] else y.H * k[1]
        w = x.W if k[2] >= s[2] else y.W * k[2]
        return x.N * min(t, x.T) * min(h, x.H) * min(w, x.W)

    def _note(self, kind: str, name: str, nbytes: int, flops: int, d: Optional[ConvDesc]) -> None:
        """``d``: the layer whose shape the launch's row shows.  The fused launches that pass None have an empty ``shape`` in the committed
        routing snapshot and in the benchmark's JSON (x3d_edp / expand_dw write their own); naming their layers changes both files."""
        shape = ""
        if d is not None:
            shape = (f"{d.Cin}->{d.Cout} k{d.kt}{d.kh}{d.kw} s{d.st}{d.sh}{d.sw} "
                     f"in{d.Ti}x{d.Hi}x{d.Wi} out{d.To}x{d.Ho}x{d.Wo}")
        self.meta.append({"kind": kind, "kernel": name, "bytes": int(nbytes), "flops": int(flops), "shape": shape})

    # ---- ops -------------------------------------------------------------------------------------
    def first_conv(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], act: str) -> Act:
        assert x.planar and x.C in (1, 3), "the first conv reads the planar 3-channel clip (or its single grey channel)"
        k, s, p = _triple(conv.kernel_size, 1), _triple(conv.stride, 1), _triple(conv.padding, 0)
        assert k[0] == 1 and s[0] == 1 and p[0] == 0, "first conv must be (1, kh, kw)"
        y = self._out_act(x, conv.out_channels, k, s, p)
        w = conv.weight.detach().float()
        if w.dim() == 5:
            w = w[:, :, 0]
        if x.C == 1:  # grey clip: the three input channels would be identical, so their taps are summed once here
            w = w.sum(dim=1, keepdim=True)
        scale, bias = fold_norm(norm, conv.bias, y.C, y.Cp, self.device)
        d = self._desc(x, y, k, s, p, act)
        code_in, code_out = _lib.dtype_code(self.in_dtype), self.code
        xb, yb, dref = x.buf, y.buf, ctypes.byref(d)
        self._use(xb, yb)
        in_es = self._in_es()
        out_pos = y.N * y.positions
        nbytes = self._touched(x, y, k, s) * x.C * in_es + out_pos * y.C * self.es
        flops = 2 * out_pos * y.C * x.C * k[1] * k[2]
        ia, ib = self.in_affine if x.C == 1 else (1.0, 0.0)
        slot = int(self.lib.pasn_first_conv_mfma_slot(dref, code_in, code_out))
        if slot >= 0:
            wq = pack_first_mfma(w, slot, y.Cp, self.device).to(torch.bfloat16).contiguous()  # matrix-core stem
            nq, bn = wq.shape[0], wq.shape[1]
            self.keep += [wq, scale, bias, d]
            a = (wq.data_ptr(), scale.data_ptr(), bias.data_ptr())
            self._note("first_conv", f"first_conv_mfma_kernel<{self._in_name()},{bn // 32},{nq // 2}>" + ("[grey]" if x.C == 1 else ""), nbytes, flops, d)
            fn = self.lib.pasn_first_conv_mfma_fwd
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], dref, code_in, ia, ib, st)))
            return y
        wp = pack_first_valu(w, y.Cp, self.device)
        self.keep += [wp, scale, bias, d]
        a = (wp.data_ptr(), scale.data_ptr(), bias.data_ptr())
        self._note("first_conv", f"first_conv_kernel<{self._in_name()},{self.tname},{y.Cp}>" + ("[grey]" if x.C == 1 else ""), nbytes, flops, d)
        if x.C == 1:
            fn = self.lib.pasn_first_conv_gray_fwd
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], dref, code_in, code_out, ia, ib, st)))
        else:
            fn = self.lib.pasn_first_conv_fwd
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], dref, code_in, code_out, st)))
        return y

    def x3d_stem(self, x: Act, conv_xy: nn.Module, conv_t: nn.Module, norm: nn.Module) -> Act:
        """X3D stem ((1,3,3) s2 conv -> depthwise (5,1,1) conv -> BN -> ReLU) as ONE launch; otherwise the two unfused ones."""
        k, s, p = _triple(conv_xy.kernel_size, 1), _triple(conv_xy.stride, 1), _triple(conv_xy.padding, 0)
        kt, st_, pt_ = _triple(conv_t.kernel_size, 1), _triple(conv_t.stride, 1), _triple(conv_t.padding, 0)
        c = conv_xy.out_channels
        y = self._geom(x, c, k, s, p)
        d = self._probe_desc(x, y, k, s, p, "relu")
        fusable = (x.planar and x.C in (1, 3) and kt == (5, 1, 1) and st_ == (1, 1, 1) and pt_ == (2, 0, 0) and conv_t.groups == c
                   and conv_xy.bias is None and conv_t.bias is None and bool(self.lib.pasn_x3d_stem_supported(ctypes.byref(d))))
        code_in, code_out = _lib.dtype_code(self.in_dtype), self.code
        mfma = fusable and bool(self.lib.pasn_x3d_stem_mfma_supported(ctypes.byref(d), code_in, code_out))
        if fusable and not mfma and self.in_dtype == torch.uint8 and x.C != 1:
            fusable = False  # x3d_stem_kernel reads uint8 from a grey clip only (stem.hip, stem_dispatch): the two launches have the instance
        if not fusable:
            e = self.first_conv(x, conv_xy, None, act="none")
            return self.dwconv(e, conv_t, norm, act="relu")
        self._alloc(y)
        wsrc = conv_xy.weight.detach().float()[:, :, 0]
        if x.C == 1:  # grey clip: taps summed over the three identical input channels (9 instead of 27)
            wsrc = wsrc.sum(dim=1, keepdim=True)
        if mfma:
            # matrix-core stem: both convs as one map, K rows R = (kt, ci, r), 4-wide window slots with tap s in slot 1 + s; rows in pairs
            wq = pack_stem_mfma(wsrc, conv_t.weight.detach().float().reshape(c, 5), self.device).to(torch.bfloat16).contiguous()
            scale, bias = fold_norm(norm, None, c, y.Cp, self.device)
            self.keep += [wq, scale, bias, d]
            a = (wq.data_ptr(), scale.data_ptr(), bias.data_ptr())
            xb, yb, dref = x.buf, y.buf, ctypes.byref(d)
            self._use(xb, yb)
            out_pos = y.N * y.positions
            self._note("stem", f"x3d_stem_mfma_kernel<{self._in_name()},{x.C}>",
                       x.N * x.C * x.positions * self._in_es() + out_pos * c * self.es, 2 * out_pos * c * (9 * x.C + 5), d)
            ia, ib = self.in_affine if x.C == 1 else (1.0, 0.0)
            fn = self.lib.pasn_x3d_stem_mfma_fwd
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], dref, code_in, ia, ib, st)))
            return y
        wxy, wt = pack_first_valu(wsrc, y.Cp, self.device), pack_dw_taps(conv_t.weight, y.Cp, self.device)
        scale, bias = fold_norm(norm, None, c, y.Cp, self.device)
        self.keep += [wxy, wt, scale, bias, d]
        a = (wxy.data_ptr(), wt.data_ptr(), scale.data_ptr(), bias.data_ptr())
        xb, yb, dref = x.buf, y.buf, ctypes.byref(d)
        self._use(xb, yb)
        in_es = self._in_es()
        out_pos = y.N * y.positions
        self._note("stem", f"x3d_stem_kernel<{self._in_name()},{self.tname},{y.Cp}{',grey' if x.C == 1 else ''}>",
                   x.N * x.C * x.positions * in_es + out_pos * c * self.es, 2 * out_pos * c * (9 * x.C + 5), d)
        if x.C == 1:
            fn, (ia, ib) = self.lib.pasn_x3d_stem_gray_fwd, self.in_affine
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], a[3], ptrs[yb], dref, code_in, code_out, ia, ib, st)))
        else:
            fn = self.lib.pasn_x3d_stem_fwd
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], a[3], ptrs[yb], dref, code_in, code_out, st)))
        return y

    def conv(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], act: str, residual: Optional[Act] = None,
             in_gate: Optional[int] = None, in_swish: bool = False) -> Act:
        assert not x.planar and conv.groups == 1
        k, s, p = _triple(conv.kernel_size, 1), _triple(conv.stride, 1), _triple(conv.padding, 0)
        y = self._out_act(x, conv.out_channels, k, s, p)
        wp, kc, rows = pack_conv_weight(conv.weight, x.Cp, self.dtype)
        scale, bias = fold_norm(norm, conv.bias, y.C, rows, self.device)
        d = self._desc(x, y, k, s, p, act, in_swish, kc, rows)
        self.keep += [wp, scale, bias]
        assert residual is None or same_extent(residual, y)
        fn, code = self.lib.pasn_conv3d_fwd, self.code
        a = (wp.data_ptr(), scale.data_ptr(), bias.data_ptr())
        xb, yb, rb, gb, dref = x.buf, y.buf, (residual.buf if residual is not None else None), in_gate, ctypes.byref(d)
        self._use(xb, yb, rb, gb)
        variant = int(self.lib.pasn_conv3d_variant(dref, self.code, int(in_gate is not None) | (2 if residual is not None else 0)))
        if CONV_PW_XTILE <= variant < CONV_IGEMM or variant >= CONV_PW_WS:
            # the X-tile and the weight-stationary kernels read fragment-major weights (tconv_ws_kernel: the K axis is (tap, channel) -- the
            # packed rows are [taps][kc] already)
            wf = fragment_major(wp)
            self.keep.append(wf)
            a = (wf.data_ptr(), a[1], a[2])
            d.w_frag = 1
        taps, out_pos = k[0] * k[1] * k[2], y.N * y.positions
        self._note("conv", conv_kernel_name(variant, self.tname, in_gate is not None, in_swish, residual is not None),
                   (self._touched(x, y, k, s) * x.C + out_pos * y.C * (2 if residual is not None else 1)
                    + y.C * x.C * taps) * self.es + (x.N * x.C * 4 if in_gate is not None else 0),
                   2 * out_pos * y.C * x.C * taps, d)
        self.ops.append(
            lambda ptrs, st: _lib.check(
                fn(ptrs[xb], a[0], a[1], a[2], ptrs[rb] if rb is not None else 0, ptrs[gb] if gb is not None else 0,
                   ptrs[yb], dref, code, st)
            )
        )
        return y

    def conv_se(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], act: str, residual: Optional[Act], pooled, fc1: nn.Module,
                fc2: nn.Module) -> Optional[Act]:
        """Project conv of an X3D SE block with the squeeze-excite gate computed in its own prologue from the stencil's pool partial rows
        (``pooled`` = what ``dwconv(..., pool=True)`` returned): no stand-alone gate launch, no gate tensor.  None = not covered."""
        one = (1, 1, 1)
        if x.planar or self.dtype != torch.bfloat16 or conv.groups != 1 or _triple(conv.kernel_size, 1) != one or _triple(conv.stride, 1) != one:
            return None
        pool_buf, pool_blocks, py = pooled
        c, cse = x.C, fc1.out_channels
        y = self._geom(x, conv.out_channels, one, one, (0, 0, 0))
        wp, kc, rows = pack_conv_weight(conv.weight, x.Cp, self.dtype)
        d = self._probe_desc(x, y, one, one, (0, 0, 0), act, True, kc, rows)
        if (py.N, py.positions, py.Cp) != (x.N, x.positions, x.Cp) or \
                not int(self.lib.pasn_conv3d_se_supported(ctypes.byref(d), self.code, cse, int(residual is not None))):
            return None
        assert residual is None or same_extent(residual, y)
        self._alloc(y)
        wf = fragment_major(wp)
        d.w_frag = 1
        scale, bias = fold_norm(norm, conv.bias, y.C, rows, self.device)
        w1, b1, w2, b2 = se_operands(fc1, fc2)
        self.keep += [d, wf, scale, bias, w1, b1, w2, b2]
        fn, code = self.lib.pasn_conv3d_se_fwd, self.code
        a = tuple(t.data_ptr() for t in (wf, scale, bias, w1, b1, w2, b2))
        xb, yb, rb, pbuf, dref, pos = x.buf, y.buf, (residual.buf if residual is not None else None), pool_buf, ctypes.byref(d), x.positions
        self._use(xb, yb, rb, pbuf)
        out_pos = y.N * y.positions
        self._note("conv+se", fused_kernel_name(int(self.lib.pasn_conv3d_se_variant(dref, self.code, cse, int(residual is not None))), self.tname,
                                                res=residual is not None, se=True),
                   (out_pos * (x.C + y.C * (2 if residual is not None else 1)) + y.C * x.C) * self.es + (x.N * pool_blocks * c + 2 * c * cse) * 4,
                   2 * out_pos * y.C * x.C + 4 * x.N * c * cse, None)
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[rb] if rb is not None else 0, ptrs[pbuf], pool_blocks, pos,
                                                       a[3], a[4], a[5], a[6], cse, ptrs[yb], dref, code, st)))
        return y

    def short_fusable(self, x: Act, blk) -> bool:
        """Whether ``conv_short`` will cover this block (asked BEFORE the block's launches are emitted: a fusable shortcut conv is not
        emitted on its own).  ``x`` = the block input, ``blk`` = a block with ``conv_c`` / ``shortcut.conv`` / ``se``."""
        if self.dtype != torch.bfloat16 or x.planar:
            return False
        sc, pc = blk.shortcut.conv, blk.conv_c
        if _triple(sc.kernel_size, 1) != (1, 1, 1) or _triple(pc.kernel_size, 1) != (1, 1, 1) or _triple(pc.stride, 1) != (1, 1, 1):
            return False
        s2 = _triple(sc.stride, 1)
        if s2[0] != 1:
            return False
        one, zero = (1, 1, 1), (0, 0, 0)
        mid = self._geom(x, pc.in_channels, one, s2, zero)  # the block's stencil output: the project conv's input
        y = self._geom(mid, pc.out_channels, one, one, zero)
        rows = round_up(y.Cp, 128)
        d = self._probe_desc(mid, y, one, one, zero, "relu", blk.se is not None, round_up(mid.Cp, 16), rows)
        d2 = self._probe_desc(x, y, one, s2, zero, "none", False, round_up(x.Cp, 16), rows)
        return bool(self.lib.pasn_conv3d_short_supported(ctypes.byref(d), ctypes.byref(d2), self.code))

    def conv_short(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], act: str, x2: Act, conv2: nn.Module, norm2: Optional[nn.Module],
                   in_gate: Optional[int] = None, in_swish: bool = False) -> Optional[Act]:
        """A block's project conv + norm with the block's strided 1x1x1 shortcut conv + norm accumulated in the SAME launch
        (``y = act(norm(conv(x')) + norm2(conv2(x2)))``): the first block of an X3D stage.  Returns None when the fused kernel does
        not cover the pair (the caller then emits the shortcut conv and the project conv with a residual)."""
        one = (1, 1, 1)
        if x.planar or x2.planar or self.dtype != torch.bfloat16 or conv.groups != 1 or conv2.groups != 1:
            return None
        if _triple(conv.kernel_size, 1) != one or _triple(conv.stride, 1) != one or _triple(conv2.kernel_size, 1) != one:
            return None
        s2 = _triple(conv2.stride, 1)
        y = self._geom(x, conv.out_channels, one, one, (0, 0, 0))
        wp, kc, rows = pack_conv_weight(conv.weight, x.Cp, self.dtype)
        d = self._probe_desc(x, y, one, one, (0, 0, 0), act, in_swish, kc, rows)
        w2, kc2, rows2 = pack_conv_weight(conv2.weight, x2.Cp, self.dtype)
        d2 = self._probe_desc(x2, y, one, s2, (0, 0, 0), "none", False, kc2, rows2)
        if (x2.T, (x2.H - 1) // s2[1] + 1, (x2.W - 1) // s2[2] + 1) != (y.T, y.H, y.W) or conv2.out_channels != conv.out_channels or \
                not int(self.lib.pasn_conv3d_short_supported(ctypes.byref(d), ctypes.byref(d2), self.code)):
            return None
        self._alloc(y)
        scale, bias = fold_norm(norm, conv.bias, y.C, rows, self.device)
        scale2, bias2 = fold_norm(norm2, conv2.bias, y.C, rows2, self.device)
        bias = (bias + bias2[: bias.numel()]).contiguous()
        self.keep += [d, d2, wp, w2, scale, bias, scale2]
        fn, code = self.lib.pasn_conv3d_short_fwd, self.code
        a = tuple(t.data_ptr() for t in (wp, scale, bias, w2, scale2))
        xb, x2b, gb, yb, r1, r2 = x.buf, x2.buf, in_gate, y.buf, ctypes.byref(d), ctypes.byref(d2)
        self._use(xb, x2b, gb, yb)
        pos = y.N * y.positions
        self._note("conv+shortcut", fused_kernel_name(int(self.lib.pasn_conv3d_short_variant(r1, r2, self.code)), self.tname),
                   (pos * (x.C + x2.C + y.C) + y.C * (x.C + x2.C)) * self.es + (x.N * x.C * 4 if in_gate is not None else 0),
                   2 * pos * y.C * (x.C + x2.C), d2)  # (the row shows the shortcut conv's shape: it carries the block's stride)
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[gb] if gb is not None else 0, ptrs[x2b], a[3], a[4],
                                                       ptrs[yb], r1, r2, code, st)))
        return y

    def conv_pair(self, x: Act, conv1: nn.Module, norm1: Optional[nn.Module], act1: str, residual: Act,
                  conv2: nn.Module, norm2: Optional[nn.Module], act2: str, in_gate: Optional[int] = None,
                  in_swish: bool = False, se=None):
        """Two chained 1x1x1 convs in ONE launch (X3D: a block's project conv + the next block's expand conv): returns
        (y1, y2), or None when the chained kernel does not cover the geometry (the caller then emits the two convs).
        ``se = (pooled, fc1, fc2)``: the first conv's squeeze-excite gate is computed in the launch's prologue from the stencil's pool
        partial rows (no gate launch, no gate tensor); None is returned when THAT form is not covered."""
        if x.planar or self.dtype != torch.bfloat16 or conv1.groups != 1 or conv2.groups != 1:
            return None
        one = (1, 1, 1)
        for cv in (conv1, conv2):
            if _triple(cv.kernel_size, 1) != one or _triple(cv.stride, 1) != one or _triple(cv.padding, 0) != (0, 0, 0):
                return None
        zero = (0, 0, 0)
        y1 = self._geom(x, conv1.out_channels, one, one, zero)
        w1, kc1, rows1 = pack_conv_weight(conv1.weight, x.Cp, self.dtype)
        d1 = self._probe_desc(x, y1, one, one, zero, act1, in_swish, kc1, rows1)
        y2 = self._geom(y1, conv2.out_channels, one, one, zero)
        w2, kc2, rows2 = pack_conv_weight(conv2.weight, y1.Cp, self.dtype)
        d2 = self._probe_desc(y1, y2, one, one, zero, act2, False, kc2, rows2)
        r1, r2 = ctypes.byref(d1), ctypes.byref(d2)
        (pool_buf, pool_blocks, py), fc1, fc2 = se if se is not None else ((None, 0, None), None, None)
        cse = fc1.out_channels if se is not None else 0
        pool_ok = se is None or (py.N, py.positions, py.Cp) == (x.N, x.positions, x.Cp)
        if se is not None:
            supported = pool_ok and int(self.lib.pasn_conv3d_pair_se_supported(r1, r2, self.code, cse))
        else:
            supported = int(self.lib.pasn_conv3d_pair_supported(r1, r2, self.code))
        pe = not supported
        if pe:
            # the 432-channel stage: both weight sets do not fit a wave's registers; x3d_pe.hip streams them per row tile instead (same contract,
            # bit-identical results).  Its weights are fragment-major with K zero-padded to an EVEN number of 16-wide steps
            w1, kc1, rows1 = pack_conv_weight(conv1.weight, round_up(x.Cp, 32), self.dtype)
            w2, kc2, rows2 = pack_conv_weight(conv2.weight, round_up(y1.Cp, 32), self.dtype)
            d1.w_kc, d1.w_rows, d2.w_kc, d2.w_rows = kc1, rows1, kc2, rows2
            d1.w_frag = d2.w_frag = 1
            if not (in_gate is None and pool_ok and same_extent(residual, y1) and int(self.lib.pasn_x3d_pe_supported(r1, r2, self.code, cse))):
                return None
        assert same_extent(residual, y1)
        d1.w_frag = d2.w_frag = 1
        self._alloc(y1)
        self._alloc(y2)
        w1f, w2f = fragment_major(w1), fragment_major(w2)
        s1, b1 = fold_norm(norm1, conv1.bias, y1.C, rows1, self.device)
        s2, b2 = fold_norm(norm2, conv2.bias, y2.C, rows2, self.device)
        sw = se_operands(fc1, fc2) if se is not None else []
        self.keep += [d1, d2, w1f, w2f, s1, b1, s2, b2] + sw
        a = tuple(t.data_ptr() for t in (w1f, s1, b1, w2f, s2, b2))
        sa = tuple(t.data_ptr() for t in sw) or (0, 0, 0, 0)
        xb, rb, gb, y1b, y2b, code = x.buf, residual.buf, in_gate, y1.buf, y2.buf, self.code
        self._use(xb, rb, gb, y1b, y2b, pool_buf)
        pos, npos = y1.N * y1.positions, x.positions
        nbytes = (pos * (x.C + 2 * y1.C + y2.C) + y1.C * x.C + y2.C * y1.C) * self.es
        flops = 2 * pos * (y1.C * x.C + y2.C * y1.C)
        if pe or se is not None:  # the two launches that can compute the gate in their prologue share one argument list
            nbytes += (x.N * pool_blocks * x.C + 2 * x.C * cse) * 4 if se is not None else 0
            if pe:
                fn = self.lib.pasn_x3d_pe_fwd
                self._note("conv_pair+se" if se is not None else "conv_pair",
                           x3d_pe_kernel_name(int(self.lib.pasn_x3d_pe_variant(r1, r2, self.code, cse)), se is not None), nbytes, flops, None)
            else:
                fn = self.lib.pasn_conv3d_pair_se_fwd
                self._note("conv_pair+se", fused_kernel_name(int(self.lib.pasn_conv3d_pair_se_variant(r1, r2, self.code, cse)), self.tname, se=True),
                           nbytes, flops + 4 * x.N * x.C * cse, None)
            self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[rb], ptrs[pool_buf] if pool_buf is not None else 0, pool_blocks, npos,
                                                           sa[0], sa[1], sa[2], sa[3], cse, ptrs[y1b], r1, a[3], a[4], a[5], ptrs[y2b], r2, code, st)))
            return y1, y2
        fn = self.lib.pasn_conv3d_pair_fwd
        pv = int(self.lib.pasn_conv3d_pair_instance(r1, r2, self.code, int(in_gate is not None)))
        self._note("conv_pair", fused_kernel_name(pv, self.tname, transform=in_gate is not None or in_swish),
                   nbytes + (x.N * x.C * 4 if in_gate is not None else 0), flops, None)
        self.ops.append(
            lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[rb], ptrs[gb] if gb is not None else 0, ptrs[y1b], r1,
                                           a[3], a[4], a[5], ptrs[y2b], r2, code, st))
        )
        return y1, y2

    def dwconv(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], act: str, pool: bool = False):
        assert not x.planar and conv.groups == conv.in_channels == conv.out_channels == x.C
        k, s, p = _triple(conv.kernel_size, 1), _triple(conv.stride, 1), _triple(conv.padding, 0)
        y = self._out_act(x, x.C, k, s, p)
        taps = k[0] * k[1] * k[2]
        wp = pack_dw_taps(conv.weight, y.Cp, self.device)
        scale, bias = fold_norm(norm, conv.bias, y.C, y.Cp, self.device)
        d = self._desc(x, y, k, s, p, act)
        self.keep += [wp, scale, bias]
        pool_buf, pool_blocks = None, 0
        if pool:
            pool_blocks = int(self.lib.pasn_dwconv3d_pool_blocks(ctypes.byref(d), self.code))
            pool_buf = self._new_buf(y.N * pool_blocks * y.Cp * 4)
        fn, code = self.lib.pasn_dwconv3d_fwd, self.code
        a = (wp.data_ptr(), scale.data_ptr(), bias.data_ptr())
        xb, yb, pb, dref = x.buf, y.buf, pool_buf, ctypes.byref(d)
        self._use(xb, yb, pb)
        out_pos = y.N * y.positions
        dv = int((self.lib.pasn_dwconv3d_pool_variant if pool else self.lib.pasn_dwconv3d_variant)(dref, self.code))
        self._note("dwconv", dwconv_kernel_name(dv, self.tname, act, pool, y.W),
                   (self._touched(x, y, k, s) + out_pos) * y.C * self.es + (y.N * pool_blocks * y.C * 4 if pool else 0),
                   2 * out_pos * y.C * taps, d)
        self.ops.append(
            lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], ptrs[pb] if pb is not None else 0, dref, code, st))
        )
        return (y, (pool_buf, pool_blocks, y)) if pool else y

    def x3d_edp(self, x: Act, conv_a: nn.Module, norm_a, conv_b: nn.Module, norm_b, conv_c: nn.Module, norm_c, conv_n: Optional[nn.Module] = None,
                norm_n=None, probe: bool = False):
        """A WHOLE X3D block without squeeze-excite on 7 x 7 planes in ONE launch (``pasn_x3d_edp_fwd``): expand conv + BN + ReLU -> depthwise
        3x3x3 + BN + Swish -> project conv + BN + x + ReLU (-> ``conv_n``: the next block's expand conv + BN + ReLU).  ``x`` = the block input.
        Returns (y, e_next or None), or None when the launch does not cover the block.  ``probe``: only say whether it would (True / False)."""
        one, zero = (1, 1, 1), (0, 0, 0)
        ok = (not x.planar and self.dtype == torch.bfloat16 and conv_b.groups == conv_b.in_channels == conv_a.out_channels and conv_a.groups == 1
              and conv_c.groups == 1 and conv_a.in_channels == x.C and conv_c.in_channels == conv_b.in_channels and conv_c.out_channels == x.C
              and conv_b.bias is None and _triple(conv_b.kernel_size, 1) == (3, 3, 3) and _triple(conv_b.stride, 1) == one
              and _triple(conv_b.padding, 0) == (1, 1, 1))
        for cv in (conv_a, conv_c, conv_n):
            ok = ok and (cv is None or (_triple(cv.kernel_size, 1) == one and _triple(cv.stride, 1) == one and _triple(cv.padding, 0) == zero and cv.groups == 1))
        if not ok or (conv_n is not None and conv_n.in_channels != conv_c.out_channels):
            return False if probe else None
        cm = conv_a.out_channels
        mid = self._geom(x, cm, one, one, zero)   # expanded activation / stencil output: never materialised
        y = self._geom(mid, conv_c.out_channels, one, one, zero)
        da = self._probe_desc(x, mid, one, one, zero, "relu", False, round_up(x.Cp, 16), round_up(mid.Cp, 128), w_frag=1)
        dd = self._probe_desc(mid, mid, (3, 3, 3), one, (1, 1, 1), "swish")
        dc = self._probe_desc(mid, y, one, one, zero, "relu", False, round_up(mid.Cp, 32), round_up(y.Cp, 128), w_frag=1)
        dn = en = None
        if conv_n is not None:
            en = self._geom(y, conv_n.out_channels, one, one, zero)
            dn = self._probe_desc(y, en, one, one, zero, "relu", False, round_up(y.Cp, 16), round_up(en.Cp, 128), w_frag=1)
        if not int(self.lib.pasn_x3d_edp_supported(ctypes.byref(da), ctypes.byref(dd), ctypes.byref(dc), ctypes.byref(dn) if dn is not None else None, self.code)):
            return False if probe else None
        if probe:
            return True
        wa, kca, ra = pack_conv_weight(conv_a.weight, x.Cp, self.dtype)
        wc, kcc, rc = pack_conv_weight(conv_c.weight, round_up(mid.Cp, 32), self.dtype)
        assert (kca, ra, kcc, rc) == (da.w_kc, da.w_rows, dc.w_kc, dc.w_rows)
        sa, ba = fold_norm(norm_a, conv_a.bias, cm, ra, self.device)
        wd = stencil_operands(conv_b.weight.to(self.device), cm, mid.Cp)
        sd, bd = fold_norm(norm_b, None, cm, mid.Cp, self.device)
        sc, bc = fold_norm(norm_c, conv_c.bias, x.C, rc, self.device)
        keep = [fragment_major(wa), sa, ba, wd, sd, bd, fragment_major(wc), sc, bc]
        self._alloc(y)
        if conv_n is not None:
            self._alloc(en)
            wn, kcn, rn = pack_conv_weight(conv_n.weight, y.Cp, self.dtype)
            sn, bn = fold_norm(norm_n, conv_n.bias, en.C, rn, self.device)
            keep += [fragment_major(wn), sn, bn]
        self.keep += keep + [da, dd, dc] + ([dn] if dn is not None else [])
        a = tuple(t.data_ptr() for t in keep) + ((0, 0, 0) if conv_n is None else ())
        xb, yb, nb = x.buf, y.buf, (en.buf if en is not None else None)
        r = (ctypes.byref(da), ctypes.byref(dd), ctypes.byref(dc), ctypes.byref(dn) if dn is not None else None)
        self._use(xb, yb, nb)
        pos, cn = y.N * y.positions, (en.C if en is not None else 0)
        self._note("block" if en is None else "block+expand", x3d_edp_kernel_name(int(self.lib.pasn_x3d_edp_variant(r[0], r[1], r[2], r[3], self.code)), en is not None),
                   (pos * (2 * x.C + y.C + cn) + cm * x.C + 27 * cm + y.C * cm + cn * y.C) * self.es, 2 * pos * (cm * x.C + 27 * cm + y.C * cm + cn * y.C), None)
        self.meta[-1]["shape"] = f"{x.C}->{cm} k111 -> dw k333 -> {cm}->{y.C}" + (f" -> {y.C}->{cn}" if cn else "") + f" k111 in{x.T}x{x.H}x{x.W}"
        fn, code = self.lib.pasn_x3d_edp_fwd, self.code
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], ptrs[yb], a[9], a[10], a[11],
                                                       ptrs[nb] if nb is not None else 0, r[0], r[1], r[2], r[3], code, st)))
        return y, en

    def expand_dw(self, x: Act, conv_a: nn.Module, norm_a: Optional[nn.Module], conv_b: nn.Module, norm_b: Optional[nn.Module], act_b: str,
                  pool: bool = False):
        """Front half of an X3D block in ONE launch (``pasn_x3d_expdw_fwd``): 1x1x1 expand conv + BN + ReLU -> depthwise 3x3x3 conv,
        stride (1,s,s) with s = 1 or 2, + BN (+ ``act_b``, + squeeze-excite pool partial rows); the expanded activation stays in LDS.
        Returns y (or (y, pooled) with ``pool``), or None when the pair is not covered (the caller emits the two launches)."""
        if x.planar or self.dtype != torch.bfloat16 or conv_a.groups != 1 or conv_b.groups != conv_b.in_channels:
            return None
        one, zero = (1, 1, 1), (0, 0, 0)
        if _triple(conv_a.kernel_size, 1) != one or _triple(conv_a.stride, 1) != one or _triple(conv_a.padding, 0) != zero:
            return None
        k, s, p = _triple(conv_b.kernel_size, 1), _triple(conv_b.stride, 1), _triple(conv_b.padding, 0)
        if k != (3, 3, 3) or s not in ((1, 1, 1), (1, 2, 2)) or p != (1, 1, 1) or conv_b.in_channels != conv_a.out_channels:
            return None
        cm = conv_a.out_channels
        mid = self._geom(x, cm, one, one, zero)  # the expanded activation: never materialised
        # norm_a's scale goes INTO the expand weights (W * scale, rounded to bf16 once) and its bias becomes the accumulator's initial
        # value: the fused kernel's expand epilogue is then swap + ReLU + rounding (PASN_EXPDW_FOLD=0: scale and bias applied in fp32
        # after the MFMAs, the rounding points of the two separate launches)
        fold = (_lib.tuning_get("PASN_EXPDW_FOLD") or "1") != "0"
        sa_full, _ = fold_norm(norm_a, conv_a.bias, cm, cm, self.device)
        w_src = conv_a.weight.detach().float() * sa_full.to(conv_a.weight.device).view(-1, 1, 1, 1, 1) if fold else conv_a.weight
        wa, kca, rowsa = pack_conv_weight(w_src, x.Cp, self.dtype)
        de = self._probe_desc(x, mid, one, one, zero, "relu", False, kca, rowsa)
        y = self._geom(mid, cm, k, s, p)
        d = self._probe_desc(mid, y, k, s, p, act_b)
        if not int(self.lib.pasn_x3d_expdw_supported(ctypes.byref(de), ctypes.byref(d), self.code)):
            return None
        self._alloc(y)
        waf = fragment_major(wa)
        de.w_frag = 1
        sa, ba = fold_norm(norm_a, conv_a.bias, cm, rowsa, self.device)
        wp = pack_dw_taps(conv_b.weight, y.Cp, self.device)
        sb, bb = fold_norm(norm_b, conv_b.bias, y.C, y.Cp, self.device)
        self.keep += [de, d, waf, sa, ba, wp, sb, bb]
        pool_buf, pool_blocks = None, 0
        if pool:
            pool_blocks = int(self.lib.pasn_x3d_expdw_pool_blocks(ctypes.byref(de), ctypes.byref(d), self.code))
            pool_buf = self._new_buf(y.N * pool_blocks * y.Cp * 4)
        fn, code = self.lib.pasn_x3d_expdw_fwd, self.code
        a = tuple(t.data_ptr() for t in (waf, sa, ba, wp, sb, bb))
        if fold:
            a = (a[0], 0) + a[2:]
        xb, yb, pb_, re_, rd_ = x.buf, y.buf, pool_buf, ctypes.byref(de), ctypes.byref(d)
        self._use(xb, yb, pb_)
        in_pos, out_pos = x.N * x.positions, y.N * y.positions
        actc = _lib.ACT[act_b]
        tz = int(self.lib.pasn_x3d_expdw_variant(ctypes.byref(de), ctypes.byref(d), self.code)) == 1
        self._note("expand+dwconv", f"x3d_expdw_tz_kernel<1,{actc},{'true' if pool else 'false'}>" if tz else
                   f"x3d_expdw_kernel<{2 if kca // 16 <= 2 else 3},{actc if actc in (_lib.ACT['none'], _lib.ACT['swish']) else -1},{s[1]}>",
                   (in_pos * x.C + out_pos * y.C + cm * x.C) * self.es + (y.N * pool_blocks * y.C * 4 if pool else 0),
                   2 * in_pos * cm * x.C + 2 * out_pos * y.C * 27, None)
        self.meta[-1]["shape"] = f"{x.C}->{cm} k111 + dw k333 s1{s[1]}{s[2]} in{x.T}x{x.H}x{x.W} out{y.T}x{y.H}x{y.W}"
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], a[3], a[4], a[5], ptrs[yb],
                                                       ptrs[pb_] if pb_ is not None else 0, re_, rd_, code, st)))
        return (y, (pool_buf, pool_blocks, y)) if pool else y

    def _gate_in_prologue(self, y: Act, fc1: nn.Module, consumer) -> bool:
        """Whether the project conv (``consumer`` = (conv_c, has residual), or None) of the SE block whose stencil output is ``y`` computes
        the gate in its own prologue (``pasn_conv3d_se_fwd`` and the chained launches built on it)."""
        if consumer is None or self.dtype != torch.bfloat16:
            return False
        cc, has_res = consumer
        one, zero = (1, 1, 1), (0, 0, 0)
        out = self._geom(y, cc.out_channels, one, one, zero)
        dc = self._probe_desc(y, out, one, one, zero, "relu", True, round_up(y.Cp, 16), round_up(out.Cp, 128))
        return bool(self.lib.pasn_conv3d_se_supported(ctypes.byref(dc), self.code, fc1.out_channels, int(has_res)))

    def se_gate_or_prologue(self, y: Act, pooled, fc1: nn.Module, fc2: nn.Module, consumer=None):
        """The gate of an SE block whose stencil produced pool partial rows: ("pooled", pooled) where the project conv (``consumer`` =
        (conv_c, has residual)) computes it in its own prologue, else the stand-alone gate launch's buffer."""
        if self._gate_in_prologue(y, fc1, consumer):
            return ("pooled", pooled)
        return self.se_gate(pooled, fc1, fc2)

    def dwconv_se(self, x: Act, conv: nn.Module, norm: Optional[nn.Module], fc1: nn.Module, fc2: nn.Module, consumer=None):
        """Depthwise 3x3x3 conv + BN (no activation: the gate comes first) + the block's squeeze-excite gate in ONE launch where the
        T-marching stencil covers the layer (the clip's last-arriving block computes the gate); otherwise the stencil launch followed
        by the stand-alone gate launch.  Returns (y, gate buffer id)."""
        assert not x.planar and conv.groups == conv.in_channels == conv.out_channels == x.C
        k, s, p = _triple(conv.kernel_size, 1), _triple(conv.stride, 1), _triple(conv.padding, 0)
        y = self._geom(x, x.C, k, s, p)
        d = self._probe_desc(x, y, k, s, p, "none")
        c, cse = y.C, fc1.out_channels
        if not int(self.lib.pasn_dwconv3d_se_supported(ctypes.byref(d), self.code, cse)):
            y, pooled = self.dwconv(x, conv, norm, act="none", pool=True)
            # the project conv may compute the gate in its own prologue: then only the pool partial rows are produced here
            return y, (("pooled", pooled) if self._gate_in_prologue(y, fc1, consumer) else self.se_gate(pooled, fc1, fc2))
        self._alloc(y)
        taps = k[0] * k[1] * k[2]
        wp = pack_dw_taps(conv.weight, y.Cp, self.device)
        scale, bias = fold_norm(norm, conv.bias, y.C, y.Cp, self.device)
        w1, b1, w2, b2 = se_operands(fc1, fc2)
        if self.se_counters is None:
            self.se_counters = torch.zeros(4096, dtype=torch.int32, device=self.device)
        assert self.se_counters_used + y.N <= self.se_counters.numel(), "too many fused SE-gate launches for the counter block"
        counter = self.se_counters[self.se_counters_used: self.se_counters_used + y.N]  # the kernel leaves it zero; Plan.run clears it anyway
        self.se_counters_used += (y.N + 3) // 4 * 4
        self.keep += [d, wp, scale, bias, w1, b1, w2, b2, counter]
        pool_blocks = int(self.lib.pasn_dwconv3d_se_pool_blocks(ctypes.byref(d), self.code))
        pool_buf = self._new_buf(y.N * pool_blocks * y.Cp * 4)
        gate = self._new_buf(y.N * y.Cp * 4)
        fn, code = self.lib.pasn_dwconv3d_se_fwd, self.code
        a = tuple(t.data_ptr() for t in (wp, scale, bias, w1, b1, w2, b2, counter))
        xb, yb, pb_, dref = x.buf, y.buf, pool_buf, ctypes.byref(d)
        self._use(xb, yb, pb_, gate)
        out_pos = y.N * y.positions
        dv = int(self.lib.pasn_dwconv3d_variant(dref, self.code))
        # the T-marching VALU stencil's instance (the layer's plain launch may be routed elsewhere: then only the stride is known here)
        kname = dwconv_kernel_name(dv, self.tname, "none", True, y.W) if DW_MARCH <= dv < DW_MFMA else f"dwconv3d_march_kernel<{s[2]},se>"
        self._note("dwconv+se", kname,
                   (self._touched(x, y, k, s) + out_pos) * y.C * self.es + (y.N * pool_blocks * y.C * 8 + y.N * c * 4 + 2 * c * cse * 4),
                   2 * out_pos * y.C * taps + 4 * y.N * c * cse, None)
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], a[0], a[1], a[2], ptrs[yb], ptrs[pb_], dref, code, a[3], a[4], a[5], a[6],
                                                       cse, ptrs[gate], a[7], st)))
        return y, gate

    def se_gate(self, pooled, fc1: nn.Module, fc2: nn.Module) -> int:
        pool_buf, pool_blocks, y = pooled
        c, cse = y.C, fc1.out_channels
        w1, b1, w2, b2 = se_operands(fc1, fc2)
        self.keep += [w1, b1, w2, b2]
        gate = self._new_buf(y.N * y.Cp * 4)
        fn = self.lib.pasn_se_gate_fwd
        a = (w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr())
        n, cp, pos = y.N, y.Cp, y.positions
        self._use(pool_buf, gate)
        self._note("se_gate", "se_gate_kernel", (y.N * pool_blocks * c + y.N * c + 2 * c * cse) * 4, 4 * y.N * c * cse, None)
        self.ops.append(
            lambda ptrs, st: _lib.check(fn(ptrs[pool_buf], pool_blocks, pos, a[0], a[1], a[2], a[3], ptrs[gate], n, c, cp, cse, st))
        )
        return gate

    def maxpool(self, x: Act, k, s, p) -> Act:
        y = self._out_act(x, x.C, k, s, p)
        d = self._desc(x, y, k, s, p, "none")
        fn, code = self.lib.pasn_maxpool3d_fwd, self.code
        xb, yb, dref = x.buf, y.buf, ctypes.byref(d)
        self._use(xb, yb)
        self._note("maxpool", f"maxpool3d_kernel<{self.tname}>", (self._touched(x, y, k, s) + y.N * y.positions) * y.C * self.es, 0, d)
        self.ops.append(lambda ptrs, st: _lib.check(fn(ptrs[xb], ptrs[yb], dref, code, st)))
        return y

    # ---- arena planning ---------------------------------------------------------------------------
    def _place(self) -> int:
        """First-fit offset of every internal buffer, in creation order, among the buffers still live then; returns the arena size."""
        live: List[Tuple[int, int, int]] = []  # (offset, size, last)
        total = 0
        for b in self.bufs:
            if b.external:
                continue
            live = [a for a in live if a[2] >= b.first]  # still needed by the op that produces b, or later
            live.sort()
            off = 0
            for (o, sz, _) in live:
                if off + b.nbytes <= o:
                    break
                off = max(off, o + sz)
            b.offset = off
            live.append((off, b.nbytes, b.last))
            total = max(total, off + b.nbytes)
        return total

    def finish(self, x_in: Act, y_out: Act) -> "Plan":
        self.bufs[y_out.buf].external = True
        return Plan(self, x_in, y_out, self._place())


class Plan:
    def __init__(self, pb: PlanBuilder, x_in: Act, y_out: Act, arena_bytes: int):
        self.ops, self.keep, self.meta = pb.ops, pb.keep, pb.meta
        self.in_buf, self.out_buf, self.out = x_in.buf, y_out.buf, y_out
        self.dtype = pb.dtype
        self.arena_bytes = arena_bytes
        self.naive_bytes = sum(b.nbytes for b in pb.bufs if not b.external)
        self.se_counters = pb.se_counters[: pb.se_counters_used] if pb.se_counters is not None else None
        self.arena = torch.empty(arena_bytes + ALIGN, dtype=torch.uint8, device=pb.device)
        base = round_up(self.arena.data_ptr(), ALIGN)
        self.ptrs = [0 if b.external else base + b.offset for b in pb.bufs]

    def run(self, x: torch.Tensor, timers: Optional[Dict[int, list]] = None) -> torch.Tensor:
        """Replay the launches on torch's current stream.  ``timers`` maps launch index -> list that receives one
        (start, end) ``torch.cuda.Event`` pair per replay (events are recorded on the same stream as the kernel)."""
        o = self.out
        y = torch.empty((o.N, o.T, o.H, o.W, o.Cp), dtype=self.dtype, device=x.device)
        ptrs = self.ptrs
        ptrs[self.in_buf] = x.data_ptr()
        ptrs[self.out_buf] = y.data_ptr()
        st = _lib.current_stream()
        if self.se_counters is not None:
            self.se_counters.zero_()  # one 16-byte-multiple fill on the launch stream (see PlanBuilder.__init__)
        if not timers:
            for op in self.ops:
                op(ptrs, st)
            return y
        for i, op in enumerate(self.ops):
            sink = timers.get(i)
            if sink is None:
                op(ptrs, st)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            op(ptrs, st)
            e1.record()
            sink.append((e0, e1))
        return y


def tensor_signature(tensors) -> tuple:
    """(storage address, autograd version counter) of every tensor: moves on ``load_state_dict``, ``.to()``, an optimizer step and any
    other in-place op -- but NOT on a write through ``.data`` or a raw pointer, which bumps no counter."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


class PlanCache:
    """Compiled device state (plans, packed weights, training runners, captured graphs) by key.  An entry is stamped with
    (``signature()``, tuning epoch) when it is built and is good only while that stamp is the current one; a miss first drops EVERY
    entry with another stamp (none can hit again, and two generations of arenas are never held at once), then builds.  With
    ``max_entries`` the least recently used entries beyond it are evicted, each reported through ``on_evict(key)``."""

    def __init__(self, signature: Callable[[], tuple], max_entries: Optional[int] = None, on_evict: Optional[Callable] = None):
        self.signature, self.max_entries, self.on_evict = signature, max_entries, on_evict
        self._entries: Dict[tuple, tuple] = {}  # key -> (stamp, value), least recently used first

    def lookup(self, key, make: Callable):
        stamp = (self.signature(), _lib.tuning_epoch())
        hit = self._entries.get(key)
        if hit is not None and hit[0] == stamp:
            self._entries[key] = self._entries.pop(key)  # most recently used last
            return hit[1]
        self._entries = {k: v for k, v in self._entries.items() if v[0] == stamp}
        value = make()
        self._entries[key] = (stamp, value)
        while self.max_entries is not None and len(self._entries) > self.max_entries:
            old = next(iter(self._entries))
            del self._entries[old]
            if self.on_evict is not None:
                self.on_evict(old)
        return value

    def values(self) -> list:
        return [v for _, v in self._entries.values()]

    def clear(self) -> None:
        self._entries = {}

    def __len__(self) -> int:
        return len(self._entries)


def logical_view(y: torch.Tensor, channels: int, video: bool) -> torch.Tensor:
    """Channels-last storage [N][T][H][W][Cp] -> the reference's logical (N,C,[T,]H,W) tensor (a strided view)."""
    v = y[..., :channels].permute(0, 4, 1, 2, 3)
    return v if video else v[:, :, 0]


def channels_last_rows(feat: torch.Tensor, dtype: torch.dtype) -> Tuple[torch.Tensor, int, int]:
    """Logical (N,C,[T,]H,W) tensor -> ([N][S][Cp] storage, S, Cp); zero-copy for views made by ``logical_view``."""
    n, c = feat.shape[0], feat.shape[1]
    s = 1
    for v in feat.shape[2:]:
        s *= int(v)
    if feat.dtype == dtype and feat.stride(1) == 1 and feat.stride(-1) % 8 == 0 and feat.stride(-1) >= c:
        cp = feat.stride(-1)
        strides, expect = feat.stride(), cp
        ok = True
        for dim in range(feat.dim() - 1, 1, -1):
            if feat.shape[dim] != 1 and strides[dim] != expect:
                ok = False
            expect *= feat.shape[dim]
        if ok and (n == 1 or strides[0] == expect):
            rows = torch.as_strided(feat, (n, s, cp), (s * cp, cp, 1), feat.storage_offset())
            return rows, s, cp
    # foreign layout (e.g. a planar tensor from a non-HIP trunk): repack with torch, zero padded channels
    cp = round_up(c, 8)
    rows = torch.zeros((n, s, cp), dtype=dtype, device=feat.device)
    rows[:, :, :c] = feat.reshape(n, c, s).transpose(1, 2).to(dtype)
    return rows, s, cp


class HipTrunk(nn.Module):
    """Base of the feature trunks: parameter container + cached eval-mode HIP plans; ``build_train`` feeds the training tape."""

    arch = "trunk"
    out_channels = 0

    def __init__(self):
        super().__init__()
        self._plans = PlanCache(self._signature)
        self.compute_dtype: Optional[torch.dtype] = None  # None: follow the parameter dtype
        self.input_affine: Tuple[float, float] = (1.0, 0.0)  # x' = x * a + b applied to a GREY (1-channel) input while loading

    def set_input_normalization(self, mean: Optional[float] = None, std: Optional[float] = None, scale: float = 1.0) -> "HipTrunk":
        """Device-side normalisation of grey (N,1,...) input clips: x' = (x * scale - mean) / std, fused into the first layer's loads
        (reference: host-side ``bin_to_norm``, as_dataloader.py:173-182, mean 0.099 / std 0.171; ``scale`` = 1/255 for uint8 clips).
        ``mean=None`` switches it off (the clip is already normalised).  3-channel inputs are never transformed."""
        self.input_affine = (1.0, 0.0) if mean is None else (float(scale) / float(std), -float(mean) / float(std))
        return self

    def build_plan(self, pb: PlanBuilder, x: Act) -> Act:  # pragma: no cover - overridden
        raise NotImplementedError

    def build_train(self, tb, x: Act) -> Act:
        raise NotImplementedError(
            f"{type(self).__name__}: no training launch list is defined for this trunk"
        )

    def _signature(self) -> tuple:
        return tensor_signature(list(self.parameters()) + list(self.buffers()))

    def invalidate_plans(self) -> None:
        """Drop every cached launch list (and its packed weights).  The cache stamp is (storage address, autograd version counter) of
        every parameter / buffer, which sees optimizer steps, ``load_state_dict``, ``.to()`` and any in-place op on the parameter --
        but NOT a write through ``param.data`` or a raw pointer, which bumps no counter.  Code that does that to a trunk calls this
        afterwards.  (The reference writes through ``.data`` only to ``prototype_vectors`` and ``last_layer.weight``
        (push_abs_revision.py:346, ProtoPNet.py:308-311); neither is packed or cached here.)"""
        self._plans.clear()

    def plan_for(self, x: torch.Tensor) -> Plan:
        dtype = self.compute_dtype or next(self.parameters()).dtype

        def make() -> Plan:
            pb = PlanBuilder(x.device, dtype, x.dtype, self.input_affine)
            x_in = pb.input(tuple(x.shape))
            with torch.no_grad():
                y_out = self.build_plan(pb, x_in)
            return pb.finish(x_in, y_out)

        return self._plans.lookup((tuple(x.shape), x.dtype, dtype, x.device, self.input_affine if x.shape[1] == 1 else None), make)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise NotImplementedError(
                f"{type(self).__name__}: a trunk on its own runs eval-mode inference only -- call .eval(); training compiles trunk + "
                "head of a XProtoNet / Video_XProtoNet model into one forward + backward launch list (model.train(); train.py)"
            )
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(
                f"{type(self).__name__}: the eval-mode HIP forward records no autograd graph; run it under torch.no_grad()"
            )
        if not x.is_cuda:
            raise RuntimeError("protoasnet_amd trunks run on the GPU only (input is on %s); there is no CPU fallback" % x.device)
        if x.dim() not in (4, 5) or x.shape[1] not in (1, 3):
            raise ValueError("expected (N,3,H,W) / (N,3,T,H,W) input -- or the single grey channel (N,1,...) of an echo clip -- got %s"
                             % (tuple(x.shape),))
        if x.dtype == torch.uint8 and x.shape[1] != 1:
            raise ValueError("uint8 clips are accepted as single-channel (N,1,...) input only")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            x = x.float()
        x = x.contiguous()
        plan = self.plan_for(x)
        y = plan.run(x, getattr(self, "_timers", None))  # bench.py brackets chosen launches with HIP events
        return logical_view(y, plan.out.C, video=(x.dim() == 5))
