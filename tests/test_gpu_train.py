"""GPU: the training path (train-mode forward with batch statistics + backward) against torch autograd on the CPU.

Kernel level: each training entry point of the C-ABI vs autograd of the same fp32 torch expression.
Model level: ``model.train()`` forward + ``loss.backward()`` of Video_XProtoNet on the X3D-S trunk vs the oracle's train-mode
pass differentiated by autograd (outputs, every parameter gradient, running statistics; fp32 tolerance 1e-3 of each
tensor's scale -- BASELINE north_star), an optimizer step in between (weights are re-packed from the live parameters), and
the bf16 activation mode as a tolerance check."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import oracle
import train_kernel_cases as tk
from conftest import assert_close
from protoasnet_amd import _lib, synth
from protoasnet_amd._lib import ConvDesc, XProtoDesc
from util import CFG_PPNET, CFG_PPNET_BOTTLENECK, CFG_VIDEO_R2P1D, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = 0, 1


def _cl(x, cp=None, dtype=torch.float32):
    """(N,C,T,H,W) -> channels-last [N][T][H][W][Cp] on the GPU, zero padded."""
    n, c = x.shape[:2]
    cp = cp or (c + 7) // 8 * 8
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=dtype, device=DEV)
    out[..., :c] = x.permute(0, 2, 3, 4, 1).to(DEV).to(dtype)
    return out


def _ncl(y, c):
    return y[..., :c].permute(0, 4, 1, 2, 3).float().cpu()


def _st():
    return _lib.current_stream()


def _rel(a, e, tol, name):
    a, e = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(e).detach().float().cpu()
    scale = float(e.abs().max()) + 1e-12
    assert_close(a, e, tol * scale, 0.0, f"{name} (scale {scale:.3g})")


def _desc(x, y, k, s, p):
    return ConvDesc(N=x.shape[0], Ti=x.shape[2], Hi=x.shape[3], Wi=x.shape[4], Cin=x.shape[1], Cin_p=(x.shape[1] + 7) // 8 * 8,
                    To=y.shape[2], Ho=y.shape[3], Wo=y.shape[4], Cout=y.shape[1], Cout_p=(y.shape[1] + 7) // 8 * 8,
                    kt=k[0], kh=k[1], kw=k[2], st=s[0], sh=s[1], sw=s[2], pt=p[0], ph=p[1], pw=p[2])


# ------------------------------------------------------------------------------------------------- kernels
# The cases (inputs, fp64 references) come from tests/train_kernel_cases.py; tests/test_cpu_train_kernel_cases.py checks them without a GPU.
# Bounds: fp32 as ever (1e-5 ... 2e-4 of a tensor's scale).  bf16: the activations are rounded BEFORE the reference is taken, so sums the
# kernels take in fp32 keep the fp32 bound, and an elementwise output behind k stores in bf16 gets k * 2^-8 of its scale on top
# (tk.tol_stores; round-to-nearest is within 2^-9, the factor 2 is the margin).
FP32, BF = torch.float32, torch.bfloat16


def _variants(cases, ids):
    """cases x {fp32, bf16} x PASN_TRAIN_ROWS_CONTIG {unset, 1}; the fp32 run with the switch unset carries the bare id of its case."""
    return [pytest.param(case, dtype, contig, id=cid + ("" if dtype == FP32 and not contig else f"-{dname}-{lname}"))
            for case, cid in zip(cases, ids) for dtype, dname in ((FP32, "fp32"), (BF, "bf16")) for contig, lname in ((False, "default"), (True, "rows-contig"))]


UNIT_IDS = ["54-shape0-0.0", "24-shape1-300.0", "432-shape2--5.0", "24-2x1x5x5", "432-2x3x7x7", "54-3x3x21x19", "24-2x3x31x31"]
GROUP_IDS = ["54-shape0-2", "24-shape1-3", "216-shape2-2", "54-4x3x21x19-2"]
SE_IDS = ["54-8-2x5x6", "432-32-3x7x7", "54-8-3x21x19"]


def _rows_switch(monkeypatch, contig):
    if contig:
        monkeypatch.setenv("PASN_TRAIN_ROWS_CONTIG", "1")
    else:
        monkeypatch.delenv("PASN_TRAIN_ROWS_CONTIG", raising=False)


def _chunks(lib, n, S, cp, contig, multi):
    """The library's chunk count under the switch setting of this run (== the CPU replica); a multi-chunk case has a ragged last chunk."""
    chunks = lib.pasn_train_chunks(n, S, cp)
    assert chunks == tk.row_geom(n, S, cp, contig)["chunks"]
    if multi:
        assert chunks >= 2 and S % chunks != 0, (chunks, S)
    return chunks


def _nan_like(t):
    return torch.full_like(t, float("nan"))  # an output buffer: every element must have been written


def _pad_zero(t, c, name):
    if t.shape[-1] > c:
        assert float(t[..., c:].float().abs().max()) == 0.0, f"{name}: padded channels must stay zero"


@pytest.mark.parametrize("case,dtype,contig", _variants(tk.UNIT_CASES, UNIT_IDS))
def test_bn_unit_forward_backward(case, dtype, contig, monkeypatch):
    """stats -> affine+act forward; mode-0 reduce + apply backward; vs the fp64 gradient of relu(batch_norm(y) + residual).  The last three
    shapes cut every clip into two chunks with a ragged end (S = 147 / 1197 / 2883: rows past a chunk read as zeros, their stores are dropped),
    each in fp32 and bf16 and under both thread layouts of a block (PASN_TRAIN_ROWS_CONTIG)."""
    _rows_switch(monkeypatch, contig)
    lib = _lib.lib()
    c, shape, offset = case
    k = tk.unit_case(c, shape, offset, dtype)
    n, cp, S, code = k["n"], k["cp"], k["S"], _lib.dtype_code(dtype)
    yd, rd, dd = _cl(k["y"], dtype=dtype), _cl(k["res"], dtype=dtype), _cl(k["da"], dtype=dtype)
    chunks = _chunks(lib, n, S, cp, contig, case in tk.UNIT_MULTI_CHUNK)
    ws = torch.zeros(n * chunks * 2 * cp, device=DEV)
    stat, coef = torch.zeros(4 * cp, device=DEV), torch.zeros(2 * cp, device=DEV)
    gm, bt = k["gamma"].to(DEV), k["beta"].to(DEV)
    rmd, rvd = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    _lib.check(lib.pasn_bn_stats_fwd(yd.data_ptr(), ws.data_ptr(), gm.data_ptr(), bt.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), 0.1, 1e-5,
                                     stat.data_ptr(), 0, n, S, c, cp, code, _st()))
    a = _nan_like(yd)
    _lib.check(lib.pasn_affine_act_fwd(yd.data_ptr(), stat.data_ptr(), rd.data_ptr(), 0, a.data_ptr(), n, S, c, cp, 1, code, _st()))
    _rel(_ncl(a, c), k["out"], tk.tol_stores(1e-4, 1, dtype), "unit output")
    _pad_zero(a, c, "unit output")
    _rel(rmd, k["running_mean"], 1e-5, "running_mean")
    _rel(rvd, k["running_var"], 1e-4, "running_var")
    _rel(stat.view(4, cp)[0, :c], k["mean"][0], 1e-5, "batch mean")
    _rel(stat.view(4, cp)[1, :c], k["invstd"][0], 1e-4, "batch invstd")
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.pasn_unit_bwd_reduce(0, dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), rd.data_ptr(), 0, 0, ws.data_ptr(), coef.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), n, S, c, cp, 1, code, _st()))
    _rel(_ncl(dd, c), k["dres"], tk.tol_stores(1e-5, 1, dtype), "residual gradient")
    _pad_zero(dd, c, "residual gradient")
    dy = _nan_like(yd)
    _lib.check(lib.pasn_bn_bwd_apply(dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), coef.data_ptr(), dy.data_ptr(), n, S, c, cp, 0, code, _st()))
    _rel(dg, k["dgamma"], 1e-4, "dgamma")
    _rel(db, k["dbeta"], 1e-4, "dbeta")
    _rel(coef.view(2, cp)[:, :c], k["coef"][0], 1e-4, "coef")
    _rel(_ncl(dy, c), k["dy"], tk.tol_stores(2e-4, 2, dtype), "dy")  # behind the stored d' and its own store
    _pad_zero(dy, c, "dy")
    # mode 3 (sums only, d untouched) + apply differentiating on the fly == mode 0 + plain apply, for a unit without residual.
    # (Not for the large-mean case: u = y*sc + sh carries ~ulp(mean) of absolute error there, enough to flip one ReLU mask
    # against torch's (y - mean) * invstd form, and one flipped element shifts its whole channel's dy by d/R.)
    if offset != 0.0:
        return
    d2 = _cl(k["da"], dtype=dtype)
    keep = d2.clone()
    _lib.check(lib.pasn_unit_bwd_reduce(3, d2.data_ptr(), yd.data_ptr(), stat.data_ptr(), 0, 0, 0, ws.data_ptr(), coef.data_ptr(), dg.data_ptr(),
                                        db.data_ptr(), n, S, c, cp, 1, code, _st()))
    assert torch.equal(d2, keep), "mode 3 must not write d"
    _rel(dg, k["dgamma_plain"], 1e-4, "dgamma (no residual)")
    _rel(db, k["dbeta_plain"], 1e-4, "dbeta (no residual)")
    dy = _nan_like(yd)
    _lib.check(lib.pasn_bn_bwd_apply(d2.data_ptr(), yd.data_ptr(), stat.data_ptr(), coef.data_ptr(), dy.data_ptr(), n, S, c, cp, 1, code, _st()))
    _rel(_ncl(dy, c), k["dy_plain"], tk.tol_stores(2e-4, 1, dtype), "dy (lazy differentiation)")
    _pad_zero(dy, c, "dy (lazy differentiation)")


@pytest.mark.parametrize("case,dtype,contig", _variants(tk.GROUP_CASES, GROUP_IDS))
def test_bn_unit_statistics_groups(case, dtype, contig, monkeypatch):
    """The `_g` entry points: `groups` runs of N / groups clips, each normalised with its own batch statistics (stat [groups][4][Cp],
    coef [groups][2][Cp]), the running estimates updated group by group, dgamma / dbeta summed over the groups -- against the fp64 gradient of
    `groups` separate relu(batch_norm(.) + residual) calls on the sub-batches sharing gamma / beta / running buffers (what the reference's two
    trunk passes do to a norm layer).  The last shape: two chunks per clip, ragged."""
    _rows_switch(monkeypatch, contig)
    lib = _lib.lib()
    c, shape, groups = case
    k = tk.unit_case(c, shape, 0.0, dtype, groups)
    n, cp, S, code = k["n"], k["cp"], k["S"], _lib.dtype_code(dtype)
    yd, rd, dd = _cl(k["y"], dtype=dtype), _cl(k["res"], dtype=dtype), _cl(k["da"], dtype=dtype)
    chunks = _chunks(lib, n, S, cp, contig, case in tk.GROUP_MULTI_CHUNK)
    ws = torch.zeros(n * chunks * 2 * cp, device=DEV)
    stat, coef = torch.zeros(groups * 4 * cp, device=DEV), torch.zeros(groups * 2 * cp, device=DEV)
    gm, bt = k["gamma"].to(DEV), k["beta"].to(DEV)
    rmd, rvd = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    _lib.check(lib.pasn_bn_stats_fwd_g(yd.data_ptr(), ws.data_ptr(), gm.data_ptr(), bt.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), 0.1, 1e-5,
                                       stat.data_ptr(), 0, n, S, c, cp, code, groups, _st()))
    a = _nan_like(yd)
    _lib.check(lib.pasn_affine_act_fwd_g(yd.data_ptr(), stat.data_ptr(), rd.data_ptr(), 0, a.data_ptr(), n, S, c, cp, 1, code, groups, _st()))
    _rel(_ncl(a, c), k["out"], tk.tol_stores(1e-4, 1, dtype), "unit output")
    _pad_zero(a, c, "unit output")
    _rel(rmd, k["running_mean"], 1e-5, "running_mean after the groups' updates, in order")
    _rel(rvd, k["running_var"], 1e-4, "running_var")
    means = stat.view(groups, 4, cp)[:, 0, :c].cpu()
    for g in range(groups):
        _rel(means[g], k["mean"][g], 1e-5, f"mean of group {g}")
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.pasn_unit_bwd_reduce_g(0, dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), rd.data_ptr(), 0, 0, ws.data_ptr(), coef.data_ptr(),
                                          dg.data_ptr(), db.data_ptr(), n, S, c, cp, 1, code, groups, _st()))
    _rel(_ncl(dd, c), k["dres"], tk.tol_stores(1e-5, 1, dtype), "residual gradient")
    dy = _nan_like(yd)
    _lib.check(lib.pasn_bn_bwd_apply_g(dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), coef.data_ptr(), dy.data_ptr(), n, S, c, cp, 0, code, groups, _st()))
    _rel(dg, k["dgamma"], 1e-4, "dgamma (summed over the groups)")
    _rel(db, k["dbeta"], 1e-4, "dbeta")
    _rel(coef.view(groups, 2, cp)[:, :, :c], k["coef"], 1e-4, "coef of each group")
    _rel(_ncl(dy, c), k["dy"], tk.tol_stores(2e-4, 2, dtype), "dy")
    _pad_zero(dy, c, "dy")
    # an indivisible batch is refused
    assert lib.pasn_affine_act_fwd_g(yd.data_ptr(), stat.data_ptr(), 0, 0, a.data_ptr(), n, S, c, cp, 1, code, n + 1, _st()) != 0


@pytest.mark.parametrize("spec,dtype,contig", _variants(tk.SE_CASES, SE_IDS))
def test_se_unit_forward_backward(spec, dtype, contig, monkeypatch):
    """BN -> squeeze-excite gate -> Swish (X3D block with SE): forward and the three backward passes vs the fp64 gradient -- in fp32 and bf16,
    under both thread layouts, and at two shapes that cut a clip into two ragged chunks: bn_finalize's per-clip pool over several chunks,
    se_mlp_bwd folding the mode-4 partials into chunk 0, se_bn_coef, the `ok ? .. : 0` guards of modes 2 and 4."""
    _rows_switch(monkeypatch, contig)
    lib = _lib.lib()
    k = tk.se_case(*spec, dtype=dtype)
    n, c, cp, cse, S, code = k["n"], k["c"], k["cp"], k["cse"], k["S"], _lib.dtype_code(dtype)
    yd, dd = _cl(k["y"], dtype=dtype), _cl(k["da"], dtype=dtype)
    chunks = _chunks(lib, n, S, cp, contig, spec in tk.SE_MULTI_CHUNK)
    ws = torch.zeros(n * chunks * 2 * cp, device=DEV)
    stat, coef, pool_u, gated = (torch.zeros(m, device=DEV) for m in (4 * cp, 2 * cp, n * cp, n * cp))
    P = [t_.to(DEV).contiguous() for t_ in k["params"]]
    names = ("dgamma", "dbeta", "dw1", "db1", "dw2", "db2")
    labels = ("dgamma", "dbeta", "dfc1.w", "dfc1.b", "dfc2.w", "dfc2.b")
    _lib.check(lib.pasn_bn_stats_fwd(yd.data_ptr(), ws.data_ptr(), P[0].data_ptr(), P[1].data_ptr(), 0, 0, 0.1, 1e-5, stat.data_ptr(),
                                     pool_u.data_ptr(), n, S, c, cp, code, _st()))
    _rel(pool_u.view(n, cp)[:, :c], k["pool"], 1e-5, "per-clip pool of the normalised rows (summed over the chunks)")
    _lib.check(lib.pasn_se_gate_fwd(pool_u.data_ptr(), 1, 1, P[2].data_ptr(), P[3].data_ptr(), P[4].data_ptr(), P[5].data_ptr(),
                                    gated.data_ptr(), n, c, cp, cse, _st()))
    _rel(gated.view(n, cp)[:, :c], k["gate"], 1e-5, "gate")
    a = _nan_like(yd)
    _lib.check(lib.pasn_affine_act_fwd(yd.data_ptr(), stat.data_ptr(), 0, gated.data_ptr(), a.data_ptr(), n, S, c, cp, 3, code, _st()))
    _rel(_ncl(a, c), k["out"], tk.tol_stores(1e-4, 1, dtype), "unit output")
    _pad_zero(a, c, "unit output")
    add = torch.zeros(n * cp, device=DEV)
    pn = torch.zeros(lib.pasn_se_bwd_workspace_floats(n, c, cse), device=DEV)
    G = [torch.zeros_like(t_) for t_ in P]
    _lib.check(lib.pasn_unit_bwd_reduce(1, dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), 0, gated.data_ptr(), 0, ws.data_ptr(), 0, 0, 0, n, S, c,
                                        cp, 3, code, _st()))
    _rel(_ncl(dd, c), k["dv"], tk.tol_stores(2e-4, 1, dtype), "d' = d swish'(.)")
    _lib.check(lib.pasn_se_gate_bwd(ws.data_ptr(), pool_u.data_ptr(), P[2].data_ptr(), P[3].data_ptr(), P[4].data_ptr(), P[5].data_ptr(),
                                    add.data_ptr(), pn.data_ptr(), G[2].data_ptr(), G[3].data_ptr(), G[4].data_ptr(), G[5].data_ptr(), n, S, c, cp,
                                    cse, _st()))
    _rel(add.view(n, cp)[:, :c], k["add"], 2e-4, "add = dL/dpool / S")
    _lib.check(lib.pasn_unit_bwd_reduce(2, dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), 0, gated.data_ptr(), add.data_ptr(), ws.data_ptr(),
                                        coef.data_ptr(), G[0].data_ptr(), G[1].data_ptr(), n, S, c, cp, 3, code, _st()))
    _lib.check(lib.pasn_bn_bwd_apply(dd.data_ptr(), yd.data_ptr(), stat.data_ptr(), coef.data_ptr(), dd.data_ptr(), n, S, c, cp, 0, code, _st()))
    ref = k["two_pass"]  # (mode 2 sums the d' that mode 1 STORED: the reference rounds at the same store)
    for got, name, label in zip(G, names, labels):
        _rel(got, ref[name], 2e-4, label)
    _rel(_ncl(dd, c), ref["dy"], tk.tol_stores(2e-4, 3, dtype), "dy")  # behind the stored d', the stored d'' and its own store
    # the analytic form: ONE pass over (d, y) (mode 4), everything else from per-clip sums, d'' formed inside the apply pass
    d4 = _cl(k["da"], dtype=dtype)
    ws3 = torch.zeros(n * chunks * 3 * cp, device=DEV)
    add4, coef4 = torch.zeros(n * cp, device=DEV), torch.zeros(2 * cp, device=DEV)
    G4 = [torch.zeros_like(t_) for t_ in P]
    _lib.check(lib.pasn_unit_bwd_reduce(4, d4.data_ptr(), yd.data_ptr(), stat.data_ptr(), 0, gated.data_ptr(), 0, ws3.data_ptr(), 0, 0, 0, n, S, c,
                                        cp, 3, code, _st()))
    _lib.check(lib.pasn_se_gate_bwd_stat(ws3.data_ptr(), pool_u.data_ptr(), stat.data_ptr(), gated.data_ptr(), P[2].data_ptr(), P[3].data_ptr(),
                                         P[4].data_ptr(), P[5].data_ptr(), add4.data_ptr(), pn.data_ptr(), G4[2].data_ptr(), G4[3].data_ptr(),
                                         G4[4].data_ptr(), G4[5].data_ptr(), coef4.data_ptr(), G4[0].data_ptr(), G4[1].data_ptr(), n, S, c, cp, cse,
                                         _st()))
    _lib.check(lib.pasn_bn_bwd_apply_se(d4.data_ptr(), yd.data_ptr(), stat.data_ptr(), coef4.data_ptr(), gated.data_ptr(), add4.data_ptr(),
                                        d4.data_ptr(), n, S, c, cp, code, _st()))
    ref4 = k["analytic"]  # (mode 4 sums the unrounded d': autograd's sums)
    for got, name, label in zip(G4, names, labels):
        _rel(got, ref4[name], 2e-4, label + " (analytic)")
    if dtype == FP32:  # (in bf16 the two-pass sums see the rounded d', the analytic ones do not: each is held to its own reference)
        _rel(coef4.view(2, cp)[:, :c], coef.view(2, cp)[:, :c], 1e-4, "coef, analytic vs two passes")
    _rel(coef.view(2, cp)[:, :c], ref["coef"], 1e-4, "coef (two passes)")
    _rel(coef4.view(2, cp)[:, :c], ref4["coef"], 1e-4, "coef (analytic)")
    _rel(_ncl(d4, c), ref4["dy"], tk.tol_stores(2e-4, 2, dtype), "dy (analytic)")  # behind the stored d' and its own store
    _pad_zero(d4, c, "dy (analytic)")
    _pad_zero(dd, c, "dy")


WGRAD_CASES = [
    # cin, cout, k, s, p, (N,T,H,W)
    (24, 54, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 3, 9, 7)),
    (216, 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), (3, 2, 5, 5)),
    (24, 48, (1, 1, 1), (1, 2, 2), (0, 0, 0), (2, 2, 9, 9)),      # strided shortcut
    (20, 40, (3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 3, 7, 6)),      # windowed path
    (432, 192, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 4, 7, 7)),    # wide layers: 2 x 2 tile groups, several row partitions, ragged last step
    (192, 432, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 5, 7, 7)),
    (96, 216, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 9, 14, 14)),   # 7 / 3 tiles: half-empty last pairs
    # one case per remaining bf16 instance of the product build (WGRAD_BF16_INSTANCE below names them)
    (128, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 5, 7, 10)),   # 700 rows: two partitions of three 128-row steps, the last ragged
    (64, 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 3, 9, 7)),
    (96, 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 3, 9, 7)),
    (200, 24, (1, 1, 1), (1, 2, 2), (0, 0, 0), (2, 2, 9, 9)),
    # the regime of every real layer, a block walking several K steps: 43 200 rows is the smallest count at which the 333 partitions this
    # geometry asks for no longer hold a block to one 128-row step (256 rows per block, 192 in the last)
    (96, 96, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 6, 60, 60)),
    (64, 144, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 2, 70, 56)),   # 64 rows per block = two 32-row steps, 9 taps, borders on every side
]
# The instance pasn_conv3d_wgrad runs for each case in bf16 (pasn_conv3d_wgrad_variant; encoding: include/protoasnet_amd.h) and, where the
# case is about it, its row partitions.  pw_wgrad_bf16_kernel<32, 1> and <32, 8> are reachable only through the tuning build's PASN_WG_TPW.
WGRAD_BF16_INSTANCE = dict(zip(WGRAD_CASES, [
    (212801, None), (300102, None), (212801, None), (212801, None), (300102, None), (300201, None), (300201, None),
    (300101, 2), (212802, None), (212804, None), (203202, None), (212804, 169), (203204, 123)]))


def _assert_wgrad_instance(d, code, has_ws, variant, row_parts=None):
    """The library is about to launch the kernel instance the case names (the probe reads the route the launch reads)."""
    lib = _lib.lib()
    assert lib.pasn_conv3d_wgrad_variant(ctypes.byref(d), code, has_ws) == variant
    if row_parts is not None:
        assert lib.pasn_conv3d_wgrad_row_parts(ctypes.byref(d), code, has_ws) & 0xFFFFFFFF == row_parts


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,k,s,p,shape", WGRAD_CASES)
def test_conv_wgrad(cin, cout, k, s, p, shape, dtype):
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(n, cin, t, h, w, generator=g).to(dtype).float()
    wt = torch.zeros(cout, cin, *k, requires_grad=True)
    y = F.conv3d(x, wt, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(dy)
    d = _desc(x, y, k, s, p)
    xd, dyd = _cl(x, dtype=dtype), _cl(dy, dtype=dtype)
    dw = torch.zeros(cout, cin, k[0] * k[1] * k[2], device=DEV)
    if dtype == torch.bfloat16:
        _assert_wgrad_instance(d, BF16, 0, *WGRAD_BF16_INSTANCE[(cin, cout, k, s, p, shape)])
    else:  # conv_wgrad_kernel<float, PW>
        _assert_wgrad_instance(d, F32, 0, 100000 + (k == (1, 1, 1) and s == (1, 1, 1)))
    _lib.check(lib.pasn_conv3d_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), _lib.dtype_code(dtype), _st()))
    _rel(dw.view_as(wt), wt.grad, 1e-4, "dW")


WGRAD_HALO_CASES = [
    # cin, cout, k, p, (N,T,H,W) -- stride-1 "same" windowed convs of R(2+1)D-18 / ResNet-18 (wgrad_halo.hip, bf16)
    (64, 144, (1, 3, 3), (0, 1, 1), (2, 3, 10, 12)),    # spatial taps: 5 co tiles (two groups), 2 ci tiles, borders on every side
    (144, 64, (3, 1, 1), (1, 0, 0), (2, 5, 6, 6)),      # temporal taps: 5 ci tiles (three groups, the last one with a single tile)
    (45, 64, (3, 1, 1), (1, 0, 0), (1, 4, 9, 7)),       # 45 -> padded 48 channels, odd W (temporal taps do not care)
    (128, 288, (1, 3, 3), (0, 1, 1), (1, 2, 14, 14)),   # 9 co tiles = 3 groups, 4 ci tiles = 2 groups
    (64, 64, (1, 3, 3), (0, 1, 1), (3, 1, 28, 28)),     # ResNet-18 block conv (T = 1), several row partitions
    (64, 144, (1, 3, 3), (0, 1, 1), (1, 2, 20, 56)),    # W = 56 as in stage 1 of the 112 x 112 clip
    # the other six instances.  Temporal shape: 640 rows = two partitions, the clip boundary inside the ragged one
    (72, 128, (3, 1, 1), (1, 0, 0), (2, 5, 8, 8)),      # <3, 1>: what R(2+1)D's 230 -> 128 temporal convs run
    (16, 24, (3, 1, 1), (1, 0, 0), (2, 5, 8, 8)),
    (16, 24, (1, 3, 3), (0, 1, 1), (2, 3, 10, 12)),
    (24, 40, (1, 3, 3), (0, 1, 1), (2, 3, 10, 12)),
    (24, 96, (1, 3, 3), (0, 1, 1), (2, 3, 10, 12)),
    (64, 24, (1, 3, 3), (0, 1, 1), (2, 3, 10, 12)),
]
# conv_wgrad_halo_kernel<COT, PW> of each case: 400000 + 10000 * (temporal taps) + 100 COT + PW -- all nine instances
WGRAD_HALO_INSTANCE = dict(zip(WGRAD_HALO_CASES, [400303, 410201, 410201, 400303, 400203, 400303, 410301, 410101, 400102, 400202, 400302, 400103]))


@pytest.mark.parametrize("cin,cout,k,p,shape", WGRAD_HALO_CASES)
def test_conv_wgrad_halo(cin, cout, k, p, shape):
    """Windowed stride-1 weight gradient through the partial buffer (bf16): against autograd on the bf16-rounded operands, bitwise
    reproducible from run to run (no atomics), and the workspace query / NULL-workspace fallback of the entry point."""
    lib = _lib.lib()
    n, t, h, w = shape
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(cin + cout + w)
    x = torch.randn(n, cin, t, h, w, generator=g).to(dtype).float()
    wt = torch.zeros(cout, cin, *k, requires_grad=True)
    y = F.conv3d(x, wt, stride=1, padding=p)
    dy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(dy)
    d = _desc(x, y, k, (1, 1, 1), p)
    xd, dyd = _cl(x, dtype=dtype), _cl(dy, dtype=dtype)
    nbytes = int(lib.pasn_conv3d_wgrad_workspace_bytes(ctypes.byref(d), BF16))
    assert nbytes > 0, "this layer must take the partial-buffer path"
    assert int(lib.pasn_conv3d_wgrad_workspace_bytes(ctypes.byref(d), F32)) == 0
    _assert_wgrad_instance(d, BF16, 1, WGRAD_HALO_INSTANCE[(cin, cout, k, p, shape)])
    taps = k[0] * k[1] * k[2]
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)  # every value the reduce reads must have been written
        dw = torch.zeros(cout, cin, taps, device=DEV)
        _lib.check(lib.pasn_conv3d_wgrad_ws(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, ws.data_ptr(), _st()))
        torch.cuda.synchronize()
        outs.append(dw.clone())
    _rel(outs[0].view_as(wt), wt.grad, 1e-4, "dW (partial-buffer path)")
    assert torch.equal(outs[0], outs[1]), "the partial-buffer path has a fixed summation order"
    dw = torch.zeros(cout, cin, taps, device=DEV)
    _lib.check(lib.pasn_conv3d_wgrad_ws(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, 0, _st()))
    _rel(dw.view_as(wt), wt.grad, 1e-4, "dW (no workspace: the atomic path)")


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
def test_first_conv_wgrad(in_dtype):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 3, 17, 15, generator=g).to(in_dtype).float()
    wt = torch.zeros(24, 3, 1, 3, 3, requires_grad=True)
    y = F.conv3d(x, wt, stride=(1, 2, 2), padding=(0, 1, 1))
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    d = _desc(x, y, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    d.Cin_p = 3
    xd, dyd = x.to(DEV).to(in_dtype).contiguous(), _cl(dy)
    dw = torch.zeros(24, 27, device=DEV)
    _lib.check(lib.pasn_first_conv_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), _lib.dtype_code(in_dtype), F32, 0, _st()))
    _rel(dw.view_as(wt), wt.grad, 1e-4, "dW")
    # bf16 gradients: im2col rows + the LDS-transposed MFMA kernel (workspace given) == the gather kernel (no workspace)
    dyb = _cl(dy.bfloat16().float(), dtype=torch.bfloat16)
    wt2 = torch.zeros(24, 3, 1, 3, 3, requires_grad=True)
    F.conv3d(x.bfloat16().float(), wt2, stride=(1, 2, 2), padding=(0, 1, 1)).backward(dy.bfloat16().float())
    nbytes = lib.pasn_first_conv_wgrad_workspace_bytes(ctypes.byref(d), BF16)
    assert nbytes == 2 * 3 * 9 * 8 * 32 * 2
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for wsp in (ws.data_ptr(), 0):
        dw.zero_()
        _lib.check(lib.pasn_first_conv_wgrad(xd.data_ptr(), dyb.data_ptr(), dw.data_ptr(), ctypes.byref(d), _lib.dtype_code(in_dtype), BF16, wsp, _st()))
        _rel(dw.view_as(wt2), wt2.grad, 2e-3 if in_dtype == torch.float32 else 1e-4, "dW (bf16 dy)")


DW_DGRAD_CASES = [(54, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 3, 6, 7)), (54, (3, 3, 3), (1, 2, 2), (1, 1, 1), (2, 3, 9, 8)),
                  (24, (5, 1, 1), (1, 1, 1), (2, 0, 0), (2, 6, 4, 5)), (432, (3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 2, 5, 5))]


# the fp32 run carries the bare id of its case; bf16 (what training runs) is the dtype of the dgrad half only
@pytest.mark.parametrize("c,k,s,p,shape,dtype", [pytest.param(*case, dtype, id=f"{case[0]}-k{i}-s{i}-p{i}-shape{i}" + ("-bf16" if dtype == BF else ""))
                                                 for i, case in enumerate(DW_DGRAD_CASES) for dtype in (FP32, BF)])
def test_depthwise_dgrad_wgrad(c, k, s, p, shape, dtype):
    """dx in fp32 and bf16 (dw_dgrad_kernel, dw_dgrad_s2_kernel), dW in fp32, against autograd.  bf16: dy is rounded before the reference is
    taken, and dx is one fp32 accumulation of at most 27 products behind one bf16 store (tk.tol_stores)."""
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(c + k[0])
    x = torch.randn(n, c, t, h, w, generator=g).requires_grad_()
    wt = torch.randn(c, 1, *k, generator=g).requires_grad_()
    y = F.conv3d(x, wt, stride=s, padding=p, groups=c)
    dy = torch.randn(y.shape, generator=g)
    dyr = dy.to(dtype).float()
    (dx_ref,) = torch.autograd.grad(y, x, dyr, retain_graph=True)
    y.backward(dy)
    d = _desc(x, y, k, s, p)
    taps, cp = k[0] * k[1] * k[2], d.Cout_p
    wp = torch.zeros(taps, cp, device=DEV)
    wp[:, :c] = wt.detach().reshape(c, taps).t().to(DEV)
    xd, dyd, dyt = _cl(x.detach()), _cl(dy), _cl(dyr, dtype=dtype)
    dx = torch.empty_like(xd, dtype=dtype)
    _lib.check(lib.pasn_dwconv3d_dgrad(dyt.data_ptr(), wp.data_ptr(), dx.data_ptr(), ctypes.byref(d), _lib.dtype_code(dtype), _st()))
    _rel(_ncl(dx, c), dx_ref, tk.tol_stores(1e-5, 1, dtype), "dx")
    ws = torch.zeros(lib.pasn_dwconv3d_wgrad_workspace_floats(ctypes.byref(d)), device=DEV)
    dw = torch.zeros(c, taps, device=DEV)
    _lib.check(lib.pasn_dwconv3d_wgrad(xd.data_ptr(), dyd.data_ptr(), ws.data_ptr(), dw.data_ptr(), ctypes.byref(d), F32, _st()))
    _rel(dw.view_as(wt), wt.grad, 1e-4, "dW")


@pytest.mark.parametrize("c,s,shape,se", [(54, 1, (2, 5, 11, 13), True), (54, 2, (2, 4, 14, 18), False), (432, 1, (3, 9, 7, 7), True),
                                          (216, 2, (2, 3, 14, 14), False)])
def test_depthwise_stencil_with_fused_batch_statistics(c, s, shape, se, monkeypatch):
    """pasn_dwconv3d_stats_fwd (the stencil takes sum / sum of squares of its fp32 outputs per block; the finalize pass reads those
    partials): y identical to pasn_dwconv3d_fwd, the statistics table, the running estimates and the per-clip SE pool equal to
    pasn_bn_stats_fwd's on that y within fp32 / bf16-rounding noise, and to torch's batch_norm statistics of the fp32 conv output."""
    monkeypatch.setenv("PASN_DWMFMA", "0")  # the separate pass on the same (VALU) stencil
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(c + s)
    x = torch.randn(n, c, t, h, w, generator=g).bfloat16().float()
    wt = torch.randn(c, 1, 3, 3, 3, generator=g) * 0.3
    yref = F.conv3d(x, wt, stride=(1, s, s), padding=1, groups=c)
    d = _desc(x, yref, (3, 3, 3), (1, s, s), (1, 1, 1))
    cp, S = d.Cout_p, yref.shape[2] * yref.shape[3] * yref.shape[4]
    rows = lib.pasn_dwconv3d_stats_rows(ctypes.byref(d), BF16)
    assert rows > 0, "the T-marching stencil covers every X3D conv_b"
    wp = torch.zeros(27, cp, device=DEV)
    wp[:, :c] = wt.reshape(c, 27).t().to(DEV)
    one, zero = torch.ones(cp, device=DEV), torch.zeros(cp, device=DEV)
    gm, bt = (torch.rand(c, generator=g) + 0.5).to(DEV), torch.randn(c, generator=g).to(DEV)
    xd = _cl(x, dtype=torch.bfloat16)

    def run(fused):
        y = torch.empty(n, yref.shape[2], yref.shape[3], yref.shape[4], cp, dtype=torch.bfloat16, device=DEV)
        stat, pool = torch.zeros(4 * cp, device=DEV), torch.zeros(n * cp, device=DEV)
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        pu = pool.data_ptr() if se else 0
        if fused:
            ws = torch.zeros(n * rows * 2 * cp, device=DEV)
            _lib.check(lib.pasn_dwconv3d_stats_fwd(xd.data_ptr(), wp.data_ptr(), one.data_ptr(), zero.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                                   gm.data_ptr(), bt.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, stat.data_ptr(), pu,
                                                   ctypes.byref(d), BF16, _st()))
        else:
            ws = torch.zeros(n * lib.pasn_train_chunks(n, S, cp) * 2 * cp, device=DEV)
            _lib.check(lib.pasn_dwconv3d_fwd(xd.data_ptr(), wp.data_ptr(), one.data_ptr(), zero.data_ptr(), y.data_ptr(), 0, ctypes.byref(d), BF16, _st()))
            _lib.check(lib.pasn_bn_stats_fwd(y.data_ptr(), ws.data_ptr(), gm.data_ptr(), bt.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5,
                                             stat.data_ptr(), pu, n, S, c, cp, BF16, _st()))
        torch.cuda.synchronize()
        return y, stat.view(4, cp), pool.view(n, cp), rm, rv

    y1, st1, pl1, rm1, rv1 = run(True)
    y0, st0, pl0, rm0, rv0 = run(False)
    assert torch.equal(y1, y0), "the fused pass must write the same y"
    for i, name in enumerate(("mean", "invstd", "scale", "shift")):
        _rel(st1[i, :c], st0[i, :c], 2e-3, f"statistics table: {name} (fused vs separate)")
    _rel(rm1, rm0, 2e-3, "running_mean")
    _rel(rv1, rv0, 2e-3, "running_var")
    if se:
        _rel(pl1[:, :c], pl0[:, :c], 2e-3, "per-clip SE pool")
    # against torch on the fp32 conv output (the fused statistics never see the bf16 rounding of y)
    mean, var = yref.mean(dim=(0, 2, 3, 4)), yref.var(dim=(0, 2, 3, 4), unbiased=False)
    _rel(st1[0, :c], mean, 1e-4, "batch mean vs torch")
    _rel(st1[1, :c], 1.0 / torch.sqrt(var + 1e-5), 1e-4, "batch invstd vs torch")
    y2, st2, _, _, _ = run(True)
    assert torch.equal(st1, st2), "fixed summation order: bitwise reproducible statistics"


@pytest.mark.parametrize("stencil", ["matrix-core", "valu"])
@pytest.mark.parametrize("c,s,shape", [(54, 1, (2, 6, 14, 14)), (216, 1, (3, 5, 7, 7)), (108, 2, (2, 4, 14, 18))])
def test_stencil_statistics_are_shifted_by_the_running_mean(c, s, shape, stencil, monkeypatch):
    """The stencils' fused batch statistics take the moments of (y - k), k = the running mean as it stands before the step, so that
    sum (y - k)^2 does not cancel against the squared mean: with |mean| ~ 300 std and the running mean at the batch mean (a network a few
    steps into training) the inverse standard deviation matches torch's fp64 value to 2e-3; the same call from a running mean of zero
    (k = 0: what the first step sees, and what every step saw before round 3) is visibly worse.  Both the matrix-core stencil with the
    statistics epilogue (stride 1, default) and the VALU stencil (stride 2 / PASN_DWMFMA=0)."""
    if stencil == "valu":
        monkeypatch.setenv("PASN_DWMFMA", "0")
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(7 * c + s)
    x = (40.0 + 0.05 * torch.randn(n, c, t, h, w, generator=g)).bfloat16().float()
    wt = torch.rand(c, 1, 3, 3, 3, generator=g) * 0.2 + 0.05   # positive taps: |mean(y)| >> std(y) away from the borders
    if stencil == "matrix-core" and s == 1:
        wt = wt.bfloat16().float()  # the matrix-core stencil's weight operands are bf16 (as every other bf16 conv's)
    yref = F.conv3d(x.double(), wt.double(), stride=(1, s, s), padding=1, groups=c)
    d = _desc(x, yref, (3, 3, 3), (1, s, s), (1, 1, 1))
    cp = d.Cout_p
    rows = lib.pasn_dwconv3d_stats_rows(ctypes.byref(d), BF16)
    assert rows > 0
    wp = torch.zeros(27, cp, device=DEV)
    wp[:, :c] = wt.reshape(c, 27).t().to(DEV)
    one, zero = torch.ones(cp, device=DEV), torch.zeros(cp, device=DEV)
    gm, bt = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    xd = _cl(x, dtype=torch.bfloat16)
    mean = yref.mean(dim=(0, 2, 3, 4))
    invstd = 1.0 / torch.sqrt(yref.var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5)

    def run(rm0):
        y = torch.empty(n, yref.shape[2], yref.shape[3], yref.shape[4], cp, dtype=torch.bfloat16, device=DEV)
        stat = torch.zeros(4 * cp, device=DEV)
        rm, rv = rm0.clone().to(DEV), torch.ones(c, device=DEV)
        ws = torch.zeros(n * rows * 2 * cp, device=DEV)
        _lib.check(lib.pasn_dwconv3d_stats_fwd(xd.data_ptr(), wp.data_ptr(), one.data_ptr(), zero.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                               gm.data_ptr(), bt.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, stat.data_ptr(), 0,
                                               ctypes.byref(d), BF16, _st()))
        torch.cuda.synchronize()
        st = stat.view(4, cp).cpu().double()
        return st[0, :c], st[1, :c], rm.cpu().double()

    m1, i1, rm1 = run(mean.float())
    err_shifted = float(((i1 - invstd).abs() / invstd).max())
    assert float(((m1 - mean).abs() / mean.abs()).max()) < 1e-5
    assert err_shifted < 2e-3, err_shifted
    assert float(((rm1 - mean).abs() / mean.abs()).max()) < 1e-5      # 0.9 * mean + 0.1 * batch mean: the update reads the shift first
    _, i0, _ = run(torch.zeros(c))
    err_plain = float(((i0 - invstd).abs() / invstd).max())
    assert err_shifted < 0.5 * err_plain or err_plain < 2e-3, (err_shifted, err_plain)


@pytest.mark.parametrize("stencil", ["matrix-core", "valu"])
@pytest.mark.parametrize("c,s,shape", [(54, 1, (2, 6, 14, 14)), (108, 1, (2, 4, 7, 7)), (108, 2, (2, 4, 14, 18))])
def test_stencil_statistics_never_read_past_the_running_mean(c, s, shape, stencil, monkeypatch):
    """``running_mean`` holds C floats, the kernels' channel stride is Cp = round_up(C, 8) (54 -> 56, 108 -> 112): the shift of a padded
    channel is 0, never the bytes behind the buffer.  Here those bytes are NaN: the partial rows, the statistics table and the pooled
    means stay finite, and the real channels are bit-identical to a run whose running mean sits in a clean, padded buffer."""
    if stencil == "valu":
        monkeypatch.setenv("PASN_DWMFMA", "0")
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(11 * c + s)
    x = torch.randn(n, c, t, h, w, generator=g).bfloat16().float()
    wt = (torch.randn(c, 1, 3, 3, 3, generator=g) * 0.2).bfloat16().float()
    yref = F.conv3d(x, wt, stride=(1, s, s), padding=1, groups=c)
    d = _desc(x, yref, (3, 3, 3), (1, s, s), (1, 1, 1))
    cp = d.Cout_p
    assert cp > c
    rows = lib.pasn_dwconv3d_stats_rows(ctypes.byref(d), BF16)
    assert rows > 0
    wp = torch.zeros(27, cp, device=DEV)
    wp[:, :c] = wt.reshape(c, 27).t().to(DEV)
    one, zero = torch.ones(cp, device=DEV), torch.zeros(cp, device=DEV)
    gm, bt = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    xd = _cl(x, dtype=torch.bfloat16)
    rm0 = yref.mean(dim=(0, 2, 3, 4)) * 0.9

    def run(tail):
        buf = torch.full((c + 64,), tail, device=DEV)
        buf[:c] = rm0.to(DEV)
        rm, rv = buf[:c], torch.ones(c, device=DEV)
        y = torch.empty(n, yref.shape[2], yref.shape[3], yref.shape[4], cp, dtype=torch.bfloat16, device=DEV)
        stat = torch.zeros(4 * cp, device=DEV)
        pool = torch.zeros(n * cp, device=DEV)
        ws = torch.zeros(n * rows * 2 * cp, device=DEV)
        _lib.check(lib.pasn_dwconv3d_stats_fwd(xd.data_ptr(), wp.data_ptr(), one.data_ptr(), zero.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                               gm.data_ptr(), bt.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, stat.data_ptr(),
                                               pool.data_ptr(), ctypes.byref(d), BF16, _st()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[c:]).all()) or tail == 0.0   # the tail is only ever read, never written
        return ws.cpu(), stat.view(4, cp).cpu(), pool.view(n, cp).cpu(), buf[:c].cpu()

    ws_n, st_n, pool_n, rm_n = run(float("nan"))
    ws_c, st_c, pool_c, rm_c = run(0.0)
    for name, a in (("partial rows", ws_n), ("statistics", st_n), ("pooled means", pool_n), ("running mean", rm_n)):
        assert bool(torch.isfinite(a).all()), name
    assert torch.equal(ws_n, ws_c) and torch.equal(st_n, st_c) and torch.equal(pool_n, pool_c) and torch.equal(rm_n, rm_c)


@pytest.mark.parametrize("c,shape,act", [(54, (2, 5, 11, 13), "relu"), (432, (3, 9, 7, 7), "relu"), (108, (2, 4, 14, 28), "swish")])
def test_depthwise_dgrad_with_fused_backward_sums(c, shape, act, monkeypatch):
    """pasn_dwconv3d_dgrad_reduce (opt-in): dx identical to the stencil dgrad (pasn_dwconv3d_fwd with reversed taps), and coef / dgamma / dbeta
    equal to pasn_unit_bwd_reduce(mode 3) on (dx, y_prev) within the bf16 rounding of dx (the fused sums see the fp32 dx); then checked
    end to end against autograd of  conv_dw(act(batch_norm(y_prev)))."""
    monkeypatch.setenv("PASN_DW_DGRAD_REDUCE", "1")
    monkeypatch.setenv("PASN_DWMFMA", "0")  # the separate pass on the same (VALU) stencil
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(c)
    actc = _lib.ACT[act]
    fn = {"relu": F.relu, "swish": lambda v: v * torch.sigmoid(v)}[act]
    yp = (torch.randn(n, c, t, h, w, generator=g) * 1.5 + 0.3).bfloat16().float().requires_grad_()
    gamma = (torch.rand(c, generator=g) + 0.5).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.5).requires_grad_()
    wt = torch.randn(c, 1, 3, 3, 3, generator=g) * 0.3
    a = fn(F.batch_norm(yp, None, None, gamma, beta, True, 0.1, 1e-5))
    out = F.conv3d(a, wt, padding=1, groups=c)
    dy = torch.randn(out.shape, generator=g).bfloat16().float()
    out.backward(dy)
    d = _desc(a, out, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    cp, S = d.Cout_p, t * h * w
    rows = lib.pasn_dwconv3d_dgrad_reduce_rows(ctypes.byref(d), BF16)
    assert rows > 0
    wflip = torch.zeros(27, cp, device=DEV)
    wflip[:, :c] = wt.reshape(c, 27).flip(1).t().to(DEV)
    one, zero = torch.ones(cp, device=DEV), torch.zeros(cp, device=DEV)
    ypd, dyd = _cl(yp.detach(), dtype=torch.bfloat16), _cl(dy, dtype=torch.bfloat16)
    gm, bt = gamma.detach().to(DEV), beta.detach().to(DEV)
    stat = torch.zeros(4 * cp, device=DEV)
    ws0 = torch.zeros(n * lib.pasn_train_chunks(n, S, cp) * 2 * cp, device=DEV)
    _lib.check(lib.pasn_bn_stats_fwd(ypd.data_ptr(), ws0.data_ptr(), gm.data_ptr(), bt.data_ptr(), 0, 0, 0.1, 1e-5, stat.data_ptr(), 0, n, S, c, cp,
                                     BF16, _st()))
    # separate: stencil dgrad, then the reduce pass
    dx0 = torch.empty_like(ypd)
    _lib.check(lib.pasn_dwconv3d_fwd(dyd.data_ptr(), wflip.data_ptr(), one.data_ptr(), zero.data_ptr(), dx0.data_ptr(), 0, ctypes.byref(d), BF16, _st()))
    coef0, dg0, db0 = torch.zeros(2 * cp, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.pasn_unit_bwd_reduce(3, dx0.data_ptr(), ypd.data_ptr(), stat.data_ptr(), 0, 0, 0, ws0.data_ptr(), coef0.data_ptr(), dg0.data_ptr(),
                                        db0.data_ptr(), n, S, c, cp, actc, BF16, _st()))
    # fused
    dx1 = torch.empty_like(ypd)
    ws1 = torch.zeros(n * rows * 2 * cp, device=DEV)
    coef1, dg1, db1 = torch.zeros(2 * cp, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    _lib.check(lib.pasn_dwconv3d_dgrad_reduce(dyd.data_ptr(), wflip.data_ptr(), one.data_ptr(), zero.data_ptr(), dx1.data_ptr(), ypd.data_ptr(),
                                              stat.data_ptr(), actc, ws1.data_ptr(), coef1.data_ptr(), dg1.data_ptr(), db1.data_ptr(),
                                              ctypes.byref(d), BF16, _st()))
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx0), "the fused pass must write the same dx"
    _rel(coef1.view(2, cp)[:, :c], coef0.view(2, cp)[:, :c], 4e-3, "coef (fused vs separate)")
    _rel(dg1, dg0, 4e-3, "dgamma (fused vs separate)")
    _rel(db1, db0, 4e-3, "dbeta (fused vs separate)")
    _rel(dg1, gamma.grad, 1e-2, "dgamma vs autograd")
    _rel(db1, beta.grad, 1e-2, "dbeta vs autograd")
    dyp = torch.empty_like(ypd)
    _lib.check(lib.pasn_bn_bwd_apply(dx1.data_ptr(), ypd.data_ptr(), stat.data_ptr(), coef1.data_ptr(), dyp.data_ptr(), n, S, c, cp, actc, BF16, _st()))
    _rel(_ncl(dyp, c), yp.grad, 2e-2, "gradient of the producer's raw output vs autograd")


WGRAD_GATHER_CASES = [
    # cin, cout, k, s, p, (N,T,H,W) -- windowed / strided convs outside the halo kernel (conv_wgrad_gather_kernel, bf16)
    (64, 230, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 3, 12, 14)),   # R(2+1)D stage transition, spatial
    (230, 128, (3, 1, 1), (2, 1, 1), (1, 0, 0), (2, 6, 7, 7)),    # ... temporal, stride 2 in T
    (24, 48, (1, 1, 1), (1, 2, 2), (0, 0, 0), (2, 2, 9, 9)),      # strided shortcut
    (20, 40, (3, 3, 3), (1, 2, 2), (1, 1, 1), (1, 3, 7, 6)),      # 27 taps
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 2, 6, 7)),      # stride 1 but odd W: not the halo kernel's
]


@pytest.mark.parametrize("cin,cout,k,s,p,shape", WGRAD_GATHER_CASES)
def test_conv_wgrad_gather(cin, cout, k, s, p, shape):
    """Gathered tile weight gradient through the partial buffer (bf16): against autograd, bitwise reproducible."""
    lib = _lib.lib()
    n, t, h, w = shape
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(cin + cout + w)
    x = torch.randn(n, cin, t, h, w, generator=g).to(dtype).float()
    wt = torch.zeros(cout, cin, *k, requires_grad=True)
    y = F.conv3d(x, wt, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(dy)
    d = _desc(x, y, k, s, p)
    xd, dyd = _cl(x, dtype=dtype), _cl(dy, dtype=dtype)
    nbytes = int(lib.pasn_conv3d_wgrad_workspace_bytes(ctypes.byref(d), BF16))
    assert nbytes > 0
    _assert_wgrad_instance(d, BF16, 1, 500000)  # conv_wgrad_gather_kernel
    taps = k[0] * k[1] * k[2]
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
        dw = torch.zeros(cout, cin, taps, device=DEV)
        _lib.check(lib.pasn_conv3d_wgrad_ws(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, ws.data_ptr(), _st()))
        torch.cuda.synchronize()
        outs.append(dw.clone())
    _rel(outs[0].view_as(wt), wt.grad, 1e-4, "dW (gathered tiles, partial buffer)")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("c,s,shape", [(54, 1, (2, 5, 9, 10)), (54, 2, (2, 4, 12, 14)), (432, 1, (1, 3, 7, 7)), (108, 2, (1, 16, 8, 9)), (216, 1, (2, 1, 5, 4))])
def test_depthwise_wgrad_march_bf16(c, s, shape, monkeypatch):
    """T-marching depthwise 3x3x3 weight gradient (bf16): against autograd on the bf16-rounded operands and against the strip kernel it
    replaces; T = 1 (both neighbour frames out of the clip), ragged strips, stride 2, odd widths."""
    lib = _lib.lib()
    n, t, h, w = shape
    g = torch.Generator().manual_seed(c + s + w)
    x = torch.randn(n, c, t, h, w, generator=g).bfloat16().float()
    wt = torch.zeros(c, 1, 3, 3, 3, requires_grad=True)
    y = F.conv3d(x, wt, stride=(1, s, s), padding=1, groups=c)
    dy = torch.randn(y.shape, generator=g).bfloat16().float()
    y.backward(dy)
    d = _desc(x, y, (3, 3, 3), (1, s, s), (1, 1, 1))
    xd, dyd = _cl(x, dtype=torch.bfloat16), _cl(dy, dtype=torch.bfloat16)
    outs = []
    # round 4's marching kernel (4 channels per thread, strips of 2), its 2-channel and 3-wide instances, round 2's marching kernel, the strip kernel
    arms = ({}, {"PASN_DWWG_CH": "2"}, {"PASN_DWWG_WT": "3"}, {"PASN_DWWG_CH": "2", "PASN_DWWG_WT": "3"}, {"PASN_DWWG_MARCH2": "0"}, {"PASN_NO_DWWG_MARCH": "1"})
    for env in arms:
        for k in ("PASN_DWWG_CH", "PASN_DWWG_WT", "PASN_DWWG_MARCH2", "PASN_NO_DWWG_MARCH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ws = torch.full((int(lib.pasn_dwconv3d_wgrad_workspace_floats(ctypes.byref(d))),), float("nan"), device=DEV)
        dw = torch.zeros(c, 27, device=DEV)
        _lib.check(lib.pasn_dwconv3d_wgrad(xd.data_ptr(), dyd.data_ptr(), ws.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, _st()))
        torch.cuda.synchronize()
        _rel(dw.view_as(wt), wt.grad, 1e-4, f"dW ({env})")
        outs.append(dw)
    for o in outs[:-1]:
        _rel(o, outs[-1], 1e-5, "marching vs strip kernel")


_S1, _S2 = ((3, 3, 3), 1, (1, 3, 9, 10)), ((3, 3, 3), 2, (1, 3, 12, 14))
_MARCH1, _NO_MARCH, _NO_STRIP = {"PASN_DWWG_MARCH2": "0"}, {"PASN_NO_DWWG_MARCH": "1"}, {"PASN_NO_DWWG_STRIP": "1"}
_FUSED, _FUSED_NO_MARCH = {"PASN_DWWG_FUSED": "1"}, {"PASN_DWWG_FUSED": "1", "PASN_NO_DWWG_MARCH": "1"}
# (arm of pasn_dwconv3d_wgrad's ladder, dtype, (window, spatial stride, (n, t, h, w)), switches): every arm once, 24 channels (6 lanes of 4
# padded to 8), ragged strips (widths 10 and 7 at 3 and 2 outputs per strip), T = 3 (both temporal borders and an interior frame).
# strip-fused: the four strip instances with all three temporal taps in one pass; generic-313: neither the temporal nor the strip arm takes
# a (3,1,3) window, so the row-partial kernel runs with 3 of its 9 spatial taps live.
DW_WGRAD_ARMS = [
    ("temporal", FP32, ((3, 1, 1), 1, (1, 4, 5, 6)), {}), ("temporal", BF, ((3, 1, 1), 1, (1, 4, 5, 6)), {}),
    ("march2", BF, _S1, {}), ("march2", BF, _S2, {}), ("march2-ch2-wt3", BF, _S1, {"PASN_DWWG_CH": "2", "PASN_DWWG_WT": "3"}),
    ("march", BF, _S1, _MARCH1), ("march", BF, _S2, _MARCH1),
    ("strip", FP32, _S1, {}), ("strip", FP32, _S2, {}), ("strip", BF, _S1, _NO_MARCH), ("strip", BF, _S2, _NO_MARCH),
    ("strip-133", FP32, ((1, 3, 3), 1, (1, 2, 9, 10)), {}),
    ("generic", FP32, _S1, _NO_STRIP), ("generic", BF, _S1, _NO_STRIP),
    ("strip-fused", FP32, _S1, _FUSED), ("strip-fused", FP32, _S2, _FUSED), ("strip-fused", BF, _S1, _FUSED_NO_MARCH), ("strip-fused", BF, _S2, _FUSED_NO_MARCH),
    ("generic-313", FP32, ((3, 1, 3), 1, (1, 3, 5, 6)), {}),
]


@pytest.mark.parametrize("arm,dtype,geom,env", DW_WGRAD_ARMS,
                         ids=[f"{a}-{'bf16' if t == BF else 'fp32'}-s{g[1]}" for a, t, g, _ in DW_WGRAD_ARMS])
def test_depthwise_wgrad_stays_inside_its_workspace(arm, dtype, geom, env):
    """The partial buffer of pasn_dwconv3d_wgrad is sized by pasn_dwconv3d_wgrad_workspace_floats without knowing the dtype, and the
    launch is not told its size: on every arm of the ladder the launch must stay inside it.  The buffer is followed, in the same
    allocation, by a guard of 4096 floats that must come back bit-identical; the workspace itself starts as NaN (a row that is read but
    was not written shows in dW), and dW matches autograd on the (bf16-rounded) operands."""
    lib = _lib.lib()
    k, s, (n, t, h, w) = geom
    c, p = 24, tuple(e // 2 for e in k)
    g = torch.Generator().manual_seed(sum(k) + s + w)
    x, wt = torch.randn(n, c, t, h, w, generator=g).to(dtype).float(), torch.zeros(c, 1, *k, requires_grad=True)
    y = F.conv3d(x, wt, stride=(1, s, s), padding=p, groups=c)
    dy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(dy)
    d = _desc(x, y, k, (1, s, s), p)
    xd, dyd = _cl(x, dtype=dtype), _cl(dy, dtype=dtype)
    taps, guard = k[0] * k[1] * k[2], 4096
    ambient = dict.fromkeys(("PASN_DWWG_CH", "PASN_DWWG_WT", "PASN_DWWG_MARCH2", "PASN_DWWG_BLOCKS", "PASN_DWWG_FUSED", "PASN_NO_DWWG_MARCH", "PASN_NO_DWWG_STRIP"))
    with _lib.tuning_env(**dict(ambient, **env)):  # only this case's switches choose the arm
        floats = int(lib.pasn_dwconv3d_wgrad_workspace_floats(ctypes.byref(d)))
        assert floats > 0
        buf = torch.full((floats + guard,), float("nan"), device=DEV)
        buf[floats:] = -12345.0
        sentinel = buf[floats:].clone()
        dw = torch.zeros(c, taps, device=DEV)
        _lib.check(lib.pasn_dwconv3d_wgrad(xd.data_ptr(), dyd.data_ptr(), buf.data_ptr(), dw.data_ptr(), ctypes.byref(d), _lib.dtype_code(dtype), _st()))
        torch.cuda.synchronize()
    assert torch.equal(buf[floats:].view(torch.int32), sentinel.view(torch.int32)), f"{arm}: the launch wrote past its {floats}-float workspace"
    _rel(dw.view_as(wt), wt.grad, 1e-4, f"dW ({arm})")


@pytest.mark.parametrize("layer", ["c133_64_144", "c311_144_64", "c133_s2_64_230", "dw_54"])
def test_weight_gradient_kernels_at_full_benchmark_shapes(layer, monkeypatch):
    """Round-2 weight-gradient kernels at the full R(2+1)D-18 / X3D-S benchmark shapes (no CPU oracle finishes there in seconds): each
    must agree with the kernel it replaces (same operands, another summation order) and be bitwise reproducible."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(9)
    if layer == "dw_54":
        n, c, t, h, w = 32, 54, 16, 56, 56
        d = ConvDesc(N=n, Ti=t, Hi=h, Wi=w, Cin=c, Cin_p=56, To=t, Ho=h, Wo=w, Cout=c, Cout_p=56, kt=3, kh=3, kw=3, st=1, sh=1, sw=1, pt=1, ph=1, pw=1)
        xd = torch.randn(n, t, h, w, 56, generator=g).bfloat16().to(DEV)
        dyd = torch.randn(n, t, h, w, 56, generator=g).bfloat16().to(DEV)
        xd[..., c:] = 0
        dyd[..., c:] = 0
        outs = {}
        for tag, env in (("march", "0"), ("march_again", "0"), ("strip", "1")):
            monkeypatch.setenv("PASN_NO_DWWG_MARCH", env)
            ws = torch.empty(int(lib.pasn_dwconv3d_wgrad_workspace_floats(ctypes.byref(d))), device=DEV)
            dw = torch.zeros(c, 27, device=DEV)
            _lib.check(lib.pasn_dwconv3d_wgrad(xd.data_ptr(), dyd.data_ptr(), ws.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, _st()))
            torch.cuda.synchronize()
            outs[tag] = dw
        assert torch.equal(outs["march"], outs["march_again"])  # bitwise reproducible
        _rel(outs["march"], outs["strip"], 2e-4, "marching vs strip depthwise dW at 32x16x56x56")
        return
    cin, cout, k, s_, p, shape = {"c133_64_144": (64, 144, (1, 3, 3), (1, 1, 1), (0, 1, 1), (8, 32, 56, 56)),
                                  "c311_144_64": (144, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (8, 32, 56, 56)),
                                  "c133_s2_64_230": (64, 230, (1, 3, 3), (1, 2, 2), (0, 1, 1), (8, 32, 56, 56))}[layer]
    n, t, h, w = shape
    to, ho, wo = (t + 2 * p[0] - k[0]) // s_[0] + 1, (h + 2 * p[1] - k[1]) // s_[1] + 1, (w + 2 * p[2] - k[2]) // s_[2] + 1
    cinp, coutp = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
    d = ConvDesc(N=n, Ti=t, Hi=h, Wi=w, Cin=cin, Cin_p=cinp, To=to, Ho=ho, Wo=wo, Cout=cout, Cout_p=coutp, kt=k[0], kh=k[1], kw=k[2],
                 st=s_[0], sh=s_[1], sw=s_[2], pt=p[0], ph=p[1], pw=p[2])
    xd = torch.randn(n, t, h, w, cinp, generator=g).bfloat16().to(DEV)
    dyd = torch.randn(n, to, ho, wo, coutp, generator=g).bfloat16().to(DEV)
    xd[..., cin:] = 0
    dyd[..., cout:] = 0
    taps = k[0] * k[1] * k[2]
    nbytes = int(lib.pasn_conv3d_wgrad_workspace_bytes(ctypes.byref(d), BF16))
    assert nbytes > 0
    outs = []
    for wsp in (True, True, False):
        ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
        dw = torch.zeros(cout, cin, taps, device=DEV)
        _lib.check(lib.pasn_conv3d_wgrad_ws(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), ctypes.byref(d), BF16, ws.data_ptr() if wsp else 0, _st()))
        torch.cuda.synchronize()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), "partial-buffer path: fixed summation order"
    _rel(outs[0], outs[2], 2e-4, f"{layer}: partial-buffer kernel vs the atomic per-tap kernel")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_weights_one_launch(dtype):
    """The native weight packer (one launch for all conv weights of a step) against the torch expressions it replaces, BIT-EXACT: dense
    forward and input-gradient layouts (padded [row][tap][k]; 27 / 9 / 3 / 1 taps; transposed with reversed taps), the fragment-major
    layout of the x-tile pointwise kernels, the depthwise [tap][Cp] layouts (plain and reversed), destinations that span several blocks
    and ones smaller than a block, channel counts that are not multiples of the paddings -- all in the same table."""
    from protoasnet_amd.plan import round_up
    from protoasnet_amd.train import build_pack_tables

    torch.manual_seed(5)
    kstep, ch = (16, 8) if dtype == torch.bfloat16 else (8, 4)
    jobs, want = [], []

    def dense(cout, cin, k, mode, frag):
        taps = k[0] * k[1] * k[2]
        w = torch.randn(cout, cin, *k, device=DEV)
        dc, di = (cout, cin) if mode == 0 else (cin, cout)  # the packed conv's (rows, k) extents
        kc, rows = round_up(round_up(di, 8), kstep), round_up(round_up(dc, 8), 128)
        wp = torch.zeros(rows, taps, kc, dtype=dtype, device=DEV)
        src = w if mode == 0 else w.transpose(0, 1).flip(2, 3, 4)
        wp[:dc, :, :di] = src.reshape(dc, di, taps).permute(0, 2, 1)
        ref = wp
        if frag:
            ref = torch.empty_like(wp)
            ref.view(rows // 32, kc // kstep, 2, 32, ch).copy_(wp.view(rows // 32, 32, kc // kstep, 2, ch).permute(0, 2, 3, 1, 4))
        dst = torch.full_like(wp, float("nan"))  # every element must be written
        jobs.append((w, dst, mode, cout, cin, taps, rows, kc, int(frag), kstep, ch))
        want.append(ref)

    def depthwise(c, k, flip):
        taps = k[0] * k[1] * k[2]
        cp = round_up(c, 8)
        w = torch.randn(c, 1, *k, device=DEV)
        ref = torch.zeros(taps, cp, device=DEV)
        ref[:, :c] = (w.reshape(c, taps).flip(1) if flip else w.reshape(c, taps)).t()
        dst = torch.full_like(ref, float("nan"))
        jobs.append((w, dst, 3 if flip else 2, c, 1, taps, taps, cp, 0, 0, 0))
        want.append(ref)

    dense(54, 24, (1, 1, 1), 0, False)
    dense(54, 24, (1, 1, 1), 0, True)
    dense(54, 24, (1, 1, 1), 1, False)
    dense(432, 192, (1, 1, 1), 1, True)
    dense(144, 64, (1, 3, 3), 0, False)
    dense(144, 64, (1, 3, 3), 1, False)
    dense(64, 45, (3, 1, 1), 1, False)
    dense(20, 12, (3, 3, 3), 0, False)
    dense(20, 12, (3, 3, 3), 1, False)
    dense(3, 5, (1, 1, 1), 0, False)
    depthwise(54, (3, 3, 3), False)
    depthwise(54, (3, 3, 3), True)
    depthwise(24, (5, 1, 1), True)
    depthwise(432, (3, 3, 3), False)
    tables = build_pack_tables(jobs, torch.device(DEV))
    tj, bj, bc, nb = tables
    assert nb == sum((j[1].numel() + 2047) // 2048 for j in jobs)
    _lib.check(_lib.lib().pasn_pack_weights(tj.data_ptr(), bj.data_ptr(), bc.data_ptr(), nb, _lib.current_stream()))
    torch.cuda.synchronize()
    for i, (job, ref) in enumerate(zip(jobs, want)):
        assert torch.equal(job[1], ref), f"job {i}: mode {job[2]} cout {job[3]} cin {job[4]} taps {job[5]} frag {job[8]}"


def test_scatter_strided_and_add():
    """fp32 and bf16; the stride-(1,2,2) shortcut scatter, and the zero-insertion use of _bwd_dense_dgrad: a temporal stride into an extent
    larger than (To - 1) * st + 1, whose trailing planes / rows / columns must be zeroed; Cp = 16 and 24.  Overwrite is exact; accumulate is
    exact in fp32 and within one rounding (2^-8 of the element) in bf16."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(5)
    for dtype in (FP32, BF):
        code = _lib.dtype_code(dtype)
        for cp, (to, ho, wo), (ti, hi, wi), (st, sh, sw) in [(16, (2, 4, 5), (2, 8, 9), (1, 2, 2)), (24, (2, 3, 4), (5, 7, 8), (2, 2, 2)),
                                                             (16, (3, 2, 2), (6, 4, 5), (2, 2, 2))]:
            src = torch.randn(2, to, ho, wo, cp, generator=g).to(dtype).to(DEV)
            dst = torch.randn(2, ti, hi, wi, cp, generator=g).to(dtype).to(DEV)
            d = ConvDesc(N=2, Ti=ti, Hi=hi, Wi=wi, Cin=cp, Cin_p=cp, To=to, Ho=ho, Wo=wo, Cout=cp, Cout_p=cp, kt=1, kh=1, kw=1, st=st, sh=sh, sw=sw)
            ref = dst.double()
            ref[:, ::st, ::sh, ::sw][:, :to, :ho, :wo] += src.double()
            _lib.check(lib.pasn_scatter_strided(src.data_ptr(), dst.data_ptr(), ctypes.byref(d), 1, code, _st()))
            if dtype == FP32:
                assert torch.equal(dst, ref.float())
            else:
                assert_close(dst, ref, 0.0, tk.BF16_STORE, "accumulate: the sum, rounded once to bf16")
            _lib.check(lib.pasn_scatter_strided(src.data_ptr(), dst.data_ptr(), ctypes.byref(d), 0, code, _st()))
            ref = torch.zeros_like(dst)
            ref[:, ::st, ::sh, ::sw][:, :to, :ho, :wo] = src
            assert torch.equal(dst, ref), "overwrite: the source values on the strided lattice, zeros everywhere else"
        a, b = torch.randn(4096 + 8, generator=g).to(dtype).to(DEV), torch.randn(4096 + 8, generator=g).to(dtype).to(DEV)
        want = a.double() + b.double()
        _lib.check(lib.pasn_add_inplace(a.data_ptr(), b.data_ptr(), 4096 + 8, code, _st()))
        if dtype == FP32:
            assert torch.equal(a, want.float())
        else:
            assert_close(a, want, 0.0, tk.BF16_STORE, "a + b, rounded once to bf16")


@pytest.mark.parametrize("i,occ_only,dtype", [pytest.param(0, False, FP32, id="False"), pytest.param(0, True, FP32, id="True")]
                         + [pytest.param(i, o, dt, id=f"case{i}-{'occ_only' if o else 'full'}-{'bf16' if dt == BF else 'fp32'}")
                            for i in (0, 1) for o in (False, True) for dt in (FP32, BF) if (i, dt) != (0, FP32)])
def test_xproto_tail_forward_backward(i, occ_only, dtype):
    """Head B's tail against fp64 autograd.  Case 1: D = 12 in rows of Dp = 16, P = 30 in rows of Pp = 32, S = 300 (19 row tiles of the pool
    kernels, the last one ragged).  bf16: z, r, dz, dr in bf16 -- the forward outputs and the parameter gradients are fp32 sums over the
    rounded operands (fp32 bounds), dz and dr are stored once."""
    lib = _lib.lib()
    k = tk.xproto_case(i, occ_only, dtype)
    n, s, dch, dp, p, pp, kk, code = k["n"], k["S"], k["D"], k["Dp"], k["P"], k["Pp"], k["K"], _lib.dtype_code(dtype)
    zd = torch.zeros(n, s, dp, dtype=dtype, device=DEV)
    zd[..., :dch] = k["z"].permute(0, 2, 1)
    rd = torch.zeros(n, s, pp, dtype=dtype, device=DEV)
    rd[..., :p] = k["r"].permute(0, 2, 1)
    d = XProtoDesc(N=n, S=s, Cb=0, Cbp=0, D=dch, Dp=dp, Hd=dch // 2, Hp=(dch // 2 + 7) // 8 * 8, P=p, Pp=pp, K=kk, mode=int(occ_only))
    pv, fw = k["protos"].to(DEV), k["fcw"].to(DEV)
    o_occ, o_feat, o_sim, o_log = (torch.zeros(sh, device=DEV) for sh in ((n, p, s), (n, p, dch), (n, p), (n, kk)))
    zp = 0 if occ_only else zd.data_ptr()
    _lib.check(lib.pasn_xproto_tail_fwd(zp, rd.data_ptr(), pv.data_ptr(), fw.data_ptr(), o_occ.data_ptr(), o_feat.data_ptr(), o_sim.data_ptr(),
                                        o_log.data_ptr(), ctypes.byref(d), code, _st()))
    _rel(o_occ, k["occ"], 1e-6, "occ")
    if not occ_only:
        _rel(o_feat, k["feat"], 1e-5, "feat")
        _rel(o_sim, k["sim"], 1e-5, "sim")
        _rel(o_log, k["logits"], 1e-5, "logits")
    dz, dr = _nan_like(zd), _nan_like(rd)
    dfeat, dpv, dfw = torch.zeros(n, p, dch, device=DEV), torch.zeros_like(pv), torch.zeros_like(fw)
    gl, gs, go = k["dl"].to(DEV), k["dsm"].to(DEV), k["doc"].to(DEV).contiguous()
    _lib.check(lib.pasn_xproto_tail_bwd(zp, rd.data_ptr(), pv.data_ptr(), fw.data_ptr(), o_feat.data_ptr(), o_sim.data_ptr(), gl.data_ptr(),
                                        0 if occ_only else gs.data_ptr(), go.data_ptr(), dfeat.data_ptr(), dz.data_ptr(), dr.data_ptr(),
                                        dpv.data_ptr(), dfw.data_ptr(), ctypes.byref(d), code, _st()))
    _rel(dr[..., :p].permute(0, 2, 1), k["dr"], tk.tol_stores(1e-4, 1, dtype), "dr")
    _pad_zero(dr, p, "dr")
    if not occ_only:
        _rel(dz[..., :dch].permute(0, 2, 1), k["dz"], tk.tol_stores(1e-4, 1, dtype), "dz")
        _pad_zero(dz, dch, "dz")
        _rel(dpv, k["dprotos"], 1e-4, "dprototypes")
        _rel(dfw, k["dfcw"], 1e-4, "dlast_layer")


@pytest.mark.parametrize("dtype", [FP32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(tk.MAXPOOL_CASES)))
def test_maxpool_forward_backward_with_tied_windows(i, dtype):
    """pasn_maxpool3d_fwd / _bwd called directly against F.max_pool3d and its autograd (fp64, on the rounded input), on post-ReLU inputs: a
    quarter to two thirds of the windows have a tied (zero) maximum, one channel group is all zeros, a bf16 plane holds four values.  The
    window's gradient goes to its FIRST maximum in scan order -- in a padded border window that is the first in-range slot.  dx is a sum of
    at most 8 routed dy values per element (fp32: 1e-5; bf16: one store on top), and every window routes to exactly one element, so
    the sums of dx and dy agree per (clip, channel)."""
    lib = _lib.lib()
    k = tk.maxpool_case(i, dtype)
    n, c, cp, code = k["n"], k["c"], k["cp"], _lib.dtype_code(dtype)
    d = _desc(k["x"], k["y"], k["k"], k["s"], k["p"])
    xd, dyd = _cl(k["x"], dtype=dtype), _cl(k["dy"], dtype=dtype)
    yd = _nan_like(dyd)
    _lib.check(lib.pasn_maxpool3d_fwd(xd.data_ptr(), yd.data_ptr(), ctypes.byref(d), code, _st()))
    assert_close(_ncl(yd, c), k["y"], 0, 0, "maxpool is exact")
    _pad_zero(yd, c, "y")
    dx = _nan_like(xd)
    _lib.check(lib.pasn_maxpool3d_bwd(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), ctypes.byref(d), code, _st()))
    tol = tk.tol_stores(1e-5, 1, dtype)
    _rel(_ncl(dx, c), k["dx"], tol, "dx")
    _pad_zero(dx, c, "dx")
    _rel(_ncl(dx, c).double().sum(dim=(2, 3, 4)), k["dy"].double().sum(dim=(2, 3, 4)), tol, "sum of dx per (clip, channel) == sum of dy")


HEAD_PARAMS = [pytest.param(tag, act, dt, True, id=f"{tag}-{'log' if act == 0 else 'linear'}-{'bf16' if dt == BF else 'fp32'}")
               for tag in tk.HEAD_CASES for act in (0, 1) for dt in (FP32, BF)]
HEAD_PARAMS += [pytest.param("r128", act, dt, False, id=f"r128-{'log' if act == 0 else 'linear'}-{'bf16' if dt == BF else 'fp32'}-no_dmin")
                for act in (0, 1) for dt in (FP32, BF)]


@pytest.mark.parametrize("tag,activation,dtype,with_dmin", HEAD_PARAMS)
def test_l2_head_backward(tag, activation, dtype, with_dmin):
    """pasn_l2_head_fwd then pasn_l2_head_bwd, called directly, against fp64 autograd of oracle.heads.ppnet_head's expression (l2_convolution ->
    min over positions -> distance_2_similarity -> linear) with loss weights on both outputs; once with dmin == NULL.  Shapes: D = 512 (two
    rounds of the 256-thread channel loop), S = 1, D = 12 in rows of Dp = 16 (the pad stays zero), and two constructed cases: five
    prototypes around ONE latent row of a clip (the ordered accumulation of l2_head_bwd_z_kernel), and a prototype EQUAL to a latent row
    (the state right after a push): d == 0 exactly, everything finite, dfc_w takes sim(0), the row's contribution 2 g (z - p) is 0.
    The kernel differentiates the UNCLAMPED distance |z|^2 - 2 z.p + |p|^2: the gradient of the true, non-negative distance -- the relu of
    the reference only clips rounding noise, and where it clips (d == 0) both gradients are 0 because z == p there.

    Bounds.  min_dist, fp32 and bf16 alike (bf16 products are exact in the fp32 accumulator): three fp32 sums of D terms of size ~D/3 cancel
    to ~D/6, each off by ~sqrt(D) * 6e-8 of its value -- 6 sqrt(D) * 6e-8 = 8e-6 of the result at D = 512: 1e-4 of the scale.  logits, coef,
    dprotos, dfc_w: fp32 sums, 1e-4.  dz: 1e-4, plus in bf16 one store per prototype that shares the row (read-modify-write in bf16);
    rows that are nobody's arg-min are exactly zero."""
    lib = _lib.lib()
    k = tk.head_case(tag, dtype, activation, with_dmin)
    n, S, D, Dp, P, K, code = k["n"], k["S"], k["D"], k["Dp"], k["P"], k["K"], _lib.dtype_code(dtype)
    zd = torch.zeros(n, S, Dp, dtype=dtype, device=DEV)
    zd[..., :D] = k["z"]
    pv, fw, gl = k["protos"].to(DEV), k["fcw"].to(DEV), k["dlogits"].to(DEV)
    gm = k["dmin"].to(DEV) if with_dmin else None
    mind, logits = torch.full((n, P), float("nan"), device=DEV), torch.full((n, K), float("nan"), device=DEV)
    amin = torch.full((n, P), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.pasn_l2_head_fwd(zd.data_ptr(), pv.data_ptr(), fw.data_ptr(), 0, mind.data_ptr(), amin.data_ptr(), logits.data_ptr(), n, S, D, Dp,
                                    P, K, code, activation, 1e-4, _st()))
    _rel(mind, k["min_dist"], 1e-4, "min_dist")
    assert torch.equal(amin.cpu().long(), k["argmin"]), "arg-min positions (every gap is above 1e-3 of the minimum)"
    _rel(logits, k["logits"], 1e-4, "logits")
    if tag == "exact":
        assert float(mind[1, 4]) == 0.0, "a prototype equal to a latent row: d == 0 exactly"
    outs = []
    for _ in range(2):
        dz, coef = _nan_like(zd), torch.full((n, P), float("nan"), device=DEV)
        dpv, dfw = _nan_like(pv), _nan_like(fw)
        _lib.check(lib.pasn_l2_head_bwd(zd.data_ptr(), pv.data_ptr(), fw.data_ptr(), mind.data_ptr(), amin.data_ptr(), gl.data_ptr(), _lib.ptr(gm),
                                        dz.data_ptr(), coef.data_ptr(), dpv.data_ptr(), dfw.data_ptr(), n, S, D, Dp, P, K, code, activation, 1e-4,
                                        _st()))
        torch.cuda.synchronize()
        outs.append((dz, coef, dpv, dfw))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "fixed accumulation order: two calls are bitwise equal"
    dz, coef, dpv, dfw = outs[0]
    assert all(bool(torch.isfinite(t).all()) for t in outs[0])
    _rel(coef, k["coef"], 1e-4, "coef")
    _rel(dpv, k["dprotos"], 1e-4, "dprototypes")
    _rel(dfw, k["dfc_w"], 1e-4, "dlast_layer")
    _pad_zero(dz, D, "dz")
    got, ref, scale = dz[..., :D].float().cpu(), k["dz"], float(k["dz"].abs().max()) + 1e-12
    for share in k["shared"].unique().tolist():
        rows = k["shared"] == share
        if share == 0:
            assert float(got[rows].abs().max()) == 0.0, "a row that is nobody's arg-min carries no gradient"
        else:
            assert_close(got[rows], ref[rows], tk.tol_stores(1e-4, share, dtype) * scale, 0.0, f"dz, rows shared by {share} prototype(s) (scale {scale:.3g})")


# ------------------------------------------------------------------------------------------------- whole model
# ReLU makes the end-to-end gradient DISCONTINUOUS in the weights: one pre-activation within rounding distance of zero flips
# its mask between two fp32 implementations, and in the late stages (R = N*T'*H'*W' of 32..512 rows per channel behind a
# batch-statistics norm) ONE flipped element moves whole gradient tensors by 3-40 % (measured: the fp32 oracle vs the same
# oracle in fp64 disagree on 2 of ~1e6 masks and by 9 % on stages.2.10.bn_a.bias; every configuration tried has pre-activations
# within 1e-6 of zero).  A strict end-to-end bound is therefore asserted on a KINK-SPARSE variant of the model -- +2.5 on the bias
# of every norm that feeds a ReLU, so only ~0.6 % of the pre-activations are masked and the density of values at the kink drops
# 23-fold (+4 would make ReLU the identity, and the bias gradients a pure cancellation residue) -- which still exercises every
# kernel, the tape order, residual / shortcut accumulation, SE, Swish, the head and the parameter slots; the ReLU derivative
# itself is pinned by the kernel-level tests above.  The unmodified model is then checked with bounds a mask flip cannot
# break but a wiring error would (strict forward outputs, global gradient direction).
def _train_model(kink_free, cfg=CFG_VIDEO_X3D):
    m = synth_model(cfg).to(DEV)
    if kink_free:
        relu_fed = {n + ".bias" for n, mod in m.named_modules() if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d))
                    and not any(t in n for t in ("downsample", "shortcut", "bn_b"))}  # norms whose output (or residual sum) feeds a ReLU
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name in relu_fed:
                    p += 2.5
    return m.train()


def _loss_weights(n, p, k, spatial, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g), torch.randn(n, p, generator=g), torch.randn((n, p, 1) + spatial, generator=g) * 0.1


def _oracle_step(sd, x, wl, ws, wo, occurrence_only=False, arch="x3d_s"):
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd.items()}
    out = oracle.nets.xprotonet_train_forward(sd, x, arch=arch, occurrence_only=occurrence_only)
    if occurrence_only:
        loss = (out["occurrence_map"] * wo).sum()
    else:
        loss = (out["logits"] * wl).sum() + (out["similarity"] * ws).sum() + (out["occurrence_map"] * wo).sum()
    loss.backward()
    return out, sd, loss


def _grad_errors(m, sd_ref, skip=()):
    rows = []
    for name, p in m.named_parameters():
        ref = sd_ref[name].grad
        if name == "ones" or name in skip:
            continue
        assert p.grad is not None, f"{name}: no gradient"
        assert ref is not None, name
        scale = float(ref.abs().max()) + 1e-12
        sib = sd_ref.get(name[:-4] + "weight") if name.endswith(".bias") else None
        if sib is not None and sib.grad is not None and sib.shape == ref.shape:
            # a norm layer's dbeta = sum(d) is a cancellation residue wherever the next norm removes the shift again; its
            # natural scale is that of the sibling dgamma = sum(d * yhat), a sum over the same rows
            scale = max(scale, float(sib.grad.abs().max()))
        rows.append((float((p.grad.cpu() - ref).abs().max()) / scale, name))
    rows.sort(reverse=True)
    return rows


def _check_grads(m, sd_ref, tol, skip=()):
    rows = _grad_errors(m, sd_ref, skip)
    assert rows[0][0] < tol, "largest relative gradient errors: " + ", ".join(f"{n} {e:.2e}" for e, n in rows[:6])


def _cosine(m, sd_ref, skip=()):
    names = [n for n, p in m.named_parameters() if n != "ones" and n not in skip and p.grad is not None]
    a = torch.cat([dict(m.named_parameters())[n].grad.flatten().cpu() / (float(sd_ref[n].grad.abs().max()) + 1e-12) for n in names])
    b = torch.cat([sd_ref[n].grad.flatten() / (float(sd_ref[n].grad.abs().max()) + 1e-12) for n in names])
    return float(F.cosine_similarity(a, b, dim=0))


SHAPE, SPATIAL = (2, 3, 4, 64, 64), (4, 2, 2)


def test_video_x3d_train_step_fp32_vs_oracle_autograd():
    """forward + loss.backward() in train mode: outputs, EVERY parameter gradient and the running statistics, fp32 <= 1e-3."""
    m = _train_model(kink_free=True)
    x = synth.echo_clips(SHAPE)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(2, 30, 3, SPATIAL)
    logits, sim, occ = m(x.to(DEV))
    assert logits.requires_grad and sim.requires_grad and occ.requires_grad
    loss = (logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()
    loss.backward()
    ref, sd_ref, loss_ref = _oracle_step(sd0, x, wl, ws, wo)
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(sim, ref["similarity"], 1e-3, "similarity")
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    _check_grads(m, sd_ref, 1e-3)
    sd1 = m.state_dict()
    for k_, v in sd_ref.items():
        if "running_" in k_:
            _rel(sd1[k_], v, 1e-4, k_)
        if k_.endswith("num_batches_tracked"):
            assert int(sd1[k_]) == 1, k_


def test_video_x3d_compute_occurence_map_train_and_second_step():
    """compute_occurence_map with gradients (loss.py:302), then a gradient step and a second pass: the launch lists re-pack the
    weights from the live parameters."""
    m = _train_model(kink_free=True)
    x = synth.echo_clips(SHAPE)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _, _, wo = _loss_weights(2, 30, 3, SPATIAL)
    occ = m.compute_occurence_map(x.to(DEV))
    (occ * wo.to(DEV)).sum().backward()
    ref, sd_ref, _ = _oracle_step(sd0, x, None, None, wo, occurrence_only=True)
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    head_only = {n for n, _ in m.named_parameters() if n.startswith("add_on_layers") or n in ("prototype_vectors", "last_layer.weight")}
    for n in head_only:
        assert dict(m.named_parameters())[n].grad is None, f"{n} is not on the occurrence-map path"
    _check_grads(m, sd_ref, 1e-3, skip=head_only)
    # a gradient step of 1 % of each tensor's magnitude, then a full pass from the same updated weights on both sides
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.grad is not None:
                p -= 1e-2 * float(p.abs().max()) / (float(p.grad.abs().max()) + 1e-12) * p.grad
            p.grad = None
    sd2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(2, 30, 3, SPATIAL, seed=9)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd_ref2, _ = _oracle_step(sd2, x, wl, ws, wo)
    _rel(logits, ref["logits"], 1e-3, "logits after the step")
    _check_grads(m, sd_ref2, 1e-3)


@pytest.mark.parametrize("cfg,shape,spatial", [(CFG_XPROTO, (3, 3, 96, 96), (3, 3)), (CFG_VIDEO_R2P1D, (2, 3, 8, 32, 32), (2, 4, 4))],
                         ids=["xprotonet_resnet18", "video_r2plus1d"])
def test_reference_trunks_train_step_fp32_vs_oracle_autograd(cfg, shape, spatial):
    """The reference's own trunks (2-D ResNet-18 with max-pool, R(2+1)D-18[:-3]: windowed dense convs, strided in space and time)
    through the same training path: outputs, every parameter gradient, running statistics."""
    m = _train_model(kink_free=True, cfg=cfg)
    arch, n = cfg["base_architecture"], shape[0]
    P, K = m.num_prototypes, m.num_classes
    x = synth.echo_clips(shape)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(n, P, K, spatial)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd_ref, _ = _oracle_step(sd0, x, wl, ws, wo, arch=arch)
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(sim, ref["similarity"], 1e-3, "similarity")
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    _check_grads(m, sd_ref, 1e-3)
    sd1 = m.state_dict()
    for k_, v in sd_ref.items():
        if "running_" in k_:
            _rel(sd1[k_], v, 1e-4, k_)


@pytest.mark.parametrize("cfg", [CFG_PPNET, CFG_PPNET_BOTTLENECK, dict(CFG_PPNET, prototype_activation_function="linear")],
                         ids=["regular", "bottleneck", "linear_activation"])
def test_ppnet_train_step_fp32_vs_oracle_autograd(cfg):
    """ProtoPNet (head A: distance map, min pooling, log activation, last layer; Sigmoid add-on) in train mode: logits,
    min_distances and every parameter gradient, with gradients entering through both outputs (cross entropy acts on the logits,
    the cluster / separation costs on min_distances: ProtoPNet_Base.py)."""
    m = _train_model(kink_free=True, cfg=cfg)
    shape = (3, 3, 96, 96)
    x = synth.echo_clips(shape)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    wl, wm = torch.randn(3, m.num_classes, generator=g), torch.randn(3, m.num_prototypes, generator=g)
    logits, min_d = m(x.to(DEV))
    assert logits.requires_grad and min_d.requires_grad
    ((logits * wl.to(DEV)).sum() + (min_d * wm.to(DEV)).sum()).backward()
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd0.items()}
    ref = oracle.nets.ppnet_train_forward(sd, x, arch="resnet18", activation=cfg["prototype_activation_function"])
    ((ref["logits"] * wl).sum() + (ref["min_distances"] * wm).sum()).backward()
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(min_d, ref["min_distances"], 1e-3, "min_distances")
    _check_grads(m, sd, 1e-3)


def test_video_x3d_train_step_ragged_shape():
    """Odd frame count, non-square planes that leave ragged strips / odd halves in every stride-2 stage, a single clip."""
    m = _train_model(kink_free=True)
    shape, spatial = (1, 3, 5, 96, 80), (5, 3, 3)
    x = synth.echo_clips(shape)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(1, 30, 3, spatial)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd_ref, _ = _oracle_step(sd0, x, wl, ws, wo)
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    _check_grads(m, sd_ref, 1e-3)


@pytest.mark.parametrize("phase", ["warm", "last_layer"])
def test_frozen_parameter_phases(phase):
    """The reference's agents freeze the trunk (warm-up) or everything but the last layer (XProtoNet_Base.py:253-293): frozen
    parts get no gradient and no backward launches; what stays trainable matches the oracle."""
    m = _train_model(kink_free=True)
    trainable = (lambda n: not n.startswith("cnn_backbone.")) if phase == "warm" else (lambda n: n == "last_layer.weight")
    for n, p in m.named_parameters():
        p.requires_grad_(trainable(n) and n != "ones")
    x = synth.echo_clips(SHAPE)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(2, 30, 3, SPATIAL)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd_ref, _ = _oracle_step(sd0, x, wl, ws, wo)
    _rel(logits, ref["logits"], 1e-3, "logits")
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n in frozen), n
    _check_grads(m, sd_ref, 1e-3, skip=frozen)
    plan = next(iter(m._train_runners.values())).plan
    n_bwd = sum(1 for k in plan.op_kind[plan.n_fwd:] if k != 2)  # (joins with the weight-gradient stream are not launches)
    assert n_bwd < (40 if phase == "warm" else 4), f"{n_bwd} backward launches for a frozen trunk"
    # running statistics still move: the norm layers stay in train mode (model.train())
    assert int(m.state_dict()["cnn_backbone.stem.bn.num_batches_tracked"]) == 1


def test_video_x3d_train_unmodified_model_vs_oracle():
    """The model as built (ReLU kinks in play): strict forward parity; gradients within what a few mask flips can move."""
    m = _train_model(kink_free=False)
    x = synth.echo_clips(SHAPE)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(2, 30, 3, SPATIAL)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd_ref, _ = _oracle_step(sd0, x, wl, ws, wo)
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(sim, ref["similarity"], 1e-3, "similarity")
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    rows = _grad_errors(m, sd_ref)
    median = rows[len(rows) // 2][0]
    cos = _cosine(m, sd_ref)
    assert cos > 0.98 and median < 5e-2, f"gradient direction cosine {cos:.4f}, median per-tensor error {median:.2e}; worst {rows[:3]}"


@pytest.mark.timeout(900)
def test_video_x3d_train_unmodified_model_calibrated_by_the_oracles_own_kink_sensitivity():
    """Gradient parity on the model AS BUILT (no bias shift: half of all units sit behind a ReLU mask, so mask handling is exercised in
    full).  A pre-activation within rounding distance of zero flips its mask between two fp32 implementations, and one flip in a late
    layer moves every gradient upstream of it -- so no fixed tolerance is both honest and tight.  The bound is CALIBRATED per run: the
    same oracle pass in fp64 gives the exact gradients, the fp32 oracle's deviation from them measures what mask flips (and fp32
    rounding) cost ANY correct fp32 implementation on this very input, and the HIP gradients -- compared with the fp64 ones, tensor by
    tensor -- must stay within a small multiple of that: median <= 3x the fp32 oracle's median (+1e-4), largest <= 10x its largest
    (+1e-3).  Clips of 8 x 128 x 128 (single flips diluted over 6x more rows than the small shape's).  Forward outputs: strict 1e-3."""
    m = _train_model(kink_free=False)
    shape, spatial = (3, 3, 8, 128, 128), (8, 4, 4)
    x = synth.echo_clips(shape)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    wl, ws, wo = _loss_weights(3, 30, 3, spatial)
    logits, sim, occ = m(x.to(DEV))
    ((logits * wl.to(DEV)).sum() + (sim * ws.to(DEV)).sum() + (occ * wo.to(DEV)).sum()).backward()
    ref, sd32, _ = _oracle_step(sd0, x, wl, ws, wo)
    sd0_64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}
    _, sd64, _ = _oracle_step(sd0_64, x.double(), wl.double(), ws.double(), wo.double())
    _rel(logits, ref["logits"], 1e-3, "logits")
    _rel(sim, ref["similarity"], 1e-3, "similarity")
    _rel(occ, ref["occurrence_map"], 1e-3, "occurrence_map")
    e_hip, e_or = [], []
    for name, p in m.named_parameters():
        if name == "ones":
            continue
        g32, g64 = sd32[name].grad, sd64[name].grad.float()
        scale = float(g64.abs().max()) + 1e-12
        sib = sd64.get(name[:-4] + "weight") if name.endswith(".bias") else None
        if sib is not None and sib.grad is not None and sib.shape == g64.shape:
            scale = max(scale, float(sib.grad.abs().max()))  # dbeta lives on the scale of its sibling dgamma (see _grad_errors)
        e_or.append((float((g32 - g64).abs().max()) / scale, name))
        e_hip.append((float((p.grad.cpu() - g64).abs().max()) / scale, name))
    med = lambda rows: sorted(r[0] for r in rows)[len(rows) // 2]
    top = lambda rows: max(rows)
    print(f"unmodified-model gradients vs the fp64 oracle, {len(e_hip)} tensors: fp32 oracle median {med(e_or):.2e} max {top(e_or)[0]:.2e} ({top(e_or)[1]}); "
          f"HIP median {med(e_hip):.2e} max {top(e_hip)[0]:.2e} ({top(e_hip)[1]})")
    assert med(e_hip) <= 3 * med(e_or) + 1e-4, f"HIP median per-tensor error {med(e_hip):.2e} vs the fp32 oracle's {med(e_or):.2e}"
    assert top(e_hip)[0] <= 10 * top(e_or)[0] + 1e-3, f"HIP worst tensor {top(e_hip)} vs the fp32 oracle's worst {top(e_or)}"


@pytest.mark.parametrize("cfg,shape,spatial,env", [(CFG_VIDEO_X3D, SHAPE, SPATIAL, ""), (CFG_VIDEO_X3D, SHAPE, SPATIAL, "PASN_DW_DGRAD_REDUCE"),
                                                   (CFG_VIDEO_X3D, SHAPE, SPATIAL, "PASN_NO_DW_STATS"), (CFG_VIDEO_X3D, SHAPE, SPATIAL, "PASN_NO_SE_ANALYTIC"),
                                                   (CFG_VIDEO_X3D, SHAPE, SPATIAL, "PASN_NO_PACK"),
                                                   (CFG_VIDEO_R2P1D, (2, 3, 8, 32, 32), (2, 4, 4), ""),
                                                   (CFG_XPROTO, (3, 3, 96, 96), (3, 3), "")],
                         ids=["x3d_s", "x3d_s-dgrad+sums", "x3d_s-separate-stats", "x3d_s-two-pass-se", "x3d_s-torch-packed-weights", "r2plus1d", "resnet18"])
def test_train_bf16_activations_track_fp32(cfg, shape, spatial, env, monkeypatch):
    """bf16 activations / activation gradients (fp32 statistics, reductions, parameter gradients) against the fp32 mode, every trunk
    (bf16 takes other kernels: T-marching stencils with the batch statistics fused in -- and, opt-in, the producer unit's backward sums
    in the stencil dgrad --, LDS-transposed MFMA weight gradients incl. the windowed ones)."""
    if env:
        monkeypatch.setenv(env, "1")
    x = synth.echo_clips(shape).to(DEV)
    grads, outs = {}, {}
    for tag, dt in (("f32", None), ("bf16", torch.bfloat16)):
        m = _train_model(kink_free=True, cfg=cfg)
        wl, ws, wo = (t.to(DEV) for t in _loss_weights(shape[0], m.num_prototypes, m.num_classes, spatial))
        m.set_compute_dtype(dt)
        logits, sim, occ = m(x)
        ((logits * wl).sum() + (sim * ws).sum() + (occ * wo).sum()).backward()
        grads[tag] = {n: p.grad.float().flatten() / (float(p.grad.abs().max()) + 1e-12) for n, p in m.named_parameters() if p.grad is not None}
        outs[tag] = (logits.detach(), sim.detach())
        assert all(torch.isfinite(g).all() for g in grads[tag].values())
    _rel(outs["bf16"][1], outs["f32"][1], 5e-2, "similarity, bf16 vs fp32 activations")
    names = sorted(grads["f32"])
    per = sorted((float(F.cosine_similarity(grads["f32"][n], grads["bf16"][n], dim=0)), n) for n in names)
    a = torch.cat([grads["f32"][n] for n in names])
    b = torch.cat([grads["bf16"][n] for n in names])
    cos = float(F.cosine_similarity(a, b, dim=0))
    assert cos > 0.95, f"bf16-activation gradients drifted from fp32: cosine {cos:.4f}; lowest per tensor {per[:5]}"


def test_second_backward_through_one_forward_is_refused():
    """The backward launch list reuses the forward's activations as scratch: a second replay (retain_graph=True) would return wrong
    gradients silently, so it raises instead."""
    m = synth_model(CFG_VIDEO_X3D).to(DEV).train()
    logits, sim, occ = m(synth.echo_clips((2, 3, 4, 64, 64)).to(DEV))
    loss = logits.sum() + sim.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already differentiated"):
        loss.backward()
    logits, sim, occ = m(synth.echo_clips((2, 3, 4, 64, 64)).to(DEV))  # a fresh forward differentiates fine
    (logits.sum() + occ.sum()).backward()


def test_training_guards():
    m = synth_model(CFG_VIDEO_X3D).to(DEV).train()
    with pytest.raises(RuntimeError):
        m.push_forward(synth.echo_clips((1, 3, 4, 64, 64)).to(DEV))
    m2 = synth_model(CFG_VIDEO_X3D).to(DEV).bfloat16().train()
    with pytest.raises(RuntimeError, match="fp32 master"):
        m2(synth.echo_clips((1, 3, 4, 64, 64)).to(DEV).bfloat16())


# ------------------------------------------------------------------------------------------------- TransformLoss
@pytest.mark.parametrize("shape,angle,scale", [((6, 3, 17, 23), 13.0, 0.8), ((4, 2, 32, 32), -20.0, 1.5), ((3, 5, 7, 7), 7.5, 0.6)])
def test_affine_warp_forward_backward_vs_torchvision_restatement(shape, angle, scale):
    from protoasnet_amd.losses import affine_warp

    g = torch.Generator().manual_seed(shape[-1])
    x = torch.randn(shape, generator=g).requires_grad_()
    ref = oracle.losses.affine(x, angle, scale)
    w = torch.randn(ref.shape, generator=g)
    (ref * w).sum().backward()
    xd = x.detach().to(DEV).requires_grad_()
    y = affine_warp(xd, angle, scale)
    (y * w.to(DEV)).sum().backward()
    _rel(y, ref, 1e-5, "warped planes")
    _rel(xd.grad, x.grad, 1e-5, "warp adjoint")
    yb = affine_warp(x.detach().to(DEV).bfloat16(), angle, scale)
    _rel(yb, oracle.losses.affine(x.detach().bfloat16().float(), angle, scale), 1e-2, "bf16 planes")


def test_transform_loss_value_and_gradients_vs_oracle():
    """TransformLoss.compute (loss.py:283-320): warped clip -> second trunk pass with gradients, warped maps, L1."""
    from protoasnet_amd.losses import TransformLoss

    m = _train_model(kink_free=True)
    x = synth.echo_clips(SHAPE)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    cfg = {"angle": 11.0, "scale": 0.9}
    _, _, occ = m(x.to(DEV))
    loss = TransformLoss(loss_weight=1e-2, reduction="mean").compute(x.to(DEV), occ, m, config=cfg)
    loss.backward()
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd0.items()}
    occ_ref = oracle.nets.xprotonet_train_forward(sd, x, arch="x3d_s")["occurrence_map"]
    ref = oracle.losses.transform_loss(x, occ_ref, lambda xt: oracle.nets.xprotonet_train_forward(sd, xt, arch="x3d_s", occurrence_only=True)["occurrence_map"],
                                       cfg["angle"], cfg["scale"], loss_weight=1e-2, reduction="mean")
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-3 * abs(float(ref.detach())), (float(loss.detach()), float(ref.detach()))
    head_only = {n for n, _ in m.named_parameters() if n.startswith("add_on_layers") or n in ("prototype_vectors", "last_layer.weight")}
    # |a - b| has its own kink at a == b; the maps differ everywhere here, so the strict bound holds
    _check_grads(m, sd, 2e-3, skip=head_only)


# ------------------------------------------------------------------------------------------------- vs the REFERENCE's own train mode
@pytest.mark.parametrize("tag,cfg", [("xproto", CFG_XPROTO), ("ppnet", CFG_PPNET)])
def test_train_step_vs_reference_train_mode_golden(golden, tag, cfg):
    """HIP training pass vs outputs / gradient summaries / running statistics recorded from the reference itself in train mode
    (tests/golden/g7_train_resnet18.npz, made by tests/golden/make_golden_train.py)."""
    import numpy as np

    from train_cases import FULL_GRADS, SHAPE as GSHAPE, kink_sparse_, loss_weights

    g = golden("g7_train_resnet18.npz")
    m = kink_sparse_(synth_model(dict(cfg, img_size=GSHAPE[-1]))).to(DEV).train()
    x = synth.echo_clips(GSHAPE).to(DEV)
    if tag == "xproto":
        logits, sim, occ = m(x)
        wl, ws, wo = (t.to(DEV) for t in loss_weights(GSHAPE[0], 40, 4, tuple(occ.shape[3:])))
        outs = {"logits": logits, "similarity": sim, "occurrence_map": occ}
        loss = (logits * wl).sum() + (sim * ws).sum() + (occ * wo).sum()
    else:
        logits, min_d = m(x)
        wl, wm, _ = (t.to(DEV) for t in loss_weights(GSHAPE[0], 30, 3, (1, 1)))
        outs = {"logits": logits, "min_distances": min_d}
        loss = (logits * wl).sum() + (min_d * wm).sum()
    loss.backward()
    for name, t in outs.items():
        _rel(t, g[f"{tag}_{name}"], 1e-3, name)
    params = dict(m.named_parameters())
    for n, (gmax, gsum, gsq) in zip(g[f"{tag}_grad_names"], g[f"{tag}_grad_stats"]):
        gr = params[str(n)].grad.double()
        assert abs(float(gr.abs().max()) - gmax) <= 2e-3 * gmax + 1e-12, (str(n), float(gr.abs().max()), gmax)
        assert abs(float((gr * gr).sum()) - gsq) <= 4e-3 * gsq + 1e-20, (str(n), "sum of squares")
    for n in FULL_GRADS:
        if f"{tag}_grad::{n}" in g.files:
            _rel(params[n].grad, g[f"{tag}_grad::{n}"], 1e-3, f"grad of {n}")
    sd = m.state_dict()
    for key in g.files:
        if key.startswith(f"{tag}_buf::"):
            _rel(sd[key.split("::", 1)[1]], g[key], 1e-4, key)


@pytest.mark.timeout(900)
def test_cfg3_full_size_train_step_bf16_tracks_fp32():
    """BASELINE config 3's per-GPU work at its FULL size under the test suite: one training step (train-mode forward, loss, backward) of
    Video ProtoASNet / X3D-S on 32 clips of 3 x 16 x 224 x 224, in bf16 activations and in fp32, same parameters and clips.  No CPU oracle at
    this size (minutes); the small-shape tests anchor both modes on it.  Here: every output and every parameter gradient finite, outputs of
    the two modes within the bf16 forward tolerance, gradient direction cosine > 0.95 over all parameters (each tensor normalised by its
    fp32 scale), and the norm layers' running statistics of the two modes within 1e-2 of their scale."""
    x = synth.echo_clips((32, 3, 16, 224, 224))
    g = torch.Generator().manual_seed(3)
    wl, ws, wo = torch.randn(32, 3, generator=g), torch.randn(32, 30, generator=g), torch.randn(32, 30, 1, 16, 7, 7, generator=g) * 0.1
    grads, outs, stats = {}, {}, {}
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        m = _train_model(kink_free=True)  # as the small-shape bf16-vs-fp32 test: bf16 rounding flips ReLU masks within 2^-8 of zero, and in a random-weight
        # network as built (half of all units masked) those flips alone decorrelate the two modes' gradients (cosine 0.33 measured)
        if dt == torch.bfloat16:
            m.set_compute_dtype(dt)
        logits, sim, occ = m(x.to(DEV).to(dt))
        ((logits.float() * wl.to(DEV)).sum() + (sim.float() * ws.to(DEV)).sum() + (occ.float() * wo.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        outs[tag] = (logits.detach().float().cpu(), sim.detach().float().cpu(), occ.detach().float().cpu())
        grads[tag] = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None}
        stats[tag] = {k: v.detach().float().cpu() for k, v in m.state_dict().items() if "running_" in k}
        for n, gr in grads[tag].items():
            assert bool(torch.isfinite(gr).all()), f"{tag}: non-finite gradient in {n}"
        assert all(bool(torch.isfinite(o).all()) for o in outs[tag])
        del m, logits, sim, occ
        torch.cuda.empty_cache()
    assert len(grads["f32"]) == len(grads["bf16"]) >= 300
    assert float((outs["bf16"][1] - outs["f32"][1]).abs().max()) < 2e-2, "similarities of the two modes"
    # each mode's tensors on their OWN scale, as the small-shape test does: a norm bias behind a second norm has a TRUE gradient of ~0 (the next norm
    # removes the shift again), what is left is rounding residue, 10^4 x larger in bf16 than in fp32 -- on the fp32 scale those few tensors would
    # dominate the concatenated vector (cosine 0.006 measured that way with every weight tensor at 0.99)
    a = torch.cat([grads["bf16"][n].flatten() / (float(grads["bf16"][n].abs().max()) + 1e-12) for n in grads["f32"]])
    b = torch.cat([grads["f32"][n].flatten() / (float(grads["f32"][n].abs().max()) + 1e-12) for n in grads["f32"]])
    cos = float(F.cosine_similarity(a, b, dim=0))
    per = sorted((float(F.cosine_similarity(grads["bf16"][n].flatten(), grads["f32"][n].flatten(), dim=0)), n) for n in grads["f32"])
    hist = [sum(1 for c_, _ in per if c_ > t) for t in (0.99, 0.9, 0.5, 0.0)]
    big = sorted(((grads["f32"][n].numel(), n) for n in grads["f32"]), reverse=True)[:8]
    bigcos = [(n, round(dict((nn, cc) for cc, nn in per)[n], 4), float(grads["f32"][n].abs().max()), float(grads["bf16"][n].abs().max())) for _, n in big]
    assert hist[1] >= 0.9 * len(per), f"only {hist[1]} of {len(per)} gradient tensors have a bf16-vs-fp32 cosine above 0.9: lowest {per[:6]}"
    assert cos > 0.95, (f"bf16 vs fp32 gradient direction cosine {cos:.4f}; tensors with cos > 0.99 / 0.9 / 0.5 / 0: {hist} of {len(per)}; largest tensors "
                        f"(name, cos, max|g| fp32, bf16): {bigcos}; lowest {per[:4]}; sim diff {float((outs['bf16'][1] - outs['f32'][1]).abs().max()):.3g}")
    for k, v in stats["f32"].items():
        assert float((stats["bf16"][k] - v).abs().max()) <= 1e-2 * (float(v.abs().max()) + 1e-6) + 1e-4, k


@pytest.mark.parametrize("cfg,shape,spatial,env", [(CFG_XPROTO, (4, 3, 96, 96), (3, 3), ""), (CFG_VIDEO_R2P1D, (2, 3, 8, 32, 32), (2, 4, 4), ""),
                                                   (CFG_VIDEO_X3D, (4, 3, 8, 96, 96), (8, 3, 3), "PASN_NO_SE_ANALYTIC"),
                                                   (CFG_VIDEO_X3D, (4, 3, 8, 96, 96), (8, 3, 3), "PASN_TRAIN_STREAMS")],
                         ids=["xprotonet_resnet18", "video_r2plus1d", "x3d_se_three_pass_backward", "x3d_one_stream"])
def test_paired_pass_other_trunks_and_routes(cfg, shape, spatial, env, monkeypatch):
    """forward_pair against the two passes (fp32) on the reference's own trunks -- BatchNorm2d behind a max-pool, windowed dense 3-D convs -- and on
    the X3D model with the three-pass squeeze-excite backward (modes 1 + 2: the per-clip `add` and the per-group coefficients meet in mode 2) and
    with every launch on one stream."""
    import copy

    if env:
        monkeypatch.setenv(env, "1")
    m1 = _train_model(kink_free=True, cfg=cfg)
    m2 = copy.deepcopy(m1)
    n, P, K = shape[0], m1.num_prototypes, m1.num_classes
    x = synth.echo_clips(shape).to(DEV)
    xw = torch.roll(x, shifts=(3, -5), dims=(-2, -1)) * 0.8 + 0.05
    wl, ws, wo = (t.to(DEV) for t in _loss_weights(n, P, K, spatial))
    wo2 = wo.flip(0) * 0.7
    logits, sim, occ = m1(x)
    occ_w = m1.compute_occurence_map(xw)
    ((logits * wl).sum() + (sim * ws).sum() + (occ * wo).sum() + (occ_w * wo2).sum()).backward()
    (l2, s2, o2), ow2 = m2.forward_pair(x, xw)
    ((l2 * wl).sum() + (s2 * ws).sum() + (o2 * wo).sum() + (ow2 * wo2).sum()).backward()
    for a, b, name in ((l2, logits, "logits"), (s2, sim, "similarity"), (o2, occ, "occurrence_map"), (ow2, occ_w, "occurrence_map of the second half")):
        _rel(a, b, 2e-4, name)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        if "num_batches_tracked" in k:
            assert int(sd1[k]) == int(sd2[k]) == 2, k
        elif "running_" in k:
            _rel(sd2[k], sd1[k], 1e-4, k)
    g1 = {nm: p.grad for nm, p in m1.named_parameters()}
    for (n1, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is None:
            continue
        scale = float(p1.grad.abs().max()) + 1e-12
        sib = g1.get(n1[:-4] + "weight") if n1.endswith(".bias") else None
        if sib is not None and sib.shape == p1.grad.shape:
            scale = max(scale, float(sib.abs().max()))
        err = float((p1.grad - p2.grad).abs().max()) / scale
        assert err < 2e-3, f"{n1}: paired-pass gradient off by {err:.2e} of its scale"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_paired_pass_equals_forward_plus_compute_occurence_map(dtype):
    """model.forward_pair(x, x_w) in train mode -- ONE compiled pass over [x, x_w] with two statistics groups (TrainRunner mode 2) -- against the
    reference's two passes, model(x) then model.compute_occurence_map(x_w) (Video_XProtoNet_e2e.py:84, loss.py:302), on models with identical
    weights: outputs, every parameter gradient of the summed loss, the running statistics (updated twice, in order) and num_batches_tracked.
    Each half sees only its own batch statistics: the same numbers up to the fp32 summation order (fp32 run) / bf16 storage (bf16 run)."""
    import copy

    shape, spatial = (4, 3, 8, 96, 96), (8, 3, 3)
    m1 = _train_model(kink_free=True)
    m2 = copy.deepcopy(m1)
    if dtype == torch.bfloat16:
        m1.set_compute_dtype(torch.bfloat16)
        m2.set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips(shape).to(DEV)
    xw = torch.roll(x, shifts=(3, -5), dims=(3, 4)) * 0.8 + 0.05  # a different clip distribution: different batch statistics per half
    wl, ws, wo = (t.to(DEV) for t in _loss_weights(shape[0], 30, 3, spatial))
    wo2 = wo.flip(0) * 0.7

    logits, sim, occ = m1(x)
    occ_w = m1.compute_occurence_map(xw)
    ((logits * wl).sum() + (sim * ws).sum() + (occ * wo).sum() + (occ_w * wo2).sum()).backward()

    (l2, s2, o2), ow2 = m2.forward_pair(x, xw)
    ((l2 * wl).sum() + (s2 * ws).sum() + (o2 * wo).sum() + (ow2 * wo2).sum()).backward()

    tol = 2e-4 if dtype == torch.float32 else 3e-2
    for a, b, name in ((l2, logits, "logits"), (s2, sim, "similarity"), (o2, occ, "occurrence_map"), (ow2, occ_w, "occurrence_map of the second half")):
        _rel(a, b, tol, name)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        if "num_batches_tracked" in k:
            assert int(sd1[k]) == int(sd2[k]) == 2, k
        elif "running_" in k:
            _rel(sd2[k], sd1[k], 1e-4 if dtype == torch.float32 else 2e-2, k)
    gtol = 2e-3 if dtype == torch.float32 else 5e-2
    g1 = {n: p.grad for n, p in m1.named_parameters()}
    errs = []
    for (n1, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is not None:
            scale = float(p1.grad.abs().max()) + 1e-12
            sib = g1.get(n1[:-4] + "weight") if n1.endswith(".bias") else None
            if sib is not None and sib.shape == p1.grad.shape:
                scale = max(scale, float(sib.abs().max()))  # dbeta lives on the scale of its sibling dgamma (a norm in front of another norm: ~0)
            if dtype == torch.float32:
                err = float((p1.grad - p2.grad).abs().max()) / scale
            else:  # bf16 storage of every activation and gradient, two summation orders: compare in the L2 sense (single entries of the stem's
                err = float((p1.grad - p2.grad).norm()) / (float(p1.grad.norm()) + scale)  # gradient move by 8 % of the largest one)
            errs.append((err, n1))
    if dtype == torch.float32:
        assert max(errs)[0] < gtol, f"paired-pass gradient off by {max(errs)[0]:.2e} of its scale: {max(errs)[1]}"
    else:  # per tensor the two bf16 runs differ as two bf16 evaluations of one network do (measured: median 5 %, worst 17 % in the L2 sense, i.e.
        # direction cosines 0.999 / 0.985 -- the bf16-vs-fp32 tests of this file ask 0.9 per tensor)
        med = sorted(e for e, _ in errs)[len(errs) // 2]
        assert med < 8e-2 and max(errs)[0] < 0.3, f"paired-pass gradients (bf16): median {med:.2e}, worst {max(errs)}"
