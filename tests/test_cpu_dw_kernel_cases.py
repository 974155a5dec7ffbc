"""CPU: the table of tests/dw_kernel_cases.py, checked without a GPU -- (a) every row reaches exactly the kernel instance it names, (b) the
table claims every instance ``PlanBuilder.dwconv`` / ``dwconv_se`` / ``expand_dw`` emit in the default plans (the ledger) and holds the
shapes its docstring promises, (c) the fp64 reference stays within one weight rounding of torch's conv3d(groups = C) + eval-mode BatchNorm3d
on the unrounded taps, (d) the bound holds for an fp32-accumulating emulation of a correct kernel on every row and FAILS on thirteen ways a
depthwise kernel goes subtly wrong."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dw_kernel_cases as dk
import train_kernel_cases as tk
from test_cpu_conv_kernel_cases import default_plan_meta

F64 = torch.float64
IDS = [c.id for c in dk.CASES]
KINDS = ("dwconv", "dwconv+se", "expand+dwconv")


@pytest.fixture(scope="module")
def built_on_cpu():
    """{row id: ``Built``} of every row, built on the CPU under its switches."""
    out = {}
    for c in dk.CASES:
        with dk.switches(c):
            out[c.id] = dk.build(c, "cpu")
    return out


# ------------------------------------------------------------------------------------------------- (a) instance names
@pytest.mark.parametrize("case", dk.CASES, ids=IDS)
def test_every_row_reaches_the_instance_it_names(case, built_on_cpu):
    b = built_on_cpu[case.id]
    assert b.name == case.expect, f"{case.id}: the row runs {b.name}, its label says {case.expect}"
    assert b.kind == ("expand+dwconv" if case.expand else "dwconv+se" if case.se else "dwconv") and len(b.pb.ops) == 1
    assert (b.pool_blocks > 0) == case.pool


def test_rows_cover_what_the_table_promises(built_on_cpu):
    """Per family: N >= 2 on every row, a partial 8-channel group and a partial 16-channel tile, a pool row where the family writes pool rows,
    one with several partial rows, T no multiple of the forced chunk where the family chunks T, T = 1; every instance the issue lists."""
    fam = {}
    for c in dk.CASES:
        fam.setdefault(dk.family(c), []).append(c)
    assert set(fam) == {"dwconv3d_kernel", "dwconv3d_strip_kernel", "dwconv3d_march_kernel", "dwconv_t_kernel", "dwconv3d_mfma_kernel",
                        "dwconv3d_tz_kernel", "x3d_expdw_kernel", "x3d_expdw_tz_kernel"}
    for name, rows in fam.items():
        assert all(c.nthw[0] >= 2 for c in rows), f"{name}: a row with one clip"
        assert any(c.c % 8 for c in rows) and any(c.c % 16 and not c.c % 8 for c in rows), f"{name}: no partial 8-channel group / 16-channel tile"
        assert any(c.nthw[1] == 1 for c in rows), f"{name}: no T = 1 row"
        if name != "dwconv_t_kernel":  # writes no pool rows
            assert any(c.pool for c in rows), f"{name}: no pool row"
            assert any(built_on_cpu[c.id].pool_blocks > 1 for c in rows), f"{name}: no row with pool_blocks > 1"
        if name not in ("dwconv3d_kernel", "dwconv3d_strip_kernel", "dwconv_t_kernel"):  # these do not chunk T
            assert any(dk.t_chunk(c) and c.nthw[1] > dk.t_chunk(c) and c.nthw[1] % dk.t_chunk(c) for c in rows), f"{name}: T a multiple of every forced chunk"
    names = {c.expect for c in dk.CASES}
    want = {f"dwconv3d_kernel<{t}>" for t in ("f32", "bf16")} | {f"dwconv_t_kernel<{t},{k}>" for t in ("f32", "bf16") for k in (3, 5)}
    want |= {f"dwconv3d_strip_kernel<{t},{v}>" for t in ("f32", "bf16") for v in ("8,3,1", "7,3,1", "4,3,2", "8,1,1", "7,1,1")}
    want |= {"dwconv3d_march_kernel<1,2>", "dwconv3d_march_kernel<1,3>", "dwconv3d_march_kernel<2,2>", "dwconv3d_march_kernel<1,se>"}
    want |= {f"dwconv3d_mfma_kernel<{r},false,{a}>" for r in (1, 2) for a in (0, 3, -1)}
    want |= {f"dwconv3d_tz_kernel<{a},{p}>" for a in (0, 3) for p in ("true", "false")} | {f"x3d_expdw_tz_kernel<1,{a},{p}>" for a in (0, 3) for p in ("true", "false")}
    want |= {f"x3d_expdw_kernel<2,{a},{s}>" for a, s in ((0, 2), (3, 2), (-1, 2), (0, 1), (3, 1))}
    assert want <= names, sorted(want - names)
    for inst in sorted(n for n in want if n.startswith("x3d_expdw_kernel")):  # FOLD is not in the name: both forms of every instance
        folds = {dk.expand_fold(c) for c in dk.CASES if c.expect == inst}
        assert folds == {True, False}, f"{inst}: norm_a folded / applied behind the MFMAs: {folds}"
    for sw in (1, 2):
        tcs = {dk.t_chunk(c) for c in fam["dwconv3d_march_kernel"] if c.s[2] == sw}
        assert {4, 8, 16} <= tcs, f"march, stride {sw}: PASN_DWM_TC {tcs}"
    assert {1, 3} <= {dk.t_chunk(c) for c in fam["dwconv3d_tz_kernel"]}
    assert any(c.c > 512 for c in fam["dwconv3d_strip_kernel"])
    se = [c for c in dk.CASES if c.se]
    assert len(se) >= 3 and any(built_on_cpu[c.id].pool_blocks > 1 for c in se) and any(c.c % 8 for c in se)
    # the matrix-core stencil on planes at most 8 wide and wider; Toeplitz planes without a second band, with a cut one
    assert {c.nthw[3] <= 8 for c in fam["dwconv3d_mfma_kernel"]} == {True, False}
    assert {min(c.nthw[2], 9) for c in fam["dwconv3d_tz_kernel"]} >= {5, 9} and any(8 < c.nthw[2] < 14 for c in fam["dwconv3d_tz_kernel"])


# ------------------------------------------------------------------------------------------------- (b) the ledger
def _default_plan_names():
    seen = {}
    for name, m in default_plan_meta():
        if m["kind"] in KINDS:
            seen.setdefault(m["kernel"], f"{name}: {m['shape']}")
    return seen


def _unclaimed(seen, claimed):
    return {k: v for k, v in seen.items() if k not in claimed}


def test_ledger_every_depthwise_instance_of_the_default_plans_has_a_row():
    seen = _default_plan_names()
    assert len(seen) >= 11, "the collection itself broke"
    missing = _unclaimed(seen, {c.expect for c in dk.CASES})
    assert not missing, "instances a default plan launches and no row of tests/dw_kernel_cases.py runs:\n" + "\n".join(f"  {k}   ({v})" for k, v in missing.items())


def test_ledger_notices_a_row_that_is_gone():
    """With one claimed production instance taken out of the table the ledger names exactly that instance."""
    victim = "x3d_expdw_tz_kernel<1,0,true>"
    claimed = {c.expect for c in dk.CASES if c.expect != victim}
    assert list(_unclaimed(_default_plan_names(), claimed)) == [victim]


# ------------------------------------------------------------------------------------------------- (c) the reference
def _bn64(c, q):
    bn = nn.BatchNorm3d(c).double().eval()
    with torch.no_grad():
        bn.weight.copy_(q["gamma"]), bn.bias.copy_(q["beta"]), bn.running_mean.copy_(q["mean"]), bn.running_var.copy_(q["var"])
    return bn


@pytest.mark.parametrize("case", dk.CASES, ids=IDS)
def test_reference_is_within_one_weight_rounding_of_depthwise_conv3d_and_batch_norm(case):
    """Independent restatement: F.conv3d(groups = C) + nn.BatchNorm3d.eval() in fp64 on the UNROUNDED taps.  Operand model ``none``: the two
    agree to the accuracy of the launch's fp32 fold of the norm (a few 2^-24 of |scale| and of |beta| + |mean scale| < 4); otherwise within
    2^-8 * A, the design rounding of one bf16 weight per term (2^-9 each, the factor 2 covers A being taken on the rounded weights).  An
    ``expand`` row's intermediate is held to the same statement one stage up."""
    dtype, T = dk.DT[case.dtype], dk.tensors(case.id)
    R = dk.reference(case.id)
    x, flip = dk.stencil_input(case)
    with torch.no_grad():
        if case.expand:
            x0 = tk.rnd(T["x"], dtype)
            wa = T["wa"].to(F64).view(case.c, case.expand, 1, 1, 1)
            u = _bn64(case.c, T["bn_a"])(F.conv3d(x0, wa))
            sa, ba = (v.to(F64).view(1, -1, 1, 1, 1) for v in dk.folded(T["bn_a"], case.c))
            A_e = sa.abs() * F.conv3d(x0.abs(), wa.abs()) + ba.abs()
            want_e = torch.relu(u)
            assert bool(((x - want_e).abs() <= 2.0 ** -8 * A_e + 2.0 ** -8 * want_e + 1.1 * 2.0 ** -20 * (A_e + 4)).all())
            assert R["at_risk"] < 0.01, f"{case.id}: {R['at_risk']:.4f} of the intermediate elements sit within eps_e of a rounding boundary"
            assert float((flip > 0).double().mean()) == R["at_risk"] and float((x > 0).double().mean()) > 0.2
        pre = _bn64(case.c, T["bn"])(F.conv3d(x, T["w"].to(F64), None, case.s, case.p, groups=case.c))
    want = dk.ACT[case.act](pre)
    assert want.shape == R["ref"].shape
    model, _ = dk.operand_model(case)
    tol = 1.1 * 2.0 ** -20 * (R["A"] + 4) + (0.0 if model == "none" else 2.0 ** -8 * R["A"])
    err = (R["ref"] - want).abs()
    assert bool((err <= dk.LIPSCHITZ[case.act] * tol).all()), float((err / tol).max())
    if model != "none":
        assert float(err.max()) > 2.0 ** -12, "a rounded-weight model that rounds nothing"
    assert bool((R["bound"] > 0).all()) and 0.2 < float((R["pre"] > 0).double().mean()) < 0.8
    if case.pool:
        assert bool((R["pool_bound"] > 0).all())


# ------------------------------------------------------------------------------------------------- (d) the bound discriminates
def _emulate(case, drop_tap=False, halo_wrap=False, clip_leak=False, tail_taps=False, unrounded_e=False, no_relu=False, bf16_taps=False,
             pool_after_act=False):
    """What a correct kernel computes, with fp32 accumulation: torch fp32 ops on the same rounded operands (``dk.effective_taps``, the
    expand conv's folded weights), the pool sums and the gate in fp32, the output rounded to the dtype -- as ``dk.Ran`` in the launch's
    layouts, the clip's pool sum in partial row 0.  The keywords are the faults of the test below."""
    dtype, T = dk.DT[case.dtype], dk.tensors(case.id)
    c, cp, (kt, kh, kw), (pt, ph, pw) = case.c, dk.round_up(case.c, 8), case.k, case.p
    x = T["x"].to(dtype).float()
    if case.expand:
        sa, ba = (v.view(1, -1, 1, 1, 1) for v in dk.folded(T["bn_a"], c))
        if dk.expand_fold(case):
            u = torch.einsum("ncthw,mc->nmthw", x, (T["wa"] * sa.view(-1, 1)).to(dtype).float()) + ba
        else:
            u = torch.einsum("ncthw,mc->nmthw", x, T["wa"].to(dtype).float()) * sa + ba
        e = u if no_relu else torch.relu(u)
        x = e if unrounded_e else e.to(dtype).float()
    w, scale, bias = (v.float() for v in dk.effective_taps(case))  # (values of the fp32 / bf16 grid: exact)
    if bf16_taps:
        w = w.to(torch.bfloat16).float()
    if drop_tap:
        w = w.clone()
        w[:, 0, kt // 2, kh // 2, kw // 2] = 0.0
    if tail_taps:
        g0 = c // 8 * 8
        w = w.clone()
        w[g0:] = w[g0 - 8:g0 - 8 + (c - g0)]
    n, _, t, h, wd = x.shape
    xp = F.pad(x, (pw, pw, ph, ph, pt, pt))
    if halo_wrap:   # the left halo column of row h holds the last element of row h - 1
        xp[:, :, pt:pt + t, ph + 1:ph + h, pw - 1] = x[:, :, :, :h - 1, wd - 1]
    if clip_leak:   # frame -1 of clip 1 holds clip 0's last frame
        xp[1, :, pt - 1, ph:ph + h, pw:pw + wd] = x[0, :, t - 1]
    pre = F.conv3d(xp, w, None, case.s, 0, groups=c) * scale.view(1, -1, 1, 1, 1) + bias.view(1, -1, 1, 1, 1)
    act = dk.ACT[case.act]
    out = torch.zeros(n, *pre.shape[2:], cp, dtype=dtype)
    out[..., :c] = act(pre).permute(0, 2, 3, 4, 1).to(dtype)
    pool = gate = None
    if case.pool:
        src = act(pre) if pool_after_act else pre
        if dk.operand_model(case)[1]:
            src = src.to(torch.bfloat16).float()
        pool = torch.zeros(n, 2, cp)
        pool[:, 0, :c] = src.sum(dim=(2, 3, 4))
    if case.se:
        mean = pool[:, 0, :c] * (1.0 / pre[0, 0].numel())
        gate = torch.zeros(n, cp)
        gate[:, :c] = torch.sigmoid(torch.relu(mean @ T["w1"].t() + T["b1"]) @ T["w2"].t() + T["b2"])
    return dk.Ran(out, pool, gate), pre


def _rows(out):
    return out.view(-1, out.shape[-1])


def _must_fail(case, ran, what):
    with pytest.raises(AssertionError):
        dk.check(case, ran, what)
    return 1


@pytest.mark.parametrize("case", dk.CASES, ids=IDS)
def test_bound_holds_for_fp32_accumulation_and_fails_on_subtle_faults(case):
    good, pre = _emulate(case)
    assert dk.check(case, good, "fp32 emulation") <= 1.0
    n, (to, ho, wo), c, cp = case.nthw[0], dk.out_extent(case), case.c, dk.round_up(case.c, 8)
    m = n * to * ho * wo
    tried = 0

    def with_out(out):
        return dk.Ran(out, good.pool, good.gate)

    # one tap dropped for the outputs of ONE frame at a T-chunk boundary (the first frame of the second chunk; of a single chunk the last), one 8-channel group
    tc = dk.t_chunk(case)
    tb = tc if tc and tc < to else to - 1
    bad = good.out.clone()
    bad[0, tb, :, :, :8] = _emulate(case, drop_tap=True)[0].out[0, tb, :, :, :8]
    tried += _must_fail(case, with_out(bad), "one tap dropped in one frame")
    # the left halo column reads the previous row's last element instead of zero
    if case.p[2] >= 1 and case.nthw[2] >= 2:
        tried += _must_fail(case, _emulate(case, halo_wrap=True)[0], "left halo column wraps")
    # frame -1 of clip 1 reads clip 0's last frame instead of zero
    if case.p[0] >= 1:
        tried += _must_fail(case, _emulate(case, clip_leak=True)[0], "clip 0's last frame under clip 1")
    # the partial last channel group uses the previous group's taps
    if c % 8 and c > 8:
        tried += _must_fail(case, _emulate(case, tail_taps=True)[0], "previous group's taps")
    # one position holds its neighbour's value
    bad = good.out.clone()
    _rows(bad)[m // 2 + 1] = _rows(good.out)[m // 2]
    tried += _must_fail(case, with_out(bad), "position holds its neighbour's value")
    # a padded channel holds 2^-100; the last row is NaN
    if cp > c:
        bad = good.out.clone()
        bad[0, 0, 0, 0, -1] = 2.0 ** -100
        tried += _must_fail(case, with_out(bad), "padded channel not zero")
    bad = good.out.clone()
    _rows(bad)[m - 1] = float("nan")
    tried += _must_fail(case, with_out(bad), "last row unwritten")
    if case.pool:
        # one position counted twice; the last ragged column left out; the sums taken after the activation; a partial row left unwritten
        bad = good.pool.clone()
        bad[0, 0, :c] += pre[0, :, to // 2, ho // 2, wo // 2]
        tried += _must_fail(case, dk.Ran(good.out, bad, good.gate), "pool: one position twice")
        bad = good.pool.clone()
        bad[:, 0, :c] -= pre[..., wo - 1].sum(dim=(2, 3))
        tried += _must_fail(case, dk.Ran(good.out, bad, good.gate), "pool: last column left out")
        if case.act != "none":
            tried += _must_fail(case, dk.Ran(good.out, _emulate(case, pool_after_act=True)[0].pool, good.gate), "pool: after the activation")
        bad = good.pool.clone()
        bad[n - 1, 1, cp - 1] = float("nan")
        tried += _must_fail(case, dk.Ran(good.out, bad, good.gate), "pool: a padded channel of the last row unwritten")
    if case.se:
        bad = good.gate.clone()
        bad[:, :c] = good.gate[:, :c].roll(1, 0)
        tried += _must_fail(case, dk.Ran(good.out, good.pool, bad), "gate of the neighbouring clip")
    if case.expand:
        tried += _must_fail(case, _emulate(case, unrounded_e=True)[0], "intermediate not rounded to bf16")
        tried += _must_fail(case, _emulate(case, no_relu=True)[0], "no ReLU on the intermediate")
    # weights rounded to bf16 where the model says none: an fp32 row must see it; so does every bf16 VALU-family row of this table (where
    # |ref| is small the bound is the accumulation term alone, far below a weight's bf16 rounding)
    if dk.operand_model(case)[0] == "none":
        tried += _must_fail(case, _emulate(case, bf16_taps=True)[0], "taps rounded to bf16")
    assert tried >= 3
