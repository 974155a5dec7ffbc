"""CPU: the table of tests/stem_kernel_cases.py, checked without a GPU (the library is loaded for its geometry probes only) -- (a) every
row reaches exactly the kernel instance it names and the table holds the instances and shapes its docstring promises, (b) the table claims
every ``first_conv`` / ``stem`` launch of the default plans (the ledger) and (c) every name ``PlanBuilder.first_conv`` / ``x3d_stem`` print
over a sweep of compute dtype, clip dtype, channels, windows and switches (the sweep ledger: a name a plan can print and no row runs is a
launch nobody has seen succeed), (d) the fp64 reference agrees with conv3d (+ the depthwise conv_t) + eval-mode BatchNorm3d on the same
rounded operands, (e) the bound holds for an fp32-accumulating emulation of a correct kernel on every row and FAILS on nine ways a
first-layer kernel goes subtly wrong, in every family each applies to.

The two rounding variants the model rules out, as this file's emulation sees them (``test_rounding_variants_are_measured``; reported, not
required): the VALU stem WITHOUT the rounding of its 24-channel intermediate is told apart on every bf16 row (err / bound 13 .. 1800) and
is the same kernel on the f32 rows (0.02 .. 0.06); the matrix-core stem with separately rounded factors rnd(w_t) * rnd(w_xy) instead of
rnd(w_t * w_xy) is told apart on every row (err / bound 54 .. 270)."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import stem_kernel_cases as sk
import train_kernel_cases as tk
from test_cpu_conv_kernel_cases import default_plan_meta

F64 = torch.float64
IDS = [c.id for c in sk.CASES]
KINDS = ("first_conv", "stem")
FAMILIES = ("first_conv_kernel", "first_conv_mfma_kernel", "x3d_stem_kernel", "x3d_stem_mfma_kernel")
TINS, TOUTS = ("f32", "bf16", "u8"), ("f32", "bf16")


def _claimed(cases=sk.CASES):
    return {part for c in cases for part in c.expect.split("+")}


# ------------------------------------------------------------------------------------------------- (a) instance names
@pytest.mark.parametrize("case", sk.CASES, ids=IDS)
def test_every_row_reaches_the_instance_it_names(case):
    with sk.switches(case):
        b = sk.build(case, "cpu")
    assert b.name == case.expect, f"{case.id}: the row runs {b.name}, its label says {case.expect}"
    want = ("first_conv", "dwconv") if sk.is_pair(case) else ("stem",) if case.kind == "stem" else ("first_conv",)
    assert b.kinds == want and len(b.pb.ops) == len(want)
    assert b.pb.in_affine == (sk.AFFINE if case.norm else (1.0, 0.0))


def test_rows_cover_what_the_table_promises():
    """Every instance a builder call can reach; N = 2 everywhere; per family the planes of the docstring, padded output channels, uint8 rows
    with integers 0 .. 255, a grey row that normalises and one that keeps (1, 0)."""
    names = {c.expect.replace("[grey]", "") for c in sk.CASES}
    want = {f"first_conv_kernel<{a},{b},{cop}>" for a in TINS for b in TOUTS for cop in (8, 16, 24, 32, 48, 64)}
    want |= {f"first_conv_mfma_kernel<{a},{nt},{ks}>" for a in TINS for nt in (1, 2) for ks in (11, 5, 4, 2)}
    want |= {f"x3d_stem_kernel<{a},{b},24{g}>" for a in ("f32", "bf16") for b in TOUTS for g in ("", ",grey")} | {f"x3d_stem_kernel<u8,{b},24,grey>" for b in TOUTS}
    want |= {f"x3d_stem_mfma_kernel<{a},{c}>" for a in TINS for c in (1, 3)}
    assert want <= names, sorted(want - names)
    for a in TINS:  # the two first-conv kernels on grey AND three-channel clips of every input dtype and both output dtypes
        for b in TOUTS:
            assert {c.cin for c in sk.CASES if c.expect.startswith(f"first_conv_kernel<{a},{b},")} == {1, 3}
        assert {c.cin for c in sk.CASES if c.expect.startswith(f"first_conv_mfma_kernel<{a},")} == {1, 3}
    fam = {}
    for c in sk.CASES:
        assert c.nthw[0] == 2
        if not sk.is_pair(c):
            fam.setdefault(sk.family(c), []).append(c)
        if c.x == "u8" or c.norm:
            x = sk.tensors(c.id)["x"].float()
            assert 0 <= float(x.min()) < 16 and 240 < float(x.max()) <= 255 and bool((x == x.round()).all())  # (above 127: a signed read shows)
    assert set(fam) == set(FAMILIES)
    planes = {"first_conv_kernel": {sk.A, sk.B, sk.C_, sk.D}, "first_conv_mfma_kernel": {sk.MA, sk.MB, sk.MC, sk.MD},
              "x3d_stem_kernel": {sk.SA, sk.SB, sk.SC, sk.SD},
              "x3d_stem_mfma_kernel": {(7, 18, 24), (1, 16, 16), (3, 10, 132), (2, 8, 116), (5, 6, 228), (6, 9, 20), (13, 9, 20)}}
    for name, rows in fam.items():
        assert planes[name] <= {c.nthw[1:] for c in rows}, f"{name}: {planes[name] - {c.nthw[1:] for c in rows}}"
        assert any(c.cout % 8 for c in rows) and any(c.cout % 8 == 0 for c in rows), f"{name}: padded output channels"
        grey = [c for c in rows if c.cin == 1]
        assert any(c.norm for c in grey) and any(not c.norm for c in grey), f"{name}: a grey row that normalises and one that keeps (1, 0)"
        assert any(c.x == "u8" and c.norm for c in rows), f"{name}: a uint8 row through the grey pipeline"
    fc = fam["first_conv_kernel"]
    assert {c.k for c in fc} == {(7, 7), (3, 3), (5, 5)} and {c.cout for c in fc} >= {6, 12, 20, 30, 45, 64}
    assert {c.k for c in fam["first_conv_mfma_kernel"]} == {(7, 7), (3, 3)} and {c.cout for c in fam["first_conv_mfma_kernel"]} >= {20, 24, 33, 45, 64}
    # the (1,5,5) rows at a width the matrix-core kernel would take, no switch: bf16, three channels and grey, one and two channel tiles
    k5 = [c for c in fc if c.k == (5, 5) and c.dtype == "bf16" and c.nthw[3] % 4 == 0 and not c.env]
    assert {c.cin for c in k5} == {1, 3} and {c.cout > 32 for c in k5} == {True, False}
    assert len([c for c in sk.CASES if sk.is_pair(c)]) >= 1


# ------------------------------------------------------------------------------------------------- (b) the ledger
def _default_plan_names():
    seen = {}
    for name, m in default_plan_meta():
        if m["kind"] in KINDS:
            seen.setdefault(m["kernel"], f"{name}: {m['shape']}")
    return seen


def _unclaimed(seen, claimed):
    return {k: v for k, v in seen.items() if k not in claimed}


def test_ledger_every_first_layer_instance_of_the_default_plans_has_a_row():
    seen = _default_plan_names()
    assert len(seen) >= 6, "the collection itself broke"
    missing = _unclaimed(seen, _claimed())
    assert not missing, "instances a default plan launches and no row of tests/stem_kernel_cases.py runs:\n" + "\n".join(f"  {k}   ({v})" for k, v in missing.items())


def test_ledger_notices_a_row_that_is_gone():
    """With one claimed production instance taken out of the table the ledger names exactly that instance."""
    victim = "x3d_stem_mfma_kernel<u8,1>"
    assert list(_unclaimed(_default_plan_names(), _claimed([c for c in sk.CASES if c.expect != victim]))) == [victim]


# ------------------------------------------------------------------------------------------------- (c) the sweep ledger
def _sweep():
    """{name: where first printed} over compute dtype x clip dtype x C in {1, 3} x windows kh, kw in 1 .. 7 at stride (1,2,2) x the three
    switches; first convs of 20 and 45 output channels (one and two 32-channel tiles), a stem of 20."""
    from protoasnet_amd import _lib
    from protoasnet_amd.plan import PlanBuilder

    cpu, seen = torch.device("cpu"), {}
    convs = {(kh, kw, co): nn.Conv3d(3, co, (1, kh, kw), sk.S2, (0, kh // 2, kw // 2), bias=False) for kh in range(1, 8) for kw in range(1, 8) for co in (20, 45)}
    conv_t, bn = nn.Conv3d(20, 20, (5, 1, 1), 1, (2, 0, 0), groups=20, bias=False), nn.BatchNorm3d(20).eval()
    clear = {k: None for k in os.environ if k.startswith("PASN_")}
    for env in ({}, {"PASN_NO_FC_MFMA": "1"}, {"PASN_NO_STEM_MFMA": "1"}, {"PASN_NO_STEM": "1"}):
        with _lib.tuning_env(**dict(clear, **env)), torch.no_grad():
            for dtype in TOUTS:
                for xd in TINS:
                    for cin in (1, 3):
                        for (kh, kw, co), conv in convs.items():
                            pb = PlanBuilder(cpu, sk.DT[dtype], sk.XDT[xd])
                            pb.first_conv(pb.input((2, cin, 2, 12, 24)), conv, None, "relu")
                            if co == 20:
                                pb.x3d_stem(pb.input((2, cin, 2, 12, 24)), conv, conv_t, bn)
                            for m in pb.meta:
                                if m["kind"] in KINDS:
                                    seen.setdefault(m["kernel"], f"compute {dtype}, clip {xd} x {cin}, window {kh}x{kw}, {co} channels, {env}")
    return seen


def test_sweep_ledger_every_printable_name_has_a_row():
    seen = _sweep()
    assert len(seen) >= 50 and any(k.startswith("x3d_stem_mfma_kernel") for k in seen) and any(k.startswith("first_conv_mfma_kernel") for k in seen)
    missing = _unclaimed(seen, _claimed())
    assert not missing, "names a plan prints and no row of tests/stem_kernel_cases.py runs:\n" + "\n".join(f"  {k}   ({v})" for k, v in sorted(missing.items()))


def test_probe_admits_only_windows_the_launcher_has_an_instance_for():
    """``pasn_first_conv_mfma_slot`` over kh, kw in 1 .. 7, pw in 0 .. 4, C in {1, 3}, 24 and 45 channels at W = 24: an admitted layer has
    ceil(C * kh / 2) in {11, 5, 4, 2}, the launcher's list; the 7x7 and 3x3 stems stay admitted."""
    import ctypes

    from protoasnet_amd import _lib
    from protoasnet_amd.plan import Act, PlanBuilder

    lib, bf16 = _lib.lib(), _lib.dtype_code(torch.bfloat16)
    admitted = set()
    with _lib.tuning_env(**{k: None for k in os.environ if k.startswith("PASN_")}):
        for cin in (1, 3):
            for kh in range(1, 8):
                for kw in range(1, 8):
                    for pw in range(5):
                        for co in (24, 45):
                            x = Act(2, 2, 12, 24, cin, cin, -1, planar=True)
                            k, p = (1, kh, kw), (0, kh // 2, pw)
                            d = PlanBuilder._probe_desc(x, PlanBuilder._geom(x, co, k, sk.S2, p), k, sk.S2, p, "relu")
                            if lib.pasn_first_conv_mfma_slot(ctypes.byref(d), bf16, bf16) >= 0:
                                admitted.add((cin, kh))
    assert {(cin * kh + 1) // 2 for cin, kh in admitted} == {11, 5, 4, 2}, sorted(admitted)
    assert {(3, 7), (3, 3), (1, 7), (1, 3)} <= admitted
    # kh = 1 on three channels has ceil(3 / 2) = 2 k-steps too, but the kernel's row walk wraps once per step (first_conv_mfma.hip:139-142)
    assert all(kh >= 2 for _, kh in admitted), sorted(admitted)


# ------------------------------------------------------------------------------------------------- (d) the reference
def _bn64(c, q):
    bn = nn.BatchNorm3d(c).double().eval()
    with torch.no_grad():
        bn.weight.copy_(q["gamma"]), bn.bias.copy_(q["beta"]), bn.running_mean.copy_(q["mean"]), bn.running_var.copy_(q["var"])
    return bn


@pytest.mark.parametrize("case", sk.CASES, ids=IDS)
def test_reference_is_within_one_rounding_of_the_fold_of_conv3d_and_batch_norm(case):
    """Independent restatement: F.conv3d (+ the depthwise conv_t on the rounded intermediate) + nn.BatchNorm3d.eval() in fp64 on the same
    rounded operands.  The two agree to the accuracy of the launch's fp32 fold of the norm (a few 2^-24 of |scale| and of |beta| + |mean
    scale| < 4).  The loaded clip is held to the grey pipeline's formula, (x / 255 - 0.099) / 0.171, and the bf16 stem rows to the cap on
    the share of intermediate elements at risk."""
    dtype, T, fam = sk.DT[case.dtype], sk.tensors(case.id), sk.family(case)
    R, W = sk.reference(case.id), sk.effective_weights(case)
    x, flip = sk.loaded_input(case)
    assert (flip is not None) == case.norm
    op = torch.bfloat16 if sk.mfma_family(case) else torch.float32
    want_x = (T["x"].to(F64) / 255.0 - 0.099) / 0.171 if case.norm else T["x"].to(F64)
    assert bool(((x - want_x).abs() <= (2.0 ** -8 if op == torch.bfloat16 else 2.0 ** -21) * want_x.abs() + 1e-7).all())
    assert bool((x == tk.rnd(x, op)).all())
    with torch.no_grad():
        if fam == "x3d_stem_kernel":
            e = tk.rnd(F.conv3d(x, W["w"], None, sk.S2, (0,) + case.p), dtype)
            y = F.conv3d(e, W["wt"], None, 1, (2, 0, 0), groups=case.cout)
            assert (R["at_risk"] == 1.0) if case.dtype == "f32" else (R["at_risk"] < 0.05), f"{case.id}: {R['at_risk']:.4f} of the intermediate at risk"
        else:
            y = F.conv3d(x, W["w"], None, sk.S2, ((2,) if fam == "x3d_stem_mfma_kernel" else (0,)) + case.p)
        want = sk.ACT[case.act](_bn64(case.cout, T["bn"])(y))
    assert want.shape == R["ref"].shape == (2, case.cout) + sk.out_extent(case)
    tol = 1.1 * 2.0 ** -20 * (R["A"] + 4)
    err = (R["ref"] - want).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    assert bool((R["bound"] > 0).all()) and 0.2 < float((R["pre"] > 0).double().mean()) < 0.8


# ------------------------------------------------------------------------------------------------- (e) the bound discriminates
def _emulate(case, drop_tap=False, pad_b=False, last_col=False, signed=False, clamp_t=False, shift_t=False, unrounded_e=False, split_w=False):
    """What a correct kernel computes, with fp32 accumulation: torch fp32 convs on the rounded operands of the table, the VALU stem's
    intermediate rounded to T, the output rounded to the dtype -- in the launch's layout [N][To][Ho][Wo][Cout_p].  The keywords are the
    faults and the two rounding variants of the tests below."""
    dtype, fam = sk.DT[case.dtype], sk.family(case)
    c, cp, (ph, pw) = case.cout, sk.round_up(case.cout, 8), case.p
    W = sk.effective_weights(case)
    w, scale, bias = W["w"].float(), W["scale"].float().view(1, -1, 1, 1, 1), W["bias"].float().view(1, -1, 1, 1, 1)
    if split_w:  # rnd(w_t) * rnd(w_xy): the factors rounded, not the product
        m = sk.modules(case)
        wxy = sk._summed(case, m["conv"].weight).to(torch.bfloat16).float()
        wt5 = m["conv_t"].weight.detach().float().reshape(c, 5).to(torch.bfloat16).float()
        w = (wt5[:, :, None, None, None] * wxy[:, None]).permute(0, 2, 1, 3, 4).contiguous()
    if drop_tap:  # the tap of median magnitude, of one output channel
        i = int(w.abs().flatten().argsort()[w.numel() // 2])
        w = w.flatten().clone()
        w[i] = 0.0
        w = w.view(W["w"].shape)
    x = sk.loaded_input(case, signed=signed)[0].float()
    if last_col:
        x = x.clone()
        x[..., -1] = 0.0
    op = torch.bfloat16 if sk.mfma_family(case) else torch.float32
    padv = float(torch.tensor(sk.affine(case)[1]).to(op)) if pad_b else 0.0  # what normalising a padded zero gives
    xp = F.pad(x, (pw, pw, ph, ph), value=padv)
    tpad = (0, 0, 0, 0, 1, 3) if shift_t else (0, 0, 0, 0, 2, 2)             # shift_t: output frame t from frames t - 1 .. t + 3
    if fam == "x3d_stem_kernel":
        e = F.conv3d(xp, w, None, sk.S2)
        e = e if unrounded_e else e.to(dtype).float()
        et = F.pad(e, tpad)
        if clamp_t:  # the frame after the last one holds the last frame
            et[:, :, tpad[4] + e.shape[2]] = e[:, :, -1]
        pre = F.conv3d(et, W["wt"].float(), None, 1, 0, groups=c) * scale + bias
    elif fam == "x3d_stem_mfma_kernel":
        xt = F.pad(xp, tpad, value=padv)
        if clamp_t:
            xt[:, :, tpad[4] + xp.shape[2]] = xp[:, :, -1]
        pre = F.conv3d(xt, w, None, sk.S2) * scale + bias
    else:
        pre = F.conv3d(xp, w, None, sk.S2) * scale + bias
    out = torch.zeros(pre.shape[0], *pre.shape[2:], cp, dtype=dtype)
    out[..., :c] = sk.ACT[case.act](pre).permute(0, 2, 3, 4, 1).to(dtype)
    return out


def _fails(case, out, what):
    try:
        sk.check(case, out, what)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def emulated():
    return {c.id: _emulate(c) for c in sk.CASES}


@pytest.mark.parametrize("case", sk.CASES, ids=IDS)
def test_bound_holds_for_fp32_accumulation(case, emulated):
    assert sk.check(case, emulated[case.id], "fp32 emulation") <= 1.0


def _mutants(case, good):
    """{fault: output} of every fault that applies to the row."""
    fam, (to, ho, wo), c = sk.family(case), sk.out_extent(case), case.cout
    M = {"one tap of one output channel zeroed": _emulate(case, drop_tap=True), "the last input column read as zero": _emulate(case, last_col=True)}
    if case.norm:
        M["the pad region holds in_b"] = _emulate(case, pad_b=True)
    if ho % 4 or not sk.mfma_family(case):  # (the matrix-core kernels: the last row of a ragged 4-row tile; the VALU ones: the last row)
        bad = good.clone()
        bad[:, :, ho - 1] = float("nan")
        M["the last output row left unwritten"] = bad
    bad = good.clone()
    bad[1] = good[0]
    M["clip 1 computed from clip 0"] = bad
    if case.x == "u8":
        M["uint8 read as signed"] = _emulate(case, signed=True)
    if good.shape[-1] > c:  # no tail mask and a bias row that is not padded with zeros: the neighbouring channel's act(bias)
        bad = good.clone()
        bad[..., c:] = sk.ACT[case.act](sk.effective_weights(case)["bias"][c - 1].float()).to(good.dtype)
        M["padded channels hold act(bias)"] = bad
    if case.kind == "stem":
        M["the frame after the last one clamped to the last frame"] = _emulate(case, clamp_t=True)
        M["output frame t built from frames t - 1 .. t + 3"] = _emulate(case, shift_t=True)
    return M


def test_bound_fails_on_nine_subtle_faults_in_every_family(emulated):
    """Each fault fails ``check`` on at least one row of every family it applies to (a pair row counts for ``x3d_stem_kernel``)."""
    verdicts = {}
    for case in sk.CASES:
        for what, out in _mutants(case, emulated[case.id]).items():
            verdicts.setdefault((what, sk.family(case)), []).append(_fails(case, out, what))
    faults = {w for w, _ in verdicts}
    assert len(faults) == 9, sorted(faults)
    for what in faults:
        fams = {f for w, f in verdicts if w == what}
        assert fams == ({"x3d_stem_kernel", "x3d_stem_mfma_kernel"} if "frame" in what else set(FAMILIES)), f"{what}: {sorted(fams)}"
    passed = {k: v for k, v in verdicts.items() if not any(v)}
    assert not passed, "faults the bound lets through in a whole family:\n" + "\n".join(f"  {w} ({f}: {len(v)} rows)" for (w, f), v in passed.items())
    # the faults that change every element of a region fail on EVERY row they apply to
    for what in ("the last output row left unwritten", "clip 1 computed from clip 0", "the pad region holds in_b", "uint8 read as signed", "the last input column read as zero",
                 "output frame t built from frames t - 1 .. t + 3"):
        for fam in FAMILIES:
            v = verdicts.get((what, fam))
            assert v is None or all(v), f"{what}: passes on {v.count(False)} of {len(v)} rows of {fam}"


def test_rounding_variants_are_measured():
    """The two rounding variants of the module docstring, whose numbers come from here: measured, not required to fail."""
    for case in sk.CASES:
        R, fam = sk.reference(case.id), sk.family(case)
        if fam not in ("x3d_stem_kernel", "x3d_stem_mfma_kernel"):
            continue
        out = _emulate(case, unrounded_e=True) if fam == "x3d_stem_kernel" else _emulate(case, split_w=True)
        ratio = float(((out[..., :case.cout].permute(0, 4, 1, 2, 3).to(F64) - R["ref"]).abs() / R["bound"]).max())
        assert ratio < 0.1 if (fam, case.dtype) == ("x3d_stem_kernel", "f32") else ratio == ratio, f"{case.id}: {ratio:.3g}"  # T = f32: the same kernel
