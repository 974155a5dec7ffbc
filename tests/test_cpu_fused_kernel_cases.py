"""CPU: the table of tests/fused_kernel_cases.py, checked without a GPU -- (a) every row reaches exactly the kernel instance it names (a
plan built on the CPU under the row's switches, the name decoded from the library's own variant probes), the FOUR tables together claim
every (kind, kernel) the eight default plans and the head chains launch, and no width on a grid decodes to an instance the sources do not
instantiate; (b) the fp64 reference agrees with an independent restatement through F.conv3d + eval-mode BatchNorm3d, stage by stage; (c)
the bound holds for an fp32-accumulating emulation of every launch and FAILS on the ways a fused kernel goes subtly wrong.

``maxpool`` is the one launch kind no table claims: it has no arithmetic to bound (a maximum of stored values is exact) and is compared
bit for bit with torch in tests/test_gpu_kernels.py::test_maxpool."""
import ctypes
import functools
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_kernel_cases as ck
import dw_kernel_cases as dk
import fused_kernel_cases as fk
import stem_kernel_cases as sk  # noqa: F401  (its rows are claimed through test_cpu_stem_kernel_cases._claimed)
import train_kernel_cases as tk
from test_cpu_conv_kernel_cases import _default_plan_names as conv_plan_names
from test_cpu_conv_kernel_cases import default_plan_meta
from test_cpu_stem_kernel_cases import _claimed as stem_claimed

F64, BF16 = torch.float64, torch.bfloat16
IDS = [c.id for c in fk.CASES]
FUSED_KINDS = ("conv+shortcut", "conv+se", "conv_pair", "conv_pair+se", "block", "block+expand", "se_gate")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "protoasnet_amd", "csrc")


# ------------------------------------------------------------------------------------------------- (a) instance names
@functools.lru_cache(maxsize=None)
def built_on_cpu(case_id):
    case = fk.BY_ID[case_id]
    with fk.switches(case):
        return fk.build(case, "cpu")


@pytest.mark.parametrize("case", fk.CASES, ids=IDS)
def test_every_row_reaches_the_instance_it_names(case):
    b = built_on_cpu(case.id)
    assert (b.kind, b.name) == (fk.kind(case), case.expect), f"{case.id}: the row runs {b.kind} {b.name}, its label says {fk.kind(case)} {case.expect}"
    assert len(b.pb.ops) == (2 if case.form in fk.SE_FORMS else 1)
    if case.form in fk.SE_FORMS:
        assert b.pool[1] >= 2, f"{case.id}: {b.pool[1]} pool partial row per clip"


def test_rows_cover_what_the_table_promises():
    fam = {}
    for c in fk.CASES:
        fam.setdefault(fk.family(c), []).append(c)
    assert set(fam) == {"pwconv_persist_kernel", "pwconv_ws_kernel[se]", "pwconv_ws_kernel", "pwconv_xpair_kernel", "x3d_pe_kernel", "x3d_pe_kernel[se]",
                        "x3d_edp_kernel", "se_gate_kernel"}
    names = {c.expect for c in fk.CASES}
    assert {f"pwconv_xpair_kernel<{a},{b},{x}>" for a in (8, 14) for b in (4, 6) for x in ("false", "true")} <= names
    assert {f"x3d_pe_kernel<28,12,{s},{m}>" for s in ("false", "true") for m in (2, 4)} <= names
    assert {f"pwconv_persist_kernel<bf16,{k}>" for k in ("4,1,false,2", "8,2,false,2", "8,2,false,4")} <= names
    for c in fk.CASES:
        n, (to, ho, wo) = c.nthw[0], fk.out_thw(c)
        assert n >= 2 and (n * to * ho * wo) % 32 != 0, f"{c.id}: rows are a multiple of the tile"
        if c.form != "edp":
            assert (to * ho * wo) % 32 != 0, f"{c.id}: no tile straddles two clips"
    for name, rows in fam.items():
        if name in ("x3d_edp_kernel", "se_gate_kernel"):
            continue
        assert any(c.c0 % 8 for c in rows), f"{name}: no partial 8-channel chunk"
        assert any(ch % 8 for c in rows for _, ch in fk.outputs(c)), f"{name}: no padded output channels"
    assert {c.gate for c in fam["pwconv_persist_kernel"]} == {True, False} and all((c.nthw[2] % 2, c.nthw[3] % 2) == (1, 1) for c in fam["pwconv_persist_kernel"])
    assert any(not c.res for c in fam["pwconv_ws_kernel[se]"]) and any(",2,true" in c.expect for c in fam["pwconv_ws_kernel[se]"])
    edp = fam["x3d_edp_kernel"]
    assert {c.nthw[1] for c in edp} >= {1, 2, 3} and any(c.nthw[0] * ((c.nthw[1] + 1) // 2) > 256 for c in edp) and any(c.c1 % 8 for c in edp)
    pe = fam["x3d_pe_kernel"] + fam["x3d_pe_kernel[se]"]
    assert any(8192 < c.nthw[0] * c.nthw[1] * c.nthw[2] * c.nthw[3] <= 8448 for c in pe)
    assert {c.cse % 4 == 0 for c in fam["se_gate_kernel"]} == {True, False}  # se_gate_fast_kernel and se_gate_kernel


# ------------------------------------------------------------------------------------------------- (a) the ledger of all four tables
def _launched():
    """{(kind, kernel): where} over the eight default plans and the heads' add-on / occurrence chains (kind ``conv``), ``maxpool`` left out."""
    seen = {}
    for name, m in default_plan_meta():
        if m["kind"] != "maxpool":
            seen.setdefault((m["kind"], m["kernel"]), f"{name}: {m['shape']}")
    for kernel, where in conv_plan_names().items():
        seen.setdefault(("conv", kernel), where)
    return seen


def _claimed(fused_rows):
    plain = {c.expect for c in ck.CASES} | {c.expect for c in dk.CASES} | set(stem_claimed())
    fused = {(fk.kind(c), c.expect) for c in fused_rows}
    return lambda key: (key in fused) if key[0] in FUSED_KINDS else (key[1] in plain)


@pytest.fixture(scope="module")
def launched():
    from protoasnet_amd import _lib

    with _lib.tuning_env(**{k: None for k in os.environ if k.startswith("PASN_")}):
        return _launched()


def test_ledger_the_four_tables_claim_every_launch_of_the_default_plans(launched):
    kinds = {k for k, _ in launched}
    assert len(launched) >= 60 and set(FUSED_KINDS) - {"block"} <= kinds, f"the collection itself broke: {sorted(kinds)}"  # (no default plan ends a stage on x3d_edp)
    claimed = _claimed(fk.CASES)
    missing = {k: v for k, v in launched.items() if not claimed(k)}
    assert not missing, "launches of a default plan that no row of the four tables runs:\n" + "\n".join(f"  {k}   ({v})" for k, v in missing.items())


def test_ledger_notices_a_row_that_is_gone(launched):
    victim = "x3d_edp_kernel<12,28,true>"
    claimed = _claimed([c for c in fk.CASES if c.expect != victim])
    assert [k for k in launched if not claimed(k)] == [("block+expand", victim)]


# ------------------------------------------------------------------------------------------------- (a) no width decodes to a missing instance
def _instantiated():
    """The instances the launchers' dispatch macros name, read from the sources."""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("pwconv_ws.hip", "pwconv_xpair.hip", "pwconv.hip")}
    tf = ("false", "true")
    ws = {(int(k), mt) for k in re.findall(r"PASN_WS1\((\d+)\)", src["pwconv_ws.hip"]) for mt in (1, 2)}
    ws |= {(int(k), int(mt)) for k, mt in re.findall(r"PASN_WS2\((\d+), (\d+)\)", src["pwconv_ws.hip"])}
    names = {f"pwconv_ws_kernel<{k},{mt},true,{r}>[se]" for k, mt in ws for r in tf}
    for k, mt, x, r, k2 in re.findall(r"PASN_WS4\((\d+), (\d+), (true|false), (true|false), (\d+)\)", src["pwconv_ws.hip"]):
        names.add(f"pwconv_ws_kernel<{k},{mt},{x},{r},{k2}>")
        if x == "true":
            names.add(f"pwconv_ws_kernel<{k},{mt},{x},{r},{k2}>[se]")
    names |= {f"pwconv_xpair_kernel<{a},{b},{x}>" for a, b in re.findall(r"PASN_XP_XF\((\d+), (\d+)\)", src["pwconv_xpair.hip"]) for x in tf}
    names |= {f"pwconv_persist_kernel<bf16,{k},{n},false,{k2}>" for k, n, k2 in re.findall(r"PASN_PW3\((\d+), (\d+), false, (\d+), \*sc\)", src["pwconv.hip"])}
    assert len(ws) == 13 and len(names) == 26 + 6 + 8 + 3, (len(ws), len(names))
    return names


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_no_width_decodes_to_an_instance_that_does_not_exist(res):
    """Cin_p 48 .. 448 in steps of 8 x a few output widths under PASN_WS=2 (and both pair switches): whatever the probes answer decodes to
    an instance the sources instantiate.  (The former Python formulas printed ``pwconv_ws_kernel<10,..>`` for nine and ten k-steps and
    MT = 1 where the geometry takes 2.)"""
    from protoasnet_amd import _lib
    from protoasnet_amd.plan import Act, PlanBuilder, fused_kernel_name

    lib, code, listed = _lib.lib(), _lib.dtype_code(BF16), _instantiated()
    one, zero, thw = (1, 1, 1), (0, 0, 0), (4, 8, 8)

    def desc(cin, cout, in_swish, frag=1, cin_thw=thw, s=one):
        x, y = Act(2, *cin_thw, cin, cin, -1), Act(2, *thw, cout, fk.round_up(cout, 8), -1)
        return PlanBuilder._probe_desc(x, y, one, s, zero, "relu", in_swish, fk.round_up(cin, 16), fk.round_up(y.Cp, 128), w_frag=frag)

    seen = set()
    clear = {k: None for k in os.environ if k.startswith("PASN_")}
    for env in ({"PASN_WS": "2", "PASN_WSPAIR": "2"}, {"PASN_WS": "2", "PASN_WSPAIR": "0", "PASN_XPAIR_ALL": "1"}):
        with _lib.tuning_env(**dict(clear, **env)):
            for cin_p in range(48, 449, 8):
                for cout in (24, 45, 90, 160, 192):
                    d1 = desc(cin_p, cout, True)
                    v = int(lib.pasn_conv3d_se_variant(ctypes.byref(d1), code, 8, int(res)))
                    assert bool(v) == bool(lib.pasn_conv3d_se_supported(ctypes.byref(d1), code, 8, int(res)))
                    if v:
                        seen.add(fused_kernel_name(v, "bf16", res=res, se=True))
                        if 136 <= cin_p <= 160:
                            assert fused_kernel_name(v, "bf16", res=res, se=True).startswith("pwconv_ws_kernel<12,"), (cin_p, v)
                    if not res:
                        continue
                    for cout2 in (100, 210):
                        d2 = desc(cout, cout2, False)
                        v = int(lib.pasn_conv3d_pair_se_variant(ctypes.byref(d1), ctypes.byref(d2), code, 8))
                        assert bool(v) == bool(lib.pasn_conv3d_pair_se_supported(ctypes.byref(d1), ctypes.byref(d2), code, 8))
                        if v:
                            seen.add(fused_kernel_name(v, "bf16", se=True))
                        for gate in (0, 1):
                            dp = desc(cin_p, cout, bool(gate))
                            v = int(lib.pasn_conv3d_pair_instance(ctypes.byref(dp), ctypes.byref(d2), code, gate))
                            assert v // 10000 == int(lib.pasn_conv3d_pair_variant(ctypes.byref(dp), ctypes.byref(d2), code, gate))
                            if v:
                                seen.add(fused_kernel_name(v, "bf16", transform=bool(gate)))
                    for cx in (24, 40, 48, 72):  # the strided shortcut beside the project conv: row-major weights, input planes 15 x 15 -> 8 x 8
                        dm, dx = desc(cin_p, cout, False, frag=0), desc(cx, cout, False, frag=0, cin_thw=(4, 15, 15), s=(1, 2, 2))
                        v = int(lib.pasn_conv3d_short_variant(ctypes.byref(dm), ctypes.byref(dx), code))
                        assert bool(v) == bool(lib.pasn_conv3d_short_supported(ctypes.byref(dm), ctypes.byref(dx), code))
                        if v:
                            seen.add(fused_kernel_name(v, "bf16"))
    assert seen <= listed, f"names no source instantiates: {sorted(seen - listed)}"
    assert len(seen) >= (16 if res else 8), sorted(seen)  # (the sweep is not empty)


# ------------------------------------------------------------------------------------------------- the fp32 emulation
TILE = {"pwconv_persist_kernel": 32, "x3d_pe_kernel": 32, "x3d_edp_kernel": 49}  # rows of the tile a local fault hits; 64 elsewhere


def _bf(t):
    return t.to(BF16).float()


def _fold(q):
    s, b = fk._fold(q)
    return s.view(1, -1, 1, 1, 1), b.view(1, -1, 1, 1, 1)


def _cl(t5):
    """(N,C,T,H,W) fp32 -> the launch's layout [N][T][H][W][Cp] bf16."""
    return fk._channels_last(t5, fk.round_up(t5.shape[1], 8), BF16, "cpu")


def _stencil(case, T, blocks):
    """The stencil launch ahead of an SE row: its stored output and ``blocks`` pool partial rows per clip (fp32 sums of the pre-activation)."""
    c = case.c0
    s, b = _fold(T["bn_b"])
    pre = F.conv3d(_bf(T["x"]), _bf(T["wb"]), None, 1, 1, groups=c) * s + b
    rows = torch.stack([p.sum(dim=2) for p in pre.flatten(2).tensor_split(blocks, dim=2)], dim=1)  # [N][blocks][C]
    pool = torch.zeros(rows.shape[0], blocks, fk.round_up(c, 8))
    pool[..., :c] = rows
    return _bf(pre), pool


def _gate32(case, T, pool, fault):
    P = case.nthw[1] * case.nthw[2] * case.nthw[3]
    part = pool[..., :case.c0]
    if fault == "pool_row":
        part = part[:, :-1]
    inv = torch.tensor(1.0 / (fk.round_up(P, 128) if fault == "pool_pad" else P), dtype=torch.float32)  # whole 128-row tiles, the largest any of these kernels walks
    hid = torch.relu((part.sum(1) * inv) @ T["fc1_w"].t() + T["fc1_b"])
    return torch.sigmoid(hid @ T["fc2_w"].t() + T["fc2_b"])


def emulate(case, fault=None):
    """What a correct launch computes, with fp32 accumulation, in ``fk.launch``'s format.  ``fault``: one of the global mutations (the test
    splices the tile-local ones from two emulations)."""
    T = fk.tensors(case.id)
    tile = TILE.get(case.expect.split("<")[0], 64)
    outs = {}
    if case.form == "edp":
        return _emulate_edp(case, T, fault)
    x, gate = _bf(T["x"]), None
    if case.form in fk.SE_FORMS:
        x, outs["pool"] = _stencil(case, T, built_on_cpu(case.id).pool[1])
        outs["ys"] = _cl(x)
        gate = _gate32(case, T, outs["pool"], fault)
        if case.form == "gate":
            outs["gate"] = torch.zeros(gate.shape[0], fk.round_up(case.c0, 8))
            outs["gate"][:, :case.c0] = gate
            return outs
    elif case.gate:
        gate = T["gate"]
    if gate is not None:
        if fault == "_gate_roll":
            gate = gate.roll(-1, 0)
        v = x * gate[:, :, None, None, None]
        x = _bf(v * torch.sigmoid(v))
    if fault == "_drop_chunk":
        x = x.clone()
        x[:, case.c0 // 8 * 8:] = 0.0
    s1, b1 = _fold(T["bn1"])
    pre = F.conv3d(x, _bf(T["w1"])) * s1 + b1
    if case.form == "short":
        s2, b2 = _fold(T["bn2"])
        x2 = _bf(T["x2"])
        if fault == "short_col":  # the gather one input column to the right (the last column exists on odd planes only)
            x2 = x2.roll(-1, 4)
        pre = F.conv3d(x2, _bf(T["w2"]), None, fk.S2) * s2 + (F.conv3d(x, _bf(T["w1"])) * s1 + (b1 if fault == "short_bias" else b1 + b2))
    res = _bf(T["res"]) if case.res else 0.0
    y1 = _bf(torch.relu(pre) + res if fault == "res_after" else torch.relu(pre + res))
    outs["y1"] = _cl(y1)
    if case.c2:
        src = _bf(torch.relu(pre)) if fault == "pre_res" else y1
        if fault == "_drop_chunk2":
            src = src.clone()
            src[:, case.c1 // 8 * 8:] = 0.0
        s2, b2 = _fold(T["bn2"])
        outs["y2"] = _cl(_bf(torch.relu(F.conv3d(src, _bf(T["w2"])) * s2 + b2)))
    return outs


def _emulate_edp(case, T, fault):
    x = _bf(T["x"])
    (sa, ba), (sd, bd), (sc, bc) = _fold(T["bn_a"]), _fold(T["bn_b"]), _fold(T["bn1"])
    e = _bf(torch.relu(F.conv3d(x, _bf(T["wa"])) * sa + ba))
    ep = F.pad(e, (1, 1, 1, 1, 1, 1))
    if fault == "t_before":  # the frame before a clip's first one taken from the neighbouring clip instead of zero
        ep[1:, :, 0, 1:-1, 1:-1] = e[:-1, :, -1]
    if fault == "t_after":
        ep[:-1, :, -1, 1:-1, 1:-1] = e[1:, :, 0]
    if fault == "border":    # the zero border replaced by the edge value on the left
        ep[:, :, 1:-1, 1:-1, 0] = e[..., 0]
    pre = F.conv3d(ep, _bf(T["wb"]), None, 1, 0, groups=case.c1) * sd + bd
    d = _bf(pre * torch.sigmoid(pre))
    if fault == "_drop_chunk":
        d = d.clone()
        d[:, case.c1 // 8 * 8:] = 0.0
    u = F.conv3d(d, _bf(T["w1"])) * sc + bc
    y = _bf(torch.relu(u) + x if fault == "res_after" else torch.relu(u + x))
    outs = {"y1": _cl(y)}
    if case.c2:
        s2, b2 = _fold(T["bn2"])
        outs["y2"] = _cl(_bf(torch.relu(F.conv3d(_bf(torch.relu(u)) if fault == "pre_res" else y, _bf(T["w2"])) * s2 + b2)))
    return outs


@functools.lru_cache(maxsize=None)
def good(case_id):
    return emulate(fk.BY_ID[case_id])


# ------------------------------------------------------------------------------------------------- (b) the reference
def _bn64(q):
    return fk._bn(q).double()


def _w(t):
    return tk.rnd(t, BF16)


@pytest.mark.parametrize("case", fk.CASES, ids=IDS)
def test_reference_is_conv3d_and_eval_mode_batch_norm_in_fp64(case):
    """Independent restatement, stage by stage: F.conv3d + nn.BatchNorm3d.eval() (+ F.conv3d(groups = C) + Swish on the ``edp`` rows, the two
    FCs as nn.Conv3d on the SE rows) in fp64 on the same rounded operands.  The reference reads the launch's fp32 fold of each norm, a few
    2^-24 off the fp64 fold relative to |scale| and to |beta| + |mean scale| < 4; on ``edp`` rows that difference may also move an unstored
    intermediate across a rounding boundary, which is what the flip terms of the bound already allow for: they join the tolerance there."""
    T, stored = fk.tensors(case.id), good(case.id)
    R = fk.reference(case, stored)
    m = {k: v.double() for k, v in fk.modules(case).items()}
    with torch.no_grad():
        want = {}
        if case.form == "edp":
            x = _w(T["x"])
            e = tk.rnd(torch.relu(_bn64(T["bn_a"])(F.conv3d(x, _w(T["wa"])))), BF16)
            p = _bn64(T["bn_b"])(F.conv3d(e, _w(T["wb"]), None, 1, 1, groups=case.c1))
            want["y1"] = torch.relu(_bn64(T["bn1"])(F.conv3d(tk.rnd(p * torch.sigmoid(p), BF16), _w(T["w1"]))) + x)
        else:
            x = _w(T["x"])
            gate = T["gate"].to(F64) if case.gate else None
            if case.form in fk.SE_FORMS:
                x = fk.from_cl(stored["ys"], case.c0)
                P = x[0, 0].numel()
                mean = stored["pool"].to(F64)[..., :case.c0].sum(1) / P
                gate = torch.sigmoid(m["fc2"](torch.relu(m["fc1"](mean[:, :, None, None, None]))))[:, :, 0, 0, 0]
                if case.form == "gate":
                    want["gate"] = gate
            if gate is not None:
                v = x * gate[:, :, None, None, None]
                x = tk.rnd(v * torch.sigmoid(v), BF16)
            if case.form != "gate":
                u = _bn64(T["bn1"])(F.conv3d(x, _w(T["w1"])))
                if case.form == "short":
                    u = u + _bn64(T["bn2"])(F.conv3d(_w(T["x2"]), _w(T["w2"]), None, fk.S2))
                want["y1"] = torch.relu(u + _w(T["res"])) if case.res else torch.relu(u)
        if case.c2:
            c_mid = case.c0 if case.form == "edp" else case.c1
            want["y2"] = torch.relu(_bn64(T["bn2"])(F.conv3d(fk.from_cl(stored["y1"], c_mid), _w(T["w2"]))))
    assert set(want) == set(R)
    for k, w in want.items():
        r = R[k]
        err = (r["ref"] - w).abs()
        if k == "gate":
            assert float(err.max()) < 1e-12 and bool((r["bound"] > 0).all())
            continue
        tol = 1.1 * 2.0 ** -20 * (r["A"] + 4)
        if case.form == "edp" and k == "y1":
            tol = tol + (r["bound"] - tk.BF16_STORE * r["ref"].abs())
        assert bool((err <= tol).all()), (k, float(err.max()))
        assert bool((r["bound"] > 0).all())
        pos = float((r["u"] > 0).double().mean())
        assert (0.2 < pos < 0.8) or (case.form == "edp" and k == "y1" and 0.5 < pos < 0.995), (k, pos)
    # the share of operands that may sit on the other side of a rounding boundary (fused_kernel_cases, Bound)
    if case.form == "edp":
        assert R["y1"]["at_risk_e"] < 0.035 and R["y1"]["at_risk"] < 0.5, (R["y1"]["at_risk_e"], R["y1"]["at_risk"])
    else:  # a gate the launch computes itself carries dg (about 2e-5 of the gate at 432 channels: eps ~ 4e-5 against half a bf16 spacing)
        assert all(r["at_risk"] < (2e-2 if case.cse else 2e-3) for r in R.values()), {k: r["at_risk"] for k, r in R.items()}


# ------------------------------------------------------------------------------------------------- (c) the bound discriminates
def _rows(t):
    return t.view(-1, t.shape[-1])


def _must_fail(case, outs, what):
    with pytest.raises(AssertionError):
        fk.check(case, outs, what)
    return what


def _with(outs, **kv):
    bad = {k: v.clone() for k, v in outs.items()}
    bad.update(kv)
    return bad


@pytest.mark.parametrize("case", fk.CASES, ids=IDS)
def test_bound_holds_for_fp32_accumulation_and_fails_on_subtle_faults(case):
    ok = good(case.id)
    assert fk.check(case, ok, "fp32 emulation") <= 1.0
    to, ho, wo = fk.out_thw(case)
    s, m = to * ho * wo, case.nthw[0] * to * ho * wo
    tile = TILE.get(case.expect.split("<")[0], 64)
    tried = []

    def splice(fault, key, lo, hi):
        bad = _with(ok)
        for k in ([key, "y2"] if key == "y1" and "y2" in ok else [key]):
            _rows(bad[k])[lo:hi] = _rows(emulate(case, fault)[k])[lo:hi]
        return bad

    if case.form == "gate":
        tried += [_must_fail(case, emulate(case, f), f) for f in ("pool_row", "pool_pad")]
        bad = _with(ok)
        bad["gate"][0] = ok["gate"][1]
        tried.append(_must_fail(case, bad, "the neighbouring clip's gate"))
        if case.c0 % 8:
            bad = _with(ok)
            bad["gate"][0, -1] = 0.5
            tried.append(_must_fail(case, bad, "padded channel left at 0.5"))
        bad = _with(ok)
        bad["gate"][-1] = float("nan")
        tried.append(_must_fail(case, bad, "last row unwritten"))
        assert len(tried) >= 4
        return
    k_first = case.c1 if case.form == "edp" else case.c0  # K of the conv behind the (last) input transform
    # the last partial 8-channel chunk of K dropped in one tile (the last, ragged one), in either conv
    if k_first % 8:
        tried.append(_must_fail(case, splice("_drop_chunk", "y1", (m - 1) // tile * tile, m), "partial chunk dropped"))
    if case.c2 and case.form != "edp" and case.c1 % 8:
        tried.append(_must_fail(case, splice("_drop_chunk2", "y2", (m - 1) // tile * tile, m), "partial chunk of the second conv dropped"))
    # the neighbouring clip's gate for the rows of the first tile that straddles clips 0 and 1
    if case.gate or case.cse:
        assert s % tile, f"{case.id}: no tile straddles two clips"
        tried.append(_must_fail(case, splice("_gate_roll", "y1", s // tile * tile, s), "neighbouring clip's gate"))
    if case.cse:
        tried += [_must_fail(case, emulate(case, f), f) for f in ("pool_row", "pool_pad")]
    if case.form == "short":
        tried += [_must_fail(case, emulate(case, f), f) for f in ("short_col", "short_bias")]
    if case.res or case.form == "edp":
        tried.append(_must_fail(case, emulate(case, "res_after"), "residual added after the ReLU"))
        if case.c2:
            tried.append(_must_fail(case, emulate(case, "pre_res"), "second conv fed the pre-residual sum"))
    if case.form == "edp":
        n, t = case.nthw[0], case.nthw[1]
        fr = 49
        # the frames outside a clip taken from the neighbouring clip: clip 1's first frame / clip 0's last (T = 1: the only one; T = 3: a tile's
        # first frame, whose second frame is absent), and the stencil's zero border replaced by the edge value on one side (one frame)
        lo = t * fr
        tried.append(_must_fail(case, splice("t_before", "y1", lo, lo + fr), "frame before the clip from the neighbouring clip"))
        lo = (t - 1) * fr
        tried.append(_must_fail(case, splice("t_after", "y1", lo, lo + fr), "frame after the clip from the neighbouring clip"))
        tried.append(_must_fail(case, splice("border", "y1", m - fr, m), "zero border replaced by the edge value"))
        tiles = n * ((t + 1) // 2)
        if tiles > 256:  # two tiles per block: the second frame of the last block's second tile unwritten
            last = tiles - 1
            nn_, tch = last // ((t + 1) // 2), last % ((t + 1) // 2)
            f1 = 2 * tch + 1
            assert f1 < t
            lo = (nn_ * t + f1) * fr
            for k in ok:
                bad = _with(ok)
                _rows(bad[k])[lo:lo + fr] = float("nan")
                tried.append(_must_fail(case, bad, f"second frame of the last tile unwritten in {k}"))
    for k, c in fk.outputs(case):
        bad = _with(ok)
        _rows(bad[k])[m // 2 + 1] = _rows(ok[k])[m // 2]
        tried.append(_must_fail(case, bad, f"{k}: row at its neighbour's position"))
        if c % 8:
            bad = _with(ok)
            bad[k][0, 0, 0, 0, -1] = 0.5
            tried.append(_must_fail(case, bad, f"{k}: padded channel left at 0.5"))
        bad = _with(ok)
        _rows(bad[k])[m - 1] = float("nan")
        tried.append(_must_fail(case, bad, f"{k}: last row unwritten"))
    assert len(tried) >= 4, tried
