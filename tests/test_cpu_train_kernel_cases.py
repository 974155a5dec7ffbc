"""CPU: the inputs and fp64 references of tests/train_kernel_cases.py, checked without a GPU -- the references against autograd or an
independent restatement, the geometry replica against the library, and the conditions the GPU comparisons rely on: nothing at a ReLU
kink, unambiguous arg-mins, enough tied pooling windows, and bounds that FAIL on a dropped row, a flipped mask and a tie sent to the
last maximum (as conftest.assert_discriminates does for the golden samples)."""
import pytest
import torch
import torch.nn.functional as F

import train_kernel_cases as tk
from conftest import assert_close

F64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16]


def _rel(a, e, tol, name=""):
    assert_close(a.to(F64), e.to(F64), tol * (float(e.abs().max()) + 1e-12), 0.0, name)


def _must_fail(a, e, tol, name):
    with pytest.raises(AssertionError):
        _rel(a, e, tol, name)


# ------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("contig", [False, True])
def test_row_geometry_replica_and_the_multi_chunk_shapes(contig, monkeypatch):
    """The replica of row_geom() agrees with pasn_train_chunks under both settings of PASN_TRAIN_ROWS_CONTIG, and the multi-chunk shapes are
    what the tests say: two chunks, the last one ragged, a chunk no multiple of the 4 * RL rows a block has in flight."""
    from protoasnet_amd import _lib

    if contig:
        monkeypatch.setenv("PASN_TRAIN_ROWS_CONTIG", "1")
    else:
        monkeypatch.delenv("PASN_TRAIN_ROWS_CONTIG", raising=False)
    lib = _lib.lib()
    shapes = [(sh[0], sh[1] * sh[2] * sh[3], (c + 7) // 8 * 8) for c, sh, _ in tk.UNIT_CASES + tk.GROUP_CASES]
    shapes += [(n, t * h * w, (c + 7) // 8 * 8) for n, c, _, (t, h, w) in tk.SE_CASES]
    shapes += [(32, 16 * 56 * 56, 24), (32, 16 * 7 * 7, 432), (1, 100000, 8), (2000, 5000, 2048)]
    for n, s, cp in shapes:
        assert lib.pasn_train_chunks(n, s, cp) == tk.row_geom(n, s, cp, contig)["chunks"], (n, s, cp)
    # the switch reaches the library: 2400 rows of 24 channels are two chunks of 64-row blocks, one chunk of 85-row blocks
    assert lib.pasn_train_chunks(2, 2400, 24) == (1 if contig else 2)
    want = {(432, 147): (2, 74, 4, 4), (56, 1197): (2, 599, 32, 36), (24, 2883): (2, 1442, 64, 85)}  # chunks, rows per chunk, RL default / contiguous
    multi = [(sh[0], c, sh[1] * sh[2] * sh[3]) for c, sh, _ in tk.UNIT_MULTI_CHUNK + tk.GROUP_MULTI_CHUNK]
    multi += [(n, c, t * h * w) for n, c, _, (t, h, w) in tk.SE_MULTI_CHUNK]
    for n, c, s in multi:
        cp = (c + 7) // 8 * 8
        g = tk.row_geom(n, s, cp, contig)
        chunks, rpc, rl0, rl1 = want[(cp, s)]
        assert (g["chunks"], g["rows_per_chunk"], g["RL"]) == (chunks, rpc, rl1 if contig else rl0)
        assert s % g["chunks"] != 0 and g["rows_per_chunk"] % (4 * g["RL"]) != 0
        assert g["live_threads"] == ({432: 216, 56: 252, 24: 255}[cp] if contig else 256)  # contiguous rows: some threads of a block idle
    single = [c for c in tk.UNIT_CASES + tk.GROUP_CASES if c not in tk.UNIT_MULTI_CHUNK + tk.GROUP_MULTI_CHUNK]
    for c, sh, _ in single:
        assert tk.row_geom(sh[0], sh[1] * sh[2] * sh[3], (c + 7) // 8 * 8, contig)["chunks"] == 1


# ------------------------------------------------------------------------------------------------- norm unit
def _unit_autograd(case, residual):
    n, gd = case["n"], case["n"] // case["groups"]
    y = case["y"].to(F64).requires_grad_()
    res = case["res"].to(F64).requires_grad_()
    gamma, beta = case["gamma"].to(F64).requires_grad_(), case["beta"].to(F64).requires_grad_()
    rm, rv = torch.zeros(case["c"], dtype=F64), torch.ones(case["c"], dtype=F64)
    out = torch.cat([F.relu(F.batch_norm(y[k * gd:(k + 1) * gd], rm, rv, gamma, beta, True, 0.1, 1e-5) + (res[k * gd:(k + 1) * gd] if residual else 0.0))
                     for k in range(n // gd)])
    out.backward(case["da"].to(F64))
    return out.detach(), y.grad, res.grad, gamma.grad, beta.grad, rm, rv


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("spec", [(c, sh, off, 1) for c, sh, off in tk.UNIT_CASES] + [(c, sh, 0.0, g) for c, sh, g in tk.GROUP_CASES])
def test_unit_reference_and_kink(spec, dtype):
    c, shape, offset, groups = spec
    case = tk.unit_case(c, shape, offset, dtype, groups)
    for name in ("y", "res", "da"):
        assert torch.equal(case[name], case[name].to(dtype).float()), f"{name} must hold values of the compute dtype"
    out, dy, dres, dgamma, dbeta, rm, rv = _unit_autograd(case, True)
    for got, ref, name in ((case["out"], out, "out"), (case["dy"], dy, "dy"), (case["dres"], dres, "dres"), (case["dgamma"], dgamma, "dgamma"),
                           (case["dbeta"], dbeta, "dbeta"), (case["running_mean"], rm, "running_mean"), (case["running_var"], rv, "running_var")):
        _rel(got, ref, 1e-11, name)
    us = [case["u"]]
    if "u_plain" in case:
        out0, dy0, _, dgamma0, dbeta0, _, _ = _unit_autograd(case, False)
        for got, ref, name in ((case["out_plain"], out0, "out"), (case["dy_plain"], dy0, "dy"), (case["dgamma_plain"], dgamma0, "dgamma"),
                               (case["dbeta_plain"], dbeta0, "dbeta")):
            _rel(got, ref, 1e-11, name + " (no residual)")
        us.append(case["u_plain"])
    else:
        assert offset != 0.0 or groups > 1
    for u in us:
        band = tk._kink_band(u)
        # the cap on exclusions (0.1 % of the elements, 5 % of the channels) is met with nothing to exclude at all
        assert int(band.sum()) == 0, f"{int(band.sum())} pre-activations within {tk.KINK} of the kink"
        assert 0.2 < float((u > 0).double().mean()) < 0.8 or offset != 0.0, "the mask must cut a good part of the elements"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("spec", tk.SE_CASES)
def test_se_reference(spec, dtype):
    case = tk.se_case(*spec, dtype=dtype)
    n, c = case["n"], case["c"]
    y = case["y"].to(F64).requires_grad_()
    P = [p.to(F64).requires_grad_() for p in case["params"]]
    u = F.batch_norm(y, None, None, P[0], P[1], True, 0.1, 1e-5)
    pool = u.mean(dim=(2, 3, 4))
    gate = torch.sigmoid(F.linear(F.relu(F.linear(pool, P[2], P[3])), P[4], P[5]))
    v = u * gate[:, :, None, None, None]
    out = v * torch.sigmoid(v)
    out.backward(case["da"].to(F64))
    ex = case["exact"]
    _rel(case["out"], out.detach(), 1e-11, "out")
    _rel(case["gate"], gate.detach(), 1e-11, "gate")
    _rel(ex["dy"], y.grad, 1e-10, "dy")
    for name, p in zip(("dgamma", "dbeta", "dw1", "db1", "dw2", "db2"), P):
        _rel(ex[name], p.grad, 1e-10, name)
    assert float(case["pre1"].abs().min()) > 10 * tk.KINK * float(case["pre1"].abs().max()), "a hidden unit of the SE MLP sits at its ReLU kink"
    for form in ("two_pass", "analytic"):
        for name in ("dy", "dgamma", "dbeta", "coef"):
            if dtype == torch.float32:
                _rel(case[form][name], ex[name], 1e-6, f"{form} {name}")  # an fp32 store rounds by 6e-8
            else:  # the stored d' moves the values by a rounding, never by more
                _rel(case[form][name], ex[name], 3 * tk.BF16_STORE, f"{form} {name}")
    if dtype == torch.bfloat16:
        assert not torch.equal(case["two_pass"]["dgamma"], ex["dgamma"]), "mode 2 sums the STORED d'"
        assert torch.equal(case["analytic"]["dgamma"], ex["dgamma"]), "mode 4 sums the unrounded d'"


# ------------------------------------------------------------------------------------------------- max pooling
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(tk.MAXPOOL_CASES)))
def test_maxpool_cases_ties_and_first_maximum(i, dtype):
    case = tk.maxpool_case(i, dtype)
    x, dy, k, s, p = case["x"].to(F64), case["dy"].to(F64), case["k"], case["s"], case["p"]
    win, lin = tk.pool_windows(x, k, s, p)
    assert torch.equal(win.max(dim=-1).values, case["y"])
    # torch's CPU backward == "the FIRST maximum in scan order takes the window's gradient", the contract of pasn_maxpool3d_bwd
    first = tk.pool_route(x, dy, k, s, p, "first")
    assert torch.equal(first, case["dx"])
    assert not torch.equal(tk.pool_route(x, dy, k, s, p, "last"), case["dx"])
    assert_close(case["dx"].sum(dim=(2, 3, 4)), dy.sum(dim=(2, 3, 4)), 1e-12, 0.0, "every window routes to exactly one element")
    mx = win.max(dim=-1, keepdim=True).values
    tied = (win == mx).sum(dim=-1) > 1
    assert float(tied.double().mean()) >= 0.2, f"only {float(tied.double().mean()):.3f} of the windows have a tied maximum"
    assert 0.1 < float((x > 0).double().mean()) < 0.5
    assert float(x[0, :8].abs().max()) == 0.0
    if max(p) > 0:  # a padded border window, all zeros: its first maximum is its first IN-RANGE slot, not its origin
        allzero = (win[0, 0].max(dim=-1).values == 0) & (lin[0, 0, ..., 0] < 0)
        assert bool(allzero.any())
        target = lin[0, 0][allzero]
        assert bool((target[:, 0] == -1).all()) and bool((target.max(dim=-1).values >= 0).all())
    if dtype == torch.bfloat16:
        assert x[case["n"] - 1, case["c"] - 1].unique().numel() <= 4
        assert torch.equal(case["x"], case["x"].bfloat16().float()) and torch.equal(case["dy"], case["dy"].bfloat16().float())


# ------------------------------------------------------------------------------------------------- ProtoPNet head
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("activation", [0, 1], ids=["log", "linear"])
@pytest.mark.parametrize("tag", list(tk.HEAD_CASES))
def test_head_cases_argmin_gap_and_constructed_positions(tag, activation, dtype):
    case = tk.head_case(tag, dtype, activation)
    n, s, p = case["n"], case["S"], case["P"]
    assert torch.equal(case["z"], case["z"].to(dtype).float()) and torch.equal(case["protos"], case["protos"].to(dtype).float())
    assert all(bool(torch.isfinite(case[k]).all()) for k in ("min_dist", "logits", "dz", "dprotos", "dfc_w", "coef"))
    if s > 1:
        top2 = case["dist"].sort(dim=2).values[..., :2]
        gap_ok = (top2[..., 1] - top2[..., 0]) > tk.GAP * top2[..., 0]
        assert bool(gap_ok.all()), f"{int((~gap_ok).sum())} ambiguous arg-mins"
    # the reference's gradient of the min-distance is the kernel's coefficient g = dmin + (dlogits W) sim'(d)
    d = case["min_dist"]
    dsim = (1 / (d + 1) - 1 / (d + 1e-4)) if activation == 0 else -torch.ones_like(d)
    g = case["dmin"].to(F64) + (case["dlogits"].to(F64) @ case["fcw"].to(F64)) * dsim
    _rel(case["coef"], g, 1e-12, "coef")
    # ... and only the arg-min rows carry gradient: dz[n][s*] = sum over the prototypes there of 2 g (z - p)
    zz, pv = case["z"].to(F64), case["protos"].to(F64)
    dz = torch.zeros_like(zz)
    for ni in range(n):
        for pi in range(p):
            si = int(case["argmin"][ni, pi])
            dz[ni, si] += 2 * g[ni, pi] * (zz[ni, si] - pv[pi])
    _rel(case["dz"], dz, 1e-11, "dz")
    assert bool((case["dz"][case["shared"] == 0] == 0).all())
    if tag == "shared":
        assert case["argmin"][0, :tk.HEAD_SHARED].tolist() == [3] * tk.HEAD_SHARED and int(case["shared"][0, 3]) >= 4
        assert case["min_dist"][0, :tk.HEAD_SHARED].unique().numel() == tk.HEAD_SHARED, "distinct offsets"
    if tag == "exact":
        assert float(case["min_dist"][1, 4]) == 0.0 and int(case["argmin"][1, 4]) == 7
    if tag == "dp16":
        assert case["Dp"] > case["D"]
    if tag == "r512":
        assert case["D"] > 256
    assert int(case["shared"].max()) >= 2, "two prototypes on one row: the ordered accumulation is exercised"


# ------------------------------------------------------------------------------------------------- discrimination
def _typical(v):
    """Index of the element of median magnitude: a corruption there is neither the easiest nor the hardest one to see."""
    v = v.reshape(-1).abs()
    return int((v - v.median()).abs().argmin())


def test_bounds_discriminate_a_dropped_row_a_flipped_mask_and_a_misrouted_tie():
    """Each bf16 bound of the GPU tests, applied to the reference and a corrupted copy of it, must FAIL: the fp32 bounds of the sums on one row
    of one clip left out, the k * 2^-8 bounds of the elementwise outputs on ONE element of typical size taking the wrong branch (a flipped
    ReLU mask; for Swish a dropped derivative, for |r| a flipped sign, for a sum over prototypes a missing term), the max-pool bound on a tie
    sent to its last maximum.  (A dropped row moves an elementwise output by d / R only -- below any bf16 store; the sums catch it.)"""
    bf = torch.bfloat16
    for c, shape, _ in tk.UNIT_MULTI_CHUNK:
        case = tk.unit_case(c, shape, 0.0, bf)
        n, s = case["n"], case["S"]
        flat = lambda x: x.reshape(n, c, s)
        y, dpre, yhat = flat(case["y"].to(F64)), flat(case["dres"]), flat(case["yhat"])
        row = s - 1  # the last row of clip 0: the ragged end of the last chunk
        # (a) one row of one clip left out of the sums
        _must_fail(case["dbeta"] - dpre[0, :, row], case["dbeta"], 1e-4, "dbeta")
        _must_fail(case["dgamma"] - (dpre * yhat)[0, :, row], case["dgamma"], 1e-4, "dgamma")
        _must_fail(case["coef"][0, 0] - dpre[0, :, row] / (n * s), case["coef"][0, 0], 1e-4, "coef")
        mean = y.mean(dim=(0, 2))
        _must_fail((mean * n * s - y[0, :, row]) / (n * s), mean, 1e-5, "mean")
        # (b) one element's mask flipped
        da = flat(case["da"].to(F64))
        i = _typical(da[0, 0])
        flipped = dpre.clone()
        flipped[0, 0, i] = da[0, 0, i] - dpre[0, 0, i]
        _must_fail(flipped, dpre, tk.tol_stores(1e-5, 1, bf), "residual gradient")
        sc = case["gamma"][0].double() * case["invstd"][0, 0]
        for key, stores in (("dy", 2), ("dy_plain", 1)):
            dyf = flat(case[key]).clone()
            on = float(flat(case["u" if key == "dy" else "u_plain"])[0, 0, i] > 0)
            dyf[0, 0, i] += sc * da[0, 0, i] * (1 - 2 * on)  # d' there: d <-> 0
            _must_fail(dyf, flat(case[key]), tk.tol_stores(2e-4, stores, bf), key)
        outf = flat(case["out"]).clone()
        j = _typical(flat(case["u"])[0, 0])
        outf[0, 0, j] = 0.0 if outf[0, 0, j] > 0 else -flat(case["u"])[0, 0, j]
        _must_fail(outf, flat(case["out"]), tk.tol_stores(1e-4, 1, bf), "unit output")
    # the squeeze-excite unit (Swish: no mask -- one element's derivative dropped, d' = d there)
    for spec in tk.SE_MULTI_CHUNK:
        se = tk.se_case(*spec, dtype=bf)
        n, c, s = se["n"], se["c"], se["S"]
        flat = lambda x: x.reshape(n, c, s)
        u = flat(se["u"])
        _must_fail(se["pool"][0] - u[0, :, s - 1] / s, se["pool"][0], 1e-5, "pool_u")  # the last row of clip 0 missing from the per-clip pool
        da, dv = flat(se["da"].to(F64)), flat(se["dv"])
        i = _typical(da[0, 0])
        bad = dv.clone()
        bad[0, 0, i] = da[0, 0, i]
        _must_fail(bad, dv, tk.tol_stores(2e-4, 1, bf), "d' = d swish'(.)")
        sg = se["params"][0][0].double() * se["invstd"][0] * se["gate"][0, 0]
        for form, stores in (("two_pass", 3), ("analytic", 2)):
            dyb = flat(se[form]["dy"]).clone()
            dyb[0, 0, i] += sg * (bad[0, 0, i] - dv[0, 0, i])
            _must_fail(dyb, flat(se[form]["dy"]), tk.tol_stores(2e-4, stores, bf), f"dy ({form})")
        outb = flat(se["out"]).clone()
        ch = int((se["gate"][0] - se["gate"][0].median()).abs().argmin())  # a channel whose gate is typical (some saturate at 1: nothing to see there)
        j = _typical(u[0, ch])
        v = u[0, ch, j]  # the gate left out there
        outb[0, ch, j] = v * torch.sigmoid(v)
        _must_fail(outb, flat(se["out"]), tk.tol_stores(1e-4, 1, bf), "SE unit output")
    # the XProtoNet tail: dr = sign(r) (...) with one sign flipped; dz = sum over prototypes with one term missing (dz is linear in |r|)
    for i in range(len(tk.XPROTO_CASES)):
        xp = tk.xproto_case(i, False, bf)
        j = _typical(xp["dr"][0, 0])
        bad = xp["dr"].clone()
        bad[0, 0, j] = -bad[0, 0, j]
        _must_fail(bad, xp["dr"], tk.tol_stores(1e-4, 1, bf), "dr")
        r = xp["r"].to(F64).requires_grad_()
        zz = xp["z"].to(F64).requires_grad_()
        occ = r.abs() * (1 - torch.nn.functional.one_hot(torch.tensor(0), xp["P"]).double().view(1, -1, 1) * torch.nn.functional.one_hot(torch.tensor(j), xp["S"]).double().view(1, 1, -1)
                         * torch.tensor([1.0] + [0.0] * (xp["n"] - 1), dtype=F64).view(-1, 1, 1))  # prototype 0 left out at position j of clip 0
        feat = torch.einsum("nps,nds->npd", occ, zz)
        sim = (F.cosine_similarity(feat, xp["protos"].to(F64).unsqueeze(0), dim=2, eps=1e-8) + 1) / 2
        ((F.linear(sim, xp["fcw"].to(F64)) * xp["dl"].to(F64)).sum() + (sim * xp["dsm"].to(F64)).sum()).backward()
        badz = xp["dz"].clone()
        badz[0, :, j] = zz.grad[0, :, j]
        _must_fail(badz, xp["dz"], tk.tol_stores(1e-4, 1, bf), "dz")
    # (c) one tied window routed to its last maximum instead of the first
    for i in range(len(tk.MAXPOOL_CASES)):
        case = tk.maxpool_case(i, bf)
        x, dy, k, s, p = case["x"].to(F64), case["dy"].to(F64), case["k"], case["s"], case["p"]
        win, lin = tk.pool_windows(x, k, s, p)
        tied = ((win == win.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1)[0, 0]  # clip 0, channel 0: all zeros, every window tied
        assert bool(tied.all())
        w0 = _typical(dy[0, 0])  # one window only
        slots = lin[0, 0].reshape(-1, lin.shape[-1])[w0]
        first, last = int(slots[slots >= 0][0]), int(slots[slots >= 0][-1])
        bad = case["dx"].clone().reshape(case["n"], case["c"], -1)
        bad[0, 0, first] -= dy[0, 0].reshape(-1)[w0]
        bad[0, 0, last] += dy[0, 0].reshape(-1)[w0]
        _must_fail(bad.view_as(case["dx"]), case["dx"], tk.tol_stores(1e-5, 1, bf), "max-pool dx")
    # the head: one prototype's contribution missing from a shared row
    case = tk.head_case("shared", bf, 0)
    bad = case["dz"].clone()
    bad[0, 3] -= 2 * case["coef"][0, 0] * (case["z"][0, 3].double() - case["protos"][0].double())
    _must_fail(bad[0, 3], case["dz"][0, 3], tk.tol_stores(1e-4, int(case["shared"][0, 3]), bf) * float(case["dz"].abs().max()) / float(case["dz"][0, 3].abs().max()),
               "dz of a shared row")
