"""GPU: conformal prediction (csrc/conformal.hip through protoasnet_amd.conformal) against the float64 / int64 numpy restatement of
tests/conformal_cases.py -- scores and thresholds bitwise, masks and tallies as integers --, and through SelectiveEvaluator.finish and
DPTrainer.fit_conformal / evaluate_selective."""
import csv
import os

import numpy as np
import pytest
import torch

import conformal_cases as cf
from protoasnet_amd import conformal, selective
from test_cpu_trainer import TRAIN_CFG
from test_gpu_selective import _cine_loader, _Head
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHAS = {1: (0.1,), 3: (0.05, 0.1, 0.2), 8: (0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9)}
ALL_KINDS = (("lac", False), ("aps", True), ("aps", False), ("raps", True), ("raps", False))
# (M, K_real, A, kinds): one thread, the edges of the 256-row block, several blocks, and at 70 000 rows several chunks per stratum
CASES = [(1, 2, 1, ALL_KINDS), (255, 4, 3, ALL_KINDS), (256, 16, 8, ALL_KINDS), (257, 2, 3, ALL_KINDS), (5000, 4, 3, ALL_KINDS),
         (5000, 16, 8, ALL_KINDS), (70000, 4, 3, (("aps", True), ("raps", False))), (70000, 16, 1, (("lac", False), ("raps", True))),
         (70000, 2, 8, (("aps", False),))]
SETTINGS = dict(seed=7 + (5 << 32), lam=0.01, k_reg=2)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    """fp32 arrays bitwise equal, any NaN in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    bad = np.argwhere((_bits(got) != _bits(want)) & ~nan)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def _check_fit(fit, want, what):
    _same_bits(fit.qhat.cpu().numpy(), want["qhat"], what + " qhat")
    assert fit.n.dtype == torch.int64 and np.array_equal(fit.n.cpu().numpy(), want["n"]), (what, fit.n.tolist(), want["n"].tolist())
    assert np.array_equal(fit.r.cpu().numpy(), want["r"]), what


def _check_sets(sets, want, what):
    masks, tallies = want
    got_m = sets.masks.cpu().numpy()
    assert got_m.dtype == np.uint16 and np.array_equal(got_m, masks), (what, np.argwhere(got_m != masks)[:4].tolist())
    got_t = sets.tallies.cpu().numpy()
    assert got_t.dtype == np.int64 and np.array_equal(got_t, tallies), (what, np.argwhere(got_t != tallies)[:6].tolist())


@pytest.mark.parametrize("M,K,A,kinds", CASES)
def test_scores_thresholds_and_sets_match_the_restatement(M, K, A, kinds):
    alphas = ALPHAS[A]
    probs, labels = cf.conf_case(M, K, seed=M + K)
    pt, lt = cf.conf_case(M, K, seed=M + K + 1)
    u = cf.u_case(M, seed=3)
    d_probs, d_labels, d_pt, d_lt, d_u = _dev(probs, labels, pt, lt, u)
    for kind, rnd in kinds:
        kw = dict(kind=kind, randomized=rnd, **SETTINGS)
        what = f"M={M} K={K} A={A} {kind} randomized={rnd}"
        table, own, stratum = conformal.scores(d_probs, d_labels, salt=0, **kw)
        want_table = cf.scores_ref(probs, salt=0, **kw)
        want_st = cf.strata_ref(probs, labels)
        _same_bits(table.cpu().numpy(), want_table, what + " scores")
        assert stratum.dtype == torch.int32 and np.array_equal(stratum.cpu().numpy(), want_st), what
        _same_bits(own.cpu().numpy(), cf.own_ref(want_table, want_st), what + " own")
        fit = conformal.calibrate(d_probs, d_labels, alphas, **kw)
        want_fit = cf.calibrate_ref(probs, labels, alphas, **kw)
        _check_fit(fit, want_fit, what)
        for mondrian in (False, True):
            sets = conformal.predict_sets(d_pt, fit, d_lt, d_u, mondrian=mondrian)
            _check_sets(sets, cf.predict_ref(pt, want_fit, alphas, lt, u, mondrian, **kw), f"{what} mondrian={mondrian}")
    # u omitted, labels omitted: masks and the size histogram only (the last kind of the case)
    sets = conformal.predict_sets(d_pt, fit, d_lt)
    _check_sets(sets, cf.predict_ref(pt, want_fit, alphas, lt, None, False, **kw), what + " no u")
    sets = conformal.predict_sets(d_pt, fit, None, d_u, mondrian=True)
    want = cf.predict_ref(pt, want_fit, alphas, None, u, True, **kw)
    _check_sets(sets, want, what + " no labels")
    assert not sets.has_labels and want[1][:, 1].sum() == 0 and want[1][:, 3 + 4 * (K + 1):].sum() == 0
    # the summary is the restatement's, from ONE read
    assert repr(sets.summary()) == repr(cf.summary_ref(want[1], alphas, K, has_labels=False))


def test_one_row_has_too_few_rows_for_any_level():
    """n = 1: r = ceil(2 (1 - alpha)) = 2 > n for alpha < 0.5: +inf and the full label set; at alpha = 0.5 and above r = 1."""
    probs, labels = np.array([[0.25, 0.75]], np.float32), np.array([1])
    d = _dev(probs, labels)
    fit = conformal.calibrate(*d, alphas=(0.1, 0.5, 0.9), kind="lac")
    assert fit.qhat[0].tolist() == [float("inf"), 0.25, 0.25] and fit.r[0].tolist() == [2, 1, 1] and fit.n.tolist() == [1, 0, 1]
    assert fit.qhat[1].tolist() == [float("inf")] * 3 and fit.r[1].tolist() == [1, 1, 1]  # an empty stratum
    sets = conformal.predict_sets(d[0], fit, d[1])
    assert sets.masks.tolist() == [[3], [2], [2]] and sets.summary()[0]["size_hist"] == [0, 0, 1]
    rd = fit.read()
    assert rd["qhat"] == [float("inf"), 0.25, 0.25] and rd["n"] == 1 and rd["n_per_class"] == [0, 1] and rd["kind"] == "lac"


def test_every_score_ties():
    """All rows identical: every own-label score of a class is one number, and the threshold is that number."""
    M, K = 3000, 4
    probs = np.tile(np.array([[0.5, 0.25, 0.125, 0.125]], np.float32), (M, 1))
    labels = (np.arange(M) % 3).astype(np.int32)  # class 3 has no rows: its Mondrian threshold is +inf
    d = _dev(probs, labels)
    for kind in ("lac", "aps"):
        fit = conformal.calibrate(*d, alphas=(0.05, 0.5, 0.95), kind=kind, randomized=False)
        _check_fit(fit, cf.calibrate_ref(probs, labels, (0.05, 0.5, 0.95), kind, False), kind)
        own = {"lac": [0.5, 0.75, 0.875], "aps": [0.5, 0.75, 0.875]}[kind]
        assert fit.qhat[1:4].tolist() == [[v] * 3 for v in own] and fit.qhat[4].tolist() == [float("inf")] * 3 and fit.n.tolist() == [M, 1000, 1000, 1000, 0]
        assert fit.qhat[0].tolist() == [0.875, 0.75, 0.5]  # the 2851st, 1501st and 151st of 1000 x (0.5, 0.75, 0.875)
        sets = conformal.predict_sets(d[0], fit, d[1], mondrian=True)
        _check_sets(sets, cf.predict_ref(probs, cf.calibrate_ref(probs, labels, (0.05, 0.5, 0.95), kind, False), None, labels, None, True,
                                         kind=kind, randomized=False), kind)
        assert ((sets.masks[0].view(torch.int16) & 8) != 0).all()  # +inf admits class 3 in every row


def test_salts_seeds_and_repeated_calls():
    probs, labels = cf.conf_case(5000, 4, seed=1)
    d = _dev(probs, labels)
    s0, s1 = (conformal.scores(d[0], kind="aps", seed=7, salt=s) for s in (0, 1))
    _same_bits(s0.cpu().numpy(), cf.scores_ref(probs, "aps", True, 7, salt=0), "salt 0")
    _same_bits(s1.cpu().numpy(), cf.scores_ref(probs, "aps", True, 7, salt=1), "salt 1")
    ok = ~torch.isnan(s0)
    assert (s0[ok] != s1[ok]).float().mean() > 0.9  # other uniforms
    assert torch.equal(conformal.scores(d[0], kind="aps", randomized=False, salt=0)[ok], conformal.scores(d[0], kind="aps", randomized=False, salt=1)[ok])
    # two calls on the same input are bitwise equal, in every output
    kw = dict(alphas=(0.05, 0.1, 0.2), kind="raps", seed=3, lam=0.02, k_reg=1)
    a, b = conformal.calibrate(*d, **kw), conformal.calibrate(*d, **kw)
    assert torch.equal(a.qhat.view(torch.int32), b.qhat.view(torch.int32)) and torch.equal(a.n, b.n) and torch.equal(a.r, b.r)
    u = _dev(cf.u_case(5000, 2))[0]
    x, y = (conformal.predict_sets(d[0], a, d[1], u, mondrian=True) for _ in range(2))
    assert torch.equal(x.masks.view(torch.int16), y.masks.view(torch.int16)) and torch.equal(x.tallies, y.tallies)
    # a fit that went through its state dict predicts the same sets
    z = conformal.predict_sets(d[0], conformal.ConformalFit.from_state_dict(a.state_dict(), device=DEV), d[1], u, mondrian=True)
    assert torch.equal(x.masks.view(torch.int16), z.masks.view(torch.int16)) and torch.equal(x.tallies, z.tallies)


def test_non_contiguous_and_non_fp32_inputs():
    """A strided fp64 view and a bf16 tensor: the kernels see the fp32 copy of the values; int64 labels and an fp64 u likewise."""
    M, K = 300, 4
    probs, labels = cf.conf_case(M, K, seed=5)
    u = cf.u_case(M, 6)
    wide = torch.zeros(M, 2 * K, dtype=torch.float64, device=DEV)
    wide[:, ::2] = _dev(probs)[0].double()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    kw = dict(kind="aps", randomized=True, seed=11)
    d_labels, d_u = _dev(labels.astype(np.int64), u.astype(np.float64))
    fit = conformal.calibrate(view, d_labels, (0.1, 0.2), **kw)
    want_fit = cf.calibrate_ref(probs, labels, (0.1, 0.2), **kw)
    _check_fit(fit, want_fit, "strided fp64")
    _check_sets(conformal.predict_sets(view, fit, d_labels, d_u), cf.predict_ref(probs, want_fit, None, labels, u, False, **kw), "strided fp64")
    half = _dev(probs)[0].to(torch.bfloat16)
    p16 = half.float().cpu().numpy()
    _same_bits(conformal.scores(half, **kw).cpu().numpy(), cf.scores_ref(p16, **kw), "bf16")
    _check_fit(conformal.calibrate(half, d_labels, (0.1, 0.2), **kw), cf.calibrate_ref(p16, labels, (0.1, 0.2), **kw), "bf16")


# ---- wiring --------------------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_close(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_close(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return (np.isnan(a) and np.isnan(b)) or a == b
    return a == b


def _want_conformal(probs, labels, u, fit, want_fit, mondrian):
    """res["conformal"] from the restatement, for device rows; and the masks."""
    p, y, uu = probs.cpu().numpy(), labels.cpu().numpy(), u.cpu().numpy()
    kw = {k: fit.settings[k] for k in ("kind", "randomized", "seed", "lam", "k_reg")}
    masks, t = cf.predict_ref(p, want_fit, fit.alphas, y, uu, mondrian, **kw)
    q = want_fit["qhat"].astype(np.float64)
    return {"kind": fit.kind, "mondrian": mondrian, "alphas": list(fit.alphas), "qhat": q[0].tolist(), "qhat_per_class": q[1:].tolist(),
            "levels": cf.summary_ref(t, fit.alphas, p.shape[1])}, masks


@pytest.mark.parametrize("abstain", [True, False])
def test_selective_evaluator_finish_with_conformal(abstain, monkeypatch):
    from protoasnet_amd import calibration

    rng = np.random.default_rng(16)
    Bt, nb, K = 7, 9, 4
    Kr = K - 1 if abstain else K
    names = [f"cine{g}" for g in range(11)]
    keys = [names[int(g)] for g in rng.integers(0, len(names), Bt * nb)]
    y = np.array([names.index(k) % 3 for k in keys])
    lg = np.random.default_rng(17).uniform(-4.0, 4.0, (Bt * nb, K)).astype(np.float32)
    lg[np.arange(Bt * nb), y] += 2.0
    sel = selective.SelectiveEvaluator(_Head().to(DEV), abstain_class=abstain, capacity=8)
    for b in range(nb):
        s = slice(b * Bt, (b + 1) * Bt)
        sel.update(torch.from_numpy(lg[s]).to(DEV), torch.rand(Bt, 8, device=DEV), torch.from_numpy(y[s]).to(DEV), keys[s])
    logits, labels = sel.ev.logits[: sel.ev.rows], sel.ev.labels[: sel.ev.rows]
    groups = selective.build_groups(keys)
    alphas = (0.1, 0.3)
    kw = dict(kind="raps", randomized=True, seed=5, lam=0.05, k_reg=1)
    reads = []
    to_host = torch.Tensor.cpu
    for temperature in (None, 1.7):
        if temperature is None:
            probs, u = sel.ev.probs[: sel.ev.rows], selective.uncertainty(logits, abstain)
        else:
            probs, u = calibration.scaled_probs(logits, Kr, temperature, with_u=True)
            if abstain:
                u = selective.uncertainty(logits, True)
        for level, mondrian in (("clip", False), ("clip", True), ("cine", False), ("cine", True)):
            if level == "clip":
                rows = (probs, labels, u)
            else:
                gp = selective.group_predictions(probs, u, labels, groups)
                rows = (gp.p_conf.float(), gp.labels, gp.u_mean.float())
            fit = conformal.calibrate(rows[0], rows[1], alphas, **kw)  # (held to the restatement above)
            want_fit = cf.calibrate_ref(rows[0].cpu().numpy(), rows[1].cpu().numpy(), alphas, **kw)
            _check_fit(fit, want_fit, f"{level} T={temperature}")
            with monkeypatch.context() as mp:
                mp.setattr(torch.Tensor, "cpu", lambda t, *a, **k: reads.append(t.numel()) or to_host(t, *a, **k))
                del reads[:]
                res = sel.finish(level=level, temperature=temperature, conformal=fit, conformal_mondrian=mondrian)
                assert len(reads) == 1, (level, reads)  # one synchronising read
                both = sel.finish(level=level, temperature=temperature, conformal=fit, conformal_mondrian=mondrian, bootstrap=9, seed=3,
                                  calibration=10)
                plain = sel.finish(level=level, temperature=temperature)
            want, masks = _want_conformal(*rows, fit, want_fit, mondrian)
            assert _close(res["conformal"], want), (level, mondrian, temperature)
            assert _close(both["conformal"], want) and "ci" in both and "calibration" in both  # behind the other opt-ins too
            assert res["conformal"]["levels"][0]["rows"] == res["rows"]
            if level == "cine":
                for a, alpha in enumerate(alphas):
                    assert [c[f"set@{alpha:g}"] for c in res["cines"]] == [conformal.mask_classes(m, Kr) for m in masks[a]]
                for c in res["cines"]:
                    for alpha in alphas:
                        del c[f"set@{alpha:g}"]
            assert "conformal" not in plain and _close({k: v for k, v in res.items() if k != "conformal"}, plain)  # every other key as it was


@pytest.mark.timeout(900)
def test_trainer_fit_conformal_and_evaluate_selective(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to(DEV)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    loader = _cine_loader(4, 3, 70)
    logs = []
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda s, *_: logs.append(str(s)))
    with pytest.raises(ValueError, match="fit_conformal"):
        t.evaluate_selective("test", conformal="fitted")
    state = (t.current_epoch, t.current_iteration, m.training)
    kw = dict(alphas=(0.2, 0.5), kind="aps", seed=4)
    got = t.fit_conformal("val", **kw)
    assert (t.current_epoch, t.current_iteration, m.training) == state and any("conformal aps (cine)" in s and "qhat" in s for s in logs)
    assert got == t.conformal_fit.read() and got["n"] == 3 and got["kind"] == "aps" and got["alphas"] == [0.2, 0.5]
    # the same sweep fed by hand: the default level calibrates on one row per cine
    sel = selective.SelectiveEvaluator(m, abstain_class=True)
    with torch.no_grad():
        for b in loader:
            lg, sim, _ = m(b["cine"].to(DEV))
            sel.update(lg, sim, b["target_AS"].to(DEV), b["filename"])
    ev = sel.ev
    probs, labels = ev.probs[: ev.rows], ev.labels[: ev.rows]
    gp = selective.group_predictions(probs, selective.uncertainty(ev.logits[: ev.rows], True), labels, selective.build_groups(sel.keys))
    want_fit = cf.calibrate_ref(gp.p_conf.float().cpu().numpy(), gp.labels.cpu().numpy(), (0.2, 0.5), "aps", True, 4)
    _check_fit(t.conformal_fit, want_fit, "trainer cine")
    res = t.evaluate_selective("test", level="cine", conformal="fitted")
    assert _close(res, sel.finish(level="cine", conformal=t.conformal_fit))
    want, masks = _want_conformal(gp.p_conf.float(), gp.labels, gp.u_mean.float(), t.conformal_fit, want_fit, False)
    assert _close(res["conformal"], want) and res["conformal"]["levels"][0]["rows"] == 3
    assert [c["set@0.2"] for c in res["cines"]] == [conformal.mask_classes(x, 3) for x in masks[0]]
    with open(tmp_path / "conformal_test.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0][:6] == ["alpha", "kind", "mondrian", "level", "qhat", "rows"] and len(rows) == 3 and [float(r[0]) for r in rows[1:]] == [0.2, 0.5]
    assert [float(r[4]) for r in rows[1:]] == res["conformal"]["qhat"] and [float(r[6]) for r in rows[1:]] == [lv["coverage"] for lv in res["conformal"]["levels"]]
    # clip level, Mondrian, an explicit fit
    clip = t.fit_conformal("val", level="clip", **kw)
    assert clip["n"] == 12
    _check_fit(t.conformal_fit, cf.calibrate_ref(probs.cpu().numpy(), labels.cpu().numpy(), (0.2, 0.5), "aps", True, 4), "trainer clip")
    res = t.evaluate_selective("test", level="clip", conformal=t.conformal_fit, conformal_mondrian=True)
    assert res["conformal"]["mondrian"] and res["conformal"]["levels"][1]["rows"] == 12 == res["rows"]
    assert "conformal" not in t.evaluate_selective("test", level="clip")
    assert "conformal_test.csv" in os.listdir(tmp_path)
