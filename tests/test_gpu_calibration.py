"""GPU: calibration (csrc/calibration.hip through protoasnet_amd.calibration) against the float64 / int64 numpy restatement of
tests/calibration_cases.py, a replicate against the point call on host-expanded rows, and through SelectiveEvaluator.finish and
DPTrainer.fit_temperature / evaluate_selective."""
import csv
import os

import numpy as np
import pytest
import torch

import bootstrap_cases as bc
import calibration_cases as cc
from protoasnet_amd import bootstrap, calibration, selective
from test_cpu_trainer import TRAIN_CFG
from test_gpu_selective import _cine_loader, _Head
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
# ece, mce, cw_ece and conf_gap are the same formulas on exact integers in fp64 on both sides: the bootstrap tests' gate.
GATE = 1e-12
# beta against the restatement's float64 root, relative.  Measured (profiles/calibration_parity_observed.tsv): 0 in all ten fits below --
# Newton's last steps are smaller than an ulp of beta on both sides, whatever their summation trees, so both stop on the same fp64
# number.  Eight times an observed 0 would demand that for ever; the smallest error the format can show is one ulp, 2^-52 relative, and
# the gate is 8 times THAT: 1.8e-15, far inside the 1e-9 where beta stops mattering (|z| <= 64: a 1e-9 change moves beta z by less
# than one fp32 ulp of a probability).
BETA_GATE = 8 * 2.0 ** -52


def sum_bound(Mv):
    """brier and nll (and the two NLLs of the fit) are means of at most Mv non-negative fp64 terms added in different orders: the
    order-free bound (2 Mv + 16) 2^-53, below 1.2e-12 at 5000 rows."""
    return (2 * Mv + 16) * 2.0 ** -53


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _log(name, err, gate):
    """The largest observed error next to its gate (profiles/calibration_parity_observed.tsv); never changes the verdict."""
    if os.environ.get("PASN_PARITY_LOG"):
        with open(os.environ["PASN_PARITY_LOG"], "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{name}\tmax_err={err:.3g}\tgate={gate:.3g}\n")


def _host(rel):
    return {k: getattr(rel, k).cpu().numpy() for k in cc.INT_KEYS + ("stats",)}


def _compare(got, want, Mv, name):
    """Integers exact, NaN in the same places, the four bin statistics within GATE and brier / nll within the sum bound (and GATE)."""
    for k in cc.INT_KEYS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4])
    assert np.array_equal(np.isnan(got["stats"]), np.isnan(want["stats"])), (name, got["stats"][-1], want["stats"][-1])
    err = np.abs(got["stats"] - want["stats"])
    e_bins, e_sums = (float(np.nanmax(err[:, c], initial=0.0)) for c in ([0, 1, 2, 5], [3, 4]))
    print(f"{name}: max |stats - restatement| = {e_bins:.3g} (bins), {e_sums:.3g} (brier, nll)")
    _log(name + " ece/mce/cw_ece/conf_gap", e_bins, GATE)
    _log(name + " brier/nll", e_sums, min(GATE, sum_bound(Mv)))
    assert e_bins <= GATE and e_sums <= min(GATE, sum_bound(Mv)), (name, e_bins, e_sums)


def _check(probs, labels, n_bins, conf, groups, B, seed, name):
    want = cc.reliability_ref(probs, labels, n_bins, conf, groups, B, seed)
    rel = calibration.reliability(*_dev(probs, labels), n_bins=n_bins, conf=_dev(conf)[0], groups=groups, B=B, seed=seed)
    got = _host(rel)
    assert rel.stats.dtype == torch.float64 and got["stats"].shape == (B + 1, 6) and got["cn"].shape == (B + 1, probs.shape[1], n_bins)
    assert torch.equal(rel.point, rel.stats[B])
    K = probs.shape[1]
    _compare(got, want, int(((labels >= 0) & (labels < K)).sum()), name)
    return rel, got, want


# ---- bins --------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1), (7, 3, 10), (257, 4, 15), (5000, 16, 64)]  # (M, K_real, n_bins)


@pytest.mark.parametrize("B", [0, 3, 65])
@pytest.mark.parametrize("M,K,n_bins", SHAPES)
def test_bins_match_the_restatement(M, K, n_bins, B):
    """Identity groups; padding labels (-1 and K_real) from 257 rows on.  Once with the largest probability as the confidence, once with
    an override holding exact 0.0, 1.0, the fp32 bin edges 0.3 / 0.7, NaN, 1.5 and a negative value."""
    probs, labels = cc.prob_case(M, K, seed=M + K, pad=M >= 257)
    _, got, _ = _check(probs, labels, n_bins, None, None, B, 11, f"M={M} K={K} bins={n_bins} B={B}")
    assert (got["skipped"] == 0).all()
    if M >= 257:
        assert got["n"][B].sum() == ((labels >= 0) & (labels < K)).sum() < M
    _, got, want = _check(probs, labels, n_bins, cc.conf_case(M, seed=M, bad=True), None, B, 11, f"M={M} K={K} bins={n_bins} B={B} conf")
    if M >= 7:
        assert got["skipped"][B] >= 1 and got["n"][B][-1] >= 1 and got["n"][B][0] >= 1
        assert np.array_equal(got["cn"], cc.reliability_ref(probs, labels, n_bins, None, None, B, 11)["cn"])  # the override never reaches them


def test_bin_edges_on_the_device():
    """fp32 0.3 and 0.7 with ten bins: bins 3 and 6; 1.0: the last bin; 0.0: the first; NaN and 1.5: skipped."""
    probs = np.tile(np.array([[0.75, 0.25]], np.float32), (6, 1))
    conf = np.array([0.3, 0.7, 1.0, 0.0, np.nan, 1.5], np.float32)
    rel, got, _ = _check(probs, np.zeros(6, np.int32), 10, conf, None, 0, 0, "edges")
    assert got["n"][0].tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 0, 1] and got["skipped"][0] == 2 and got["qsum"][0][9] == 1 << 32
    s = rel.summary()
    assert s["skipped"] == 2 and s["bins"][9] == {"lo": 0.9, "hi": 1.0, "n": 1, "accuracy": 1.0, "confidence": 1.0} and np.isnan(s["bins"][1]["accuracy"])


@pytest.mark.parametrize("B", [3, 65])
def test_groups(B):
    M, K, n_bins = 257, 4, 15
    probs, labels = cc.prob_case(M, K, seed=20, pad=True)
    conf = cc.conf_case(M, seed=21, bad=True)
    groups = selective.build_groups(bc.random_groups(M, seed=22))
    assert np.diff(groups[0]).max() > 1 and (np.diff(groups[1]) != 1).any()  # uneven sizes, non-contiguous rows
    _, got, _ = _check(probs, labels, n_bins, conf, groups, B, 5, f"random groups B={B}")
    assert len(set((got["n"][:B].sum(1) + got["skipped"][:B]).tolist())) > 1  # the replicates differ in their number of rows
    _, got, _ = _check(probs, labels, n_bins, None, selective.build_groups(["all"] * M), B, 5, f"one group B={B}")
    for k in got:  # the one unit is drawn once: every replicate is the sample
        assert all(np.array_equal(got[k][b], got[k][B], equal_nan=True) for b in range(B)), k
    offsets, rows = groups[0][:21].copy(), groups[1][: groups[0][20]].copy()  # the first 20 groups only: the other rows never enter
    _, got, _ = _check(probs, labels, n_bins, conf, (offsets, rows), B, 5, f"unlisted rows B={B}")
    assert got["n"][B].sum() + got["skipped"][B] == ((labels[rows] >= 0) & (labels[rows] < K)).sum()
    with pytest.raises(ValueError, match="lie in"):
        calibration.reliability(*_dev(probs[:100], labels[:100]), groups=groups, B=B)  # rows past the tensors
    with pytest.raises(ValueError, match="one group only"):
        calibration.reliability(*_dev(probs, labels), groups=(np.array([0, 2, 4]), np.array([0, 1, 1, 2])), B=B)


def test_a_replicate_is_the_point_call_on_expanded_rows():
    M, K, n_bins, B = 257, 4, 15, 3
    probs, labels = cc.prob_case(M, K, seed=30, pad=True)
    conf = cc.conf_case(M, seed=31, bad=True)
    groups = selective.build_groups(bc.random_groups(M, seed=32))
    got = _host(calibration.reliability(*_dev(probs, labels), n_bins=n_bins, conf=_dev(conf)[0], groups=groups, B=B, seed=6))
    counts = bootstrap.draw_counts(len(groups[2]), B, seed=6).cpu().numpy()  # the device's own counts
    for b in range(B):
        idx = bc.replicate_rows(counts[b], labels, K, groups)
        d_probs, d_labels, d_conf = _dev(probs[idx], labels[idx], conf[idx])
        point = _host(calibration.reliability(d_probs, d_labels, n_bins=n_bins, conf=d_conf))
        _compare({k: v[b: b + 1] for k, v in got.items()}, {k: v[:1] for k, v in point.items()}, len(idx), f"replicate {b} against the point call")


def test_two_calls_are_bitwise_equal_and_the_chunking_does_not_show(monkeypatch):
    M, K, n_bins, B = 257, 4, 15, 65
    probs, labels = cc.prob_case(M, K, seed=40)
    args = _dev(probs, labels)
    a, b = _host(calibration.reliability(*args, n_bins=n_bins, B=B, seed=9)), _host(calibration.reliability(*args, n_bins=n_bins, B=B, seed=9))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ((a["n"].sum(1) + a["skipped"]) == M).all()  # identity groups, no padding: a replicate holds G rows
    drawn = []
    draw = bootstrap.draw_counts
    monkeypatch.setattr(bootstrap, "draw_counts", lambda G, Bc, *r, **kw: drawn.append(Bc) or draw(G, Bc, *r, **kw))
    monkeypatch.setattr(calibration, "CHUNK_BYTES", 25 * 4 * M)
    c = _host(calibration.reliability(*args, n_bins=n_bins, B=B, seed=9))
    assert drawn == [25, 25, 15]  # three chunks
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k
    few = _host(calibration.reliability(*args, n_bins=n_bins, B=5, seed=9))  # a replicate depends on (seed, b, G) only
    for k in a:
        assert few[k][:5].tobytes() == a[k][:5].tobytes() and few[k][5].tobytes() == a[k][B].tobytes(), k
    other = _host(calibration.reliability(*args, n_bins=n_bins, B=5, seed=10))
    assert not np.array_equal(other["n"][:5], few["n"][:5]) and np.array_equal(other["n"][5], few["n"][5])
    rel = calibration.reliability(*args, n_bins=n_bins, B=B, seed=9)
    ci, ref = calibration.intervals(rel, 0.9), bootstrap.intervals_of(a["stats"], 0.9, names=cc.STAT_NAMES)
    assert list(ci) == list(cc.STAT_NAMES) and ci == ref and ci["ece"]["n_finite"] == B and ci["ece"]["lo"] <= ci["ece"]["hi"]


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------
def _fit(logits, labels, K):
    fit = calibration.fit_temperature(*_dev(logits, labels), K)
    assert fit.info.dtype == torch.float64 and fit.info.shape == (4,) and fit.beta.shape == (1,) and fit.beta.data_ptr() == fit.info.data_ptr()
    return fit, fit.read()


@pytest.mark.parametrize("M,K,scale", cc.FIT_CASES)
def test_fit_finds_the_restatements_interior_root(M, K, scale):
    """8 rows: one partly filled block; 257: two; 5000: twenty; 70 000: every block strides over the rows."""
    logits, labels = cc.logit_case(M, K, scale)
    want = cc.temperature_ref(logits, labels, K)
    fit, got = _fit(logits, labels, K)
    assert want[3] == 0 and got["status"] == "ok" and got["temperature"] == 1.0 / got["beta"]
    err = abs(got["beta"] - want[0]) / want[0]
    e_nll = max(abs(got["nll_before"] - want[1]), abs(got["nll_after"] - want[2]))
    print(f"M={M} K={K}: beta {got['beta']:.6g}, relative error {err:.3g}; NLL error {e_nll:.3g}")
    _log(f"fit M={M} K={K} beta (relative)", err, BETA_GATE)
    _log(f"fit M={M} K={K} nll", e_nll, sum_bound(M))
    assert err <= BETA_GATE and e_nll <= sum_bound(M)
    assert got["nll_after"] <= got["nll_before"] + sum_bound(M)
    assert fit.info.cpu().numpy().tobytes() == calibration.fit_temperature(*_dev(logits, labels), K).info.cpu().numpy().tobytes()  # bitwise
    # padding rows and an abstention column do not move beta beyond the gate
    rng = np.random.default_rng(M)
    at = rng.integers(0, M + 1, max(M // 8, 2))
    lg2 = np.insert(np.concatenate([logits, 9 * rng.standard_normal((M, 1)).astype(np.float32)], 1), at, 40.0, axis=0)
    lb2 = np.insert(labels, at, np.where(np.arange(at.size) % 2 == 0, -1, K))
    _, pad = _fit(lg2, lb2, K)
    err = abs(pad["beta"] - want[0]) / want[0]
    _log(f"fit M={M} K={K} beta with padding rows (relative)", err, BETA_GATE)
    assert pad["status"] == "ok" and err <= BETA_GATE and abs(pad["nll_after"] - want[2]) <= sum_bound(M)


def test_fit_at_the_bounds_and_without_rows():
    for case, status, beta in ((cc.separable_case, "upper_bound", 64.0), (cc.all_wrong_case, "lower_bound", 1 / 64)):
        logits, labels = case(257, 4)
        want = cc.temperature_ref(logits, labels, 4)
        _, got = _fit(logits, labels, 4)
        assert got["status"] == status and got["beta"] == beta == want[0] and got["temperature"] == 1 / beta
        assert abs(got["nll_before"] - want[1]) <= sum_bound(257) and abs(got["nll_after"] - want[2]) <= sum_bound(257)
        assert got["nll_after"] <= got["nll_before"]
    _, flat = _fit(np.zeros((5, 3), np.float32), np.array([0, 1, 2, 0, 1]), 3)  # g' = 0 everywhere
    assert flat["status"] == "lower_bound" and flat["beta"] == 1 / 64 and abs(flat["nll_after"] - np.log(3)) <= 1e-15
    _, empty = _fit(np.ones((300, 3), np.float32), -np.ones(300, np.int64), 3)
    assert empty["status"] == "empty" and empty["beta"] == 1.0 and np.isnan(empty["nll_before"]) and np.isnan(empty["nll_after"])


# ---- scaled probabilities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,extra", [(1, 2, 0), (257, 4, 1), (5000, 16, 1), (5000, 3, 0)])
def test_scaled_probs_within_one_ulp(M, K, extra):
    logits, labels = cc.logit_case(M, K, 3.0, seed=M, extra=extra)
    d_logits, d_labels = _dev(logits, labels)
    fit = calibration.fit_temperature(d_logits, d_labels, K)
    for temperature, beta in ((fit, float(fit.beta.cpu())), (2.5, 1 / 2.5), (0.02, 1 / 0.02)):
        p, u = calibration.scaled_probs(d_logits, K, temperature, with_u=True)
        assert p.dtype == u.dtype == torch.float32 and p.shape == (M, K) and u.shape == (M,)
        want = cc.scaled_probs_ref(logits, K, beta)
        got = p.cpu().numpy()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))  # non-negative floats: bit patterns are ordered
        print(f"M={M} K={K} beta={beta:.4g}: {int((ulps > 0).sum())} of {ulps.size} differ, by at most {int(ulps.max())} ulp")
        _log(f"scaled probs M={M} K={K} beta={beta:.4g} (fp32 ulps)", float(ulps.max()), 1)
        assert ulps.max() <= 1
        assert np.array_equal(u.cpu().numpy(), np.float32(1.0) - got.max(1))  # bitwise 1.0f - the largest
        assert torch.equal(calibration.scaled_probs(d_logits, K, temperature), p)


# ---- through the public entries ------------------------------------------------------------------------------------------------------------
def _close(a, b, gate):
    """Nested dicts / lists of numbers equal within ``gate`` (integers exactly), NaN in the same places."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_close(a[k], b[k], gate) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_close(x, y, gate) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= gate
    return a == b


def _want_calibration(probs, labels, u, groups, n_bins, B, seed, confidence):
    """(res["calibration"], the six calibration keys of res["ci"]) from the restatement, for device rows."""
    p, y, uu = probs.cpu().numpy(), labels.cpu().numpy(), u.cpu().numpy()
    main = cc.reliability_ref(p, y, n_bins, None, groups, B, seed)
    sel = cc.reliability_ref(p, y, n_bins, np.float32(1.0) - uu, None, 0)
    want = cc.summary_ref({k: v[B] for k, v in main.items()}, n_bins)
    s = cc.summary_ref({k: v[0] for k, v in sel.items()}, n_bins)
    want["selective"] = {k: s[k] for k in ("ece", "mce", "conf_gap", "bins")}
    return want, bootstrap.intervals_of(main["stats"], confidence, names=cc.STAT_NAMES) if B else None


@pytest.mark.parametrize("abstain", [True, False])
def test_selective_evaluator_finish_with_calibration_and_temperature(abstain, monkeypatch):
    rng = np.random.default_rng(16)
    Bt, nb, K = 7, 9, 4
    Kr = K - 1 if abstain else K
    names = [f"cine{g}" for g in range(11)]
    keys = [names[int(g)] for g in rng.integers(0, len(names), Bt * nb)]  # repeated file names, interleaved
    y = np.array([names.index(k) % 3 for k in keys])
    lg = np.random.default_rng(17).uniform(-4.0, 4.0, (Bt * nb, K)).astype(np.float32)
    lg[np.arange(Bt * nb), y] += 2.0  # the labels can be learned: an interior temperature
    sel = selective.SelectiveEvaluator(_Head().to(DEV), abstain_class=abstain, capacity=8)
    for b in range(nb):
        s = slice(b * Bt, (b + 1) * Bt)
        sel.update(torch.from_numpy(lg[s]).to(DEV), torch.rand(Bt, 8, device=DEV), torch.from_numpy(y[s]).to(DEV), keys[s])
    logits, labels = sel.ev.logits[: sel.ev.rows], sel.ev.labels[: sel.ev.rows]
    fit = calibration.fit_temperature(logits, labels, Kr)
    assert fit.read()["status"] == "ok"
    probs, u = calibration.scaled_probs(logits, Kr, fit, with_u=True)  # (held to the restatement above)
    if abstain:
        u = selective.uncertainty(logits, True)  # alpha keeps reading the raw logits
    groups = selective.build_groups(keys)
    reads = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: reads.append(t.numel()) or to_host(t, *a, **k))
    for level, unit in (("clip", "cine"), ("clip", "clip"), ("cine", "cine")):
        del reads[:]
        res = sel.finish(level=level, bootstrap=33, seed=3, confidence=0.9, unit=unit, calibration=15, temperature=fit)
        assert len(reads) == 1, (level, reads)  # one synchronising read
        plain = sel.finish(level=level, bootstrap=33, seed=3, confidence=0.9, unit=unit, temperature=fit)
        assert "calibration" not in plain and list(plain["ci"]) == list(bootstrap.STAT_NAMES)
        assert list(res["ci"]) == list(bootstrap.STAT_NAMES) + list(cc.STAT_NAMES)
        rest = {k: v for k, v in res.items() if k != "calibration"}
        rest["ci"] = {k: v for k, v in res["ci"].items() if k in bootstrap.STAT_NAMES}
        assert _close(rest, plain, 0.0)  # every other key is bitwise the call without calibration
        if level == "clip":
            rows = (probs, labels, u, groups if unit == "cine" else None)
            want_rc = selective.risk_coverage(probs, labels, u).at((1.0,))  # the scored probabilities are the scaled ones
        else:
            gp = selective.group_predictions(probs, u, labels, groups)
            rows = (gp.p_conf.float(), gp.labels, gp.u_mean.float(), None)
            want_rc = selective.risk_coverage(*rows[:3]).at((1.0,))
        assert res["aurc"] == want_rc["aurc"] and res["accuracy@1"] == want_rc["accuracy"][0]
        want, want_ci = _want_calibration(*rows, 15, 33, 3, 0.9)
        assert _close(res["calibration"], want, GATE), (level, unit)
        assert _close({k: res["ci"][k] for k in cc.STAT_NAMES}, want_ci, GATE), (level, unit)
        assert res["ci"]["ece"]["n_finite"] == 33 and abs(res["ci"]["nll"]["point"] - res["calibration"]["nll"]) <= GATE
        assert sum(b["n"] for b in res["calibration"]["bins"]) == res["rows"] == sum(b["n"] for b in res["calibration"]["selective"]["bins"])
    # without a temperature the rows are the evaluator's own probabilities
    res = sel.finish(level="clip", calibration=10)
    u0 = selective.uncertainty(logits, abstain)
    want, _ = _want_calibration(sel.ev.probs[: sel.ev.rows], labels, u0, None, 10, 0, 0, 0.9)
    assert "ci" not in res and _close(res["calibration"], want, GATE)


@pytest.mark.timeout(900)
def test_trainer_fit_temperature_and_evaluate_selective(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to(DEV)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    loader = _cine_loader(4, 3, 70)
    logs = []
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda s, *_: logs.append(str(s)))
    with pytest.raises(ValueError, match="fit_temperature"):
        t.evaluate_selective("test", calibration=15, temperature="fitted")
    with pytest.raises(ValueError, match="temperature"):
        t.evaluate_selective("test", temperature="fit")
    state = (t.current_epoch, t.current_iteration, m.training)
    fit = t.fit_temperature("val")
    assert (t.current_epoch, t.current_iteration, m.training) == state and any("temperature" in s and "NLL" in s for s in logs)
    assert fit == t.temperature_fit.read() and fit["status"] in calibration.STATUS_NAMES and fit["nll_after"] <= fit["nll_before"] + sum_bound(12)
    # the same sweep fed by hand
    sel = selective.SelectiveEvaluator(m, abstain_class=True)
    with torch.no_grad():
        for b in loader:
            lg, sim, _ = m(b["cine"].to(DEV))
            sel.update(lg, sim, b["target_AS"].to(DEV), b["filename"])
    ev = sel.ev
    assert fit == calibration.fit_temperature(ev.logits[: ev.rows], ev.labels[: ev.rows], 3).read()
    want = cc.temperature_ref(ev.logits[: ev.rows].cpu().numpy(), ev.labels[: ev.rows].cpu().numpy(), 3)
    assert fit["status"] == calibration.STATUS_NAMES[want[3]] and abs(fit["beta"] - want[0]) <= BETA_GATE * want[0]
    res = t.evaluate_selective("test", level="clip", calibration=15, temperature="fitted", bootstrap=16, seed=5)
    assert _close(res, sel.finish(level="clip", calibration=15, temperature=t.temperature_fit, bootstrap=16, seed=5), 0.0)
    assert list(res["ci"]) == list(bootstrap.STAT_NAMES) + list(cc.STAT_NAMES) and res["ci"]["brier"]["n_finite"] == 16
    with open(tmp_path / "csv_test_reliability" / "e00.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["bin", "lo", "hi", "n", "accuracy", "confidence"] and len(rows) == 16 and [int(r[0]) for r in rows[1:]] == list(range(15))
    assert sum(int(r[3]) for r in rows[1:]) == 12 == res["rows"]
    for r, b in zip(rows[1:], res["calibration"]["bins"]):
        assert _close([float(r[1]), float(r[2]), int(r[3]), float(r[4]), float(r[5])], [b["lo"], b["hi"], b["n"], b["accuracy"], b["confidence"]], 0.0)
    cine = t.evaluate_selective("test", level="cine", calibration=15, temperature=2.0)
    assert cine["groups"] == 3 and sum(b["n"] for b in cine["calibration"]["bins"]) == 3 and sorted(os.listdir(tmp_path)) == [
        "csv_test_cine", "csv_test_reliability"]
    assert "calibration" not in t.evaluate_selective("test", level="clip")
