"""GPU: the ordinal evaluation (csrc/ordinal.hip through protoasnet_amd.ordinal) against the float64 / int64 numpy restatement of
tests/ordinal_cases.py, and through SelectiveEvaluator.finish and DPTrainer.fit_operating_points / evaluate_selective.

Held exact: every tally, P, N, U2, every threshold and the confusion integers.  Held bitwise: the six agreement numbers and the AUC (each
a single fp64 expression of integers).  ap: within M 2^-50 (include/protoasnet_amd.h: the two sides sum the same terms in different
orders); the observed error is printed."""
import numpy as np
import pytest
import torch

import bootstrap_cases as bc
import ordinal_cases as oc
from protoasnet_amd import bootstrap, ordinal, selective
from test_cpu_trainer import TRAIN_CFG
from test_gpu_selective import _cine_loader, _Head
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = bootstrap.lds_max_groups  # read through the library when a test runs (collection must not need the library)
KEYS = ("pn", "u2", "stats", "op_theta", "op_tally", "fix_tally")


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _host(scr):
    return {k: getattr(scr, k).cpu().numpy() for k in KEYS}


def _same_bits(a, b):
    """Byte for byte (so +0 is not -0), after every NaN has been given one payload."""
    a, b = np.ascontiguousarray(a).copy(), np.ascontiguousarray(b).copy()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a[np.isnan(a)], b[np.isnan(b)] = np.nan, np.nan
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _compare(got, want, M, name):
    for k in ("pn", "u2", "op_tally", "fix_tally"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4])
    assert _same_bits(got["op_theta"], want["op_theta"]), (name, "theta", got["op_theta"].ravel()[:8], want["op_theta"].ravel()[:8])
    assert _same_bits(got["stats"][..., 0], want["stats"][..., 0]), (name, "auc")
    ga, wa = got["stats"][..., 1], want["stats"][..., 1]
    assert np.array_equal(np.isnan(ga), np.isnan(wa)), (name, "ap NaN")
    err = float(np.nanmax(np.abs(ga - wa))) if np.isfinite(wa).any() else 0.0
    print(f"{name}: max |ap - restatement| = {err:.3g} (gate {M * 2.0 ** -50:.3g})")
    assert err <= M * 2.0 ** -50, (name, err)


def _check(probs, labels, spec=(0.9,), sens=(0.9,), groups=None, B=0, seed=0, fixed=None, name="", counts=None):
    """``fixed`` (C, F) rides in as the thresholds of an OperatingFit-shaped tensor through ``net_benefit_at``-free plumbing: the fit."""
    K = probs.shape[1]
    fit = None
    if fixed is not None:
        fit = _RawFit(torch.from_numpy(np.asarray(fixed, dtype=np.float32).reshape(K - 1, -1)).to(DEV))
    scr = ordinal.screen(*_dev(probs, labels), specificities=spec, sensitivities=sens, groups=groups, B=B, seed=seed, fit=fit)
    got = _host(scr)
    assert scr.pn.dtype == torch.int64 and scr.stats.dtype == torch.float64 and scr.op_theta.dtype == torch.float32
    want = oc.screen_ref(probs, labels, spec, sens, groups, B, seed, fixed, counts)
    _compare(got, want, probs.shape[0], name)
    return scr, got, want


class _RawFit(ordinal.OperatingFit):
    """Any (C, F) thresholds as a fit: the kernel's fixed-threshold input without the naming of a real fit."""

    def __init__(self, thresholds):
        self.thresholds, self.K = thresholds, thresholds.shape[0] + 1
        self.kinds, self.targets = ["youden"] * thresholds.shape[1], [None] * thresholds.shape[1]
        self.specificities, self.sensitivities = [], []


# ---- agreement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 2), (257, 3), (3 * 256 + 5, 4), (1025, 16)])
def test_agreement_is_the_restatement_bitwise(M, K):
    probs, labels = oc.ordinal_case(M, K, seed=M + K, pad=0.15)
    agr = ordinal.agreement(*_dev(probs, labels))
    cm = oc.confusion_ref(probs, labels)
    assert agr.cm.dtype == torch.int64 and np.array_equal(agr.cm.cpu().numpy()[0], cm)
    assert _same_bits(agr.stats.cpu().numpy()[0], oc.agreement_ref(cm)), (M, K)
    assert list(agr.read()) == list(ordinal.AGREEMENT_NAMES)


def test_agreement_edge_cases():
    cms = np.zeros((4, 3, 3), dtype=np.int64)
    cms[1, 1, 1] = 7  # one cell: E = 0 -> both kappas NaN, the rest defined
    cms[2] = np.arange(9).reshape(3, 3)
    cms[3] = np.eye(3) * 5  # perfect: kappa 1
    got = ordinal.agreement_of(torch.from_numpy(cms).to(DEV)).stats.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[1, 4:]).all() and got[1, :4].tolist() == [0.0, 1.0, 0.0, 0.0]
    for r in range(4):
        assert _same_bits(got[r], oc.agreement_ref(cms[r])), r
    assert got[3, 4] == 1.0 and got[3, 5] == 1.0


def test_agreement_of_the_bootstrap_confusion_matrices():
    """``agreement_of(bootstrap.replicates(...).cm)``: every replicate and the point estimate in one launch, on the bootstrap's own
    resamples; equal to the restatement applied per replicate."""
    probs, labels = oc.ordinal_case(700, 4, seed=3, pad=0.1)
    keys = bc.random_groups(700, seed=4)
    groups = selective.build_groups(keys)
    B, seed = 12, 77
    rep = bootstrap.replicates(*_dev(probs, labels), None, groups, B, seed)
    agr = ordinal.agreement_of(rep.cm)
    got = agr.stats.cpu().numpy()
    counts = np.concatenate([bc.counts_ref(len(groups[2]), B, seed), np.ones((1, len(groups[2])), dtype=np.int32)])
    for b in range(B + 1):
        cm = oc.confusion_ref(probs, labels, oc.weights_ref(counts[b], labels, 4, groups))
        assert _same_bits(got[b], oc.agreement_ref(cm)), b
    ci = ordinal.intervals(agr)
    assert list(ci) == list(ordinal.AGREEMENT_NAMES) and ci["mae"]["n_finite"] == B and ci["mae"]["point"] == got[B, 0]


def test_cut_scores():
    probs, _ = oc.ordinal_case(513, 5, seed=9, denom=1 << 20)  # inexact fp32 sums: the order of the adds shows
    assert _same_bits(ordinal.cut_scores(torch.from_numpy(probs).to(DEV)).cpu().numpy(), oc.cut_scores_ref(probs))


# ---- cuts: shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 2), (255, 3), (256, 2), (257, 4), (1025, 3), (2047, 2), (2048, 3), (300, 16)])
def test_screen_shapes_without_replicates(M, K):
    """B = 0; the rank tile (255 / 256 / 257), a second rank chunk (1025), the sweep chunk with and without room for the END position
    (2047 / 2048), one cut and fifteen.  Sixteenths: tie groups straddle thread, wave and tile boundaries."""
    probs, labels = oc.ordinal_case(M, K, seed=10 * M + K)
    fixed = np.tile(np.array([0.0, 0.25, 0.5, 1.0, 1.5, np.nan], dtype=np.float32), (K - 1, 1))
    _check(probs, labels, (0.5, 0.9), (0.5, 0.9), fixed=fixed, name=f"M={M} K={K}")


def test_screen_padding_groups_and_replicates():
    """M = 3 * 256 + 5 with about 15 % padding rows interleaved, groups whose rows are not neighbours, rows that no group lists, units
    drawn zero times; the maximum number of targets and of fixed thresholds."""
    M, K, B, seed = 3 * 256 + 5, 4, 6, (5 << 32) | 11
    probs, labels = oc.ordinal_case(M, K, seed=21, pad=0.15)
    keys = bc.random_groups(M, seed=22)
    offsets, rows, names = selective.build_groups(keys)
    offsets, rows = offsets[:-3], rows[: offsets[-4]]  # the rows of the last three groups are listed by nobody
    groups = (offsets, rows)
    counts = bc.counts_ref(len(offsets) - 1, B, seed)
    assert (counts == 0).any() and (counts > 1).any()
    spec = tuple(np.linspace(0.15, 0.97, ordinal.MAX_TARGETS))
    sens = tuple(np.linspace(0.2, 0.99, ordinal.MAX_TARGETS))
    rng = np.random.default_rng(23)
    fixed = (rng.integers(-1, 18, (K - 1, ordinal.MAX_FIXED)) / 16.0).astype(np.float32)
    scr, got, want = _check(probs, labels, spec, sens, groups, B, seed, fixed, "padded, grouped")
    again = _host(ordinal.screen(*_dev(probs, labels), specificities=spec, sensitivities=sens, groups=groups, B=B, seed=seed, fit=scr.fit))
    for k in KEYS:  # two calls are bitwise equal
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    # replicate b is the restatement fed with the counts the device itself draws, and the multiset of bootstrap.replicates
    d_counts = bootstrap.draw_counts(len(offsets) - 1, B, seed).cpu().numpy()
    fed = oc.screen_ref(probs, labels, spec, sens, groups, B, seed, fixed, counts=d_counts)
    _compare(got, fed, M, "device counts")
    rep = bootstrap.replicates(*_dev(probs, labels), None, groups, B, seed)
    assert np.array_equal(rep.cm.sum(dim=(1, 2)).cpu().numpy(), got["pn"][:, 0].sum(axis=1))


def test_screen_one_group():
    probs, labels = oc.ordinal_case(130, 3, seed=31)
    groups = (np.array([0, 130], dtype=np.int64), np.arange(130, dtype=np.int32))
    _, got, _ = _check(probs, labels, groups=groups, B=2, seed=1, name="G=1")
    assert np.array_equal(got["pn"][0], got["pn"][2])  # the one unit is drawn once


def test_screen_counts_on_both_sides_of_the_lds_bound():
    """G = lds_max_groups() and G + 1, every row its own unit, B = 3: counts in LDS, and in the workspace slice."""
    for G in (BOUND(), BOUND() + 1):
        probs, labels = oc.ordinal_case(G, 3, seed=G, denom=64)
        _check(probs, labels, (0.8,), (0.8,), B=3, seed=G, fixed=np.array([[0.5], [0.25]], dtype=np.float32), name=f"G={G}")


# ---- cuts: named cases -------------------------------------------------------------------------------------------------------------------
def test_all_scores_equal():
    """One tie group: AUC exactly 0.5, ap = prevalence, and the only candidate that reaches a specificity besides the common score (which
    reaches none: everyone is positive there) is +inf."""
    M, K = 600, 3
    probs = np.tile(np.array([[0.5, 0.25, 0.25]], dtype=np.float32), (M, 1))
    labels = (np.arange(M) % K).astype(np.int32)
    _, got, _ = _check(probs, labels, (0.5,), (0.5,), name="all equal")
    assert got["stats"][0, :, 0].tolist() == [0.5, 0.5]
    assert got["stats"][0, 0, 1] == 400 / 600 and got["stats"][0, 1, 1] == 200 / 600
    assert np.isposinf(got["op_theta"][0, :, 0]).all() and (got["op_tally"][0, :, 0] == 0).all()
    assert got["op_theta"][0, :, 1].tolist() == [0.5, 0.25] and got["op_tally"][0, 0, 1].tolist() == [400, 200]
    assert np.isposinf(got["op_theta"][0, :, 2]).all()  # Youden: J = 0 everywhere, ties to the larger theta


def test_a_cut_without_positives_is_confined():
    """No row of the top grade: that cut has NaN auc, ap and thresholds, its tallies are written, and its neighbours are untouched --
    in the sample and inside a single replicate (three units, one holding every top-grade row, replicates that never draw it)."""
    M, K = 400, 4
    probs, labels = oc.ordinal_case(M, K, seed=41)
    labels[labels == 3] = 2
    fixed = np.full((K - 1, 2), 0.25, dtype=np.float32)
    _, got, _ = _check(probs, labels, fixed=fixed, name="no positives")
    assert np.isnan(got["stats"][0, 2]).all() and np.isnan(got["op_theta"][0, 2]).all() and got["pn"][0, 2].tolist() == [0, M]
    assert np.isfinite(got["stats"][0, :2]).all() and got["fix_tally"][0, 2, 0, 1] > 0
    probs, labels = oc.ordinal_case(M, K, seed=42)
    top, rest = np.flatnonzero(labels == 3), np.flatnonzero(labels != 3)
    groups = (np.array([0, 150, len(rest), M], dtype=np.int64), np.concatenate([rest, top]).astype(np.int32))
    B, seed = 8, 5
    counts = bc.counts_ref(3, B, seed)
    lost = [b for b in range(B) if counts[b, 2] == 0]
    assert lost and len(lost) < B and (counts[:, :2].sum(axis=1) > 0).all()
    _, got, _ = _check(probs, labels, groups=groups, B=B, seed=seed, fixed=fixed, name="a replicate without positives")
    for b in range(B):
        assert np.isnan(got["stats"][b, 2]).all() == (b in lost) and np.isfinite(got["stats"][b, :2]).all()


def test_a_sensitivity_met_only_at_the_lowest_candidate():
    """The lowest score belongs to a positive: sensitivity 0.999 needs every positive, so theta is the lowest candidate."""
    probs, labels = oc.ordinal_case(500, 2, seed=51)
    probs[7], labels[7] = [1.0, 0.0], 1
    _, got, _ = _check(probs, labels, (0.9,), (0.999,), name="lowest candidate")
    assert got["op_theta"][0, 0, 1] == 0.0 and got["op_tally"][0, 0, 1].tolist() == got["pn"][0, 0].tolist()


def test_a_youden_tie_goes_to_the_larger_threshold():
    """Scores 1/4 (neg), 1/2 (pos), 1/2 (neg), 3/4 (pos): J = TP N - FP P is 0, 2, 2, 0 at 1/4, 1/2, 3/4, +inf -> 3/4."""
    probs = np.array([[0.75, 0.25], [0.5, 0.5], [0.5, 0.5], [0.25, 0.75]], dtype=np.float32)
    labels = np.array([0, 1, 0, 1], dtype=np.int32)
    _, got, _ = _check(probs, labels, (), (), name="youden tie")
    assert got["op_theta"][0, 0, 0] == 0.75 and got["op_tally"][0, 0, 0].tolist() == [1, 0]


def test_a_fit_from_one_split_applied_on_another():
    """The applied tallies are a plain count of s >= theta on the other split."""
    K = 4
    val, test = oc.ordinal_case(900, K, seed=61), oc.ordinal_case(1100, K, seed=62, pad=0.1)
    fit = ordinal.fit_operating_points(*_dev(*val), specificities=(0.8, 0.95), sensitivities=(0.9,))
    want_fit = oc.screen_ref(*val, (0.8, 0.95), (0.9,))["op_theta"][0]
    assert fit.K == K and fit.kinds == ["specificity", "specificity", "sensitivity", "youden"] and fit.targets == [0.8, 0.95, 0.9, None]
    assert _same_bits(fit.thresholds.cpu().numpy(), want_fit)
    scr = ordinal.screen(*_dev(*test), fit=fit, net_benefit_at=(0.2,), B=5, seed=9)
    got = _host(scr)
    s, w = oc.cut_scores_ref(test[0]), oc.weights_ref(np.ones(1100), test[1], K)
    for c in range(K - 1):
        for t, theta in enumerate(list(want_fit[c]) + [np.float32(0.2)]):
            hit = (s[c] >= theta) & (w > 0)
            assert got["fix_tally"][5, c, t].tolist() == [int((hit & (test[1] >= c + 1)).sum()), int((hit & (test[1] < c + 1)).sum())], (c, t)
    res = scr.read()
    assert [f["kind"] for f in res["cuts"][0]["fitted"]] == fit.kinds and res["cuts"][1]["net_benefit"][0]["pt"] == 0.2
    tp, fp = got["fix_tally"][5, 1, 4]
    P, N = got["pn"][5, 1]
    assert res["cuts"][1]["net_benefit"][0]["net_benefit"] == tp / (P + N) - fp / (P + N) * (0.2 / 0.8)
    assert "cut2/fitted/sens@spec=0.95" in res["ci"] and res["ci"]["cut1/auc"]["point"] == got["stats"][5, 0, 0]
    assert ordinal.intervals(scr) == res["ci"]
    with pytest.raises(ValueError, match="classes"):
        ordinal.screen(*_dev(*oc.ordinal_case(50, 3, seed=1)), fit=fit)


# ---- evaluator and trainer ---------------------------------------------------------------------------------------------------------------
def _close(a, b):
    """Equal, NaN equal to NaN, through dicts and lists."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_close(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_close(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


def test_selective_evaluator_finish_with_ordinal(monkeypatch):
    rng = np.random.default_rng(71)
    Bt, nb, K = 8, 12, 4
    names = [f"cine{g}" for g in range(24)]
    keys = [names[(i * 7) % len(names)] for i in range(Bt * nb)]
    y = np.array([names.index(k) % K for k in keys])
    lg = rng.uniform(-2.0, 2.0, (Bt * nb, K)).astype(np.float32)
    lg[np.arange(Bt * nb), y] += 1.0
    sel = selective.SelectiveEvaluator(_Head().to(DEV), abstain_class=False, capacity=8)
    for b in range(nb):
        s = slice(b * Bt, (b + 1) * Bt)
        sel.update(torch.from_numpy(lg[s]).to(DEV), torch.rand(Bt, 8, device=DEV), torch.from_numpy(y[s]).to(DEV), keys[s])
    probs, labels = sel.ev.probs[: sel.ev.rows], sel.ev.labels[: sel.ev.rows]
    u = selective.uncertainty(sel.ev.logits[: sel.ev.rows], False)
    groups = selective.build_groups(keys)
    B, seed = 16, 2
    reads, to_host = [], torch.Tensor.cpu
    for level in ("clip", "cine"):
        if level == "clip":
            rows, g = (probs, labels), groups[:2]
        else:
            gp = selective.group_predictions(probs, u, labels, groups)
            rows, g = (gp.p_conf.float(), gp.labels), None
        p_h, l_h = rows[0].cpu().numpy(), rows[1].cpu().numpy()
        # the restatement's own replicates are all finite for this seed: asserted on the restatement first
        want = oc.screen_ref(p_h, l_h, (0.9,), (0.9,), g, B, seed)
        assert np.isfinite(want["stats"]).all() and (want["pn"] > 0).all()
        fit = ordinal.fit_operating_points(*rows, specificities=(0.8,), sensitivities=(0.8,))
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "cpu", lambda t, *a, **k: reads.append(t.numel()) or to_host(t, *a, **k))
            del reads[:]
            res = sel.finish(level=level, ordinal=True, bootstrap=B, seed=seed)
            assert len(reads) == 1, (level, reads)  # one synchronising read
            fitted = sel.finish(level=level, ordinal=fit, ordinal_net_benefit_at=(0.3,), calibration=5)
            old = sel.finish(level=level, bootstrap=B, seed=seed)
        alone = ordinal.screen(*rows, groups=g, B=B, seed=seed).read()
        agr = ordinal.agreement(*rows).read()
        assert _close(res["ordinal"], {"agreement": agr, "cuts": alone["cuts"]}), level
        assert _same_bits(np.array([res["ordinal"]["cuts"][c]["auc"] for c in range(K - 1)]), want["stats"][B, :, 0])
        assert _close({k: v for k, v in res.items() if k != "ordinal" and k != "ci"}, {k: v for k, v in old.items() if k != "ci"})
        assert list(res["ci"])[:6] == list(bootstrap.STAT_NAMES) and _close({k: res["ci"][k] for k in bootstrap.STAT_NAMES}, old["ci"])
        new = [k for k in res["ci"] if k not in bootstrap.STAT_NAMES]
        assert set(new) == set(ordinal.AGREEMENT_NAMES) | set(alone["ci"]) and all(res["ci"][k]["n_finite"] == B for k in new), level
        assert _close({k: res["ci"][k] for k in alone["ci"]}, alone["ci"])
        applied = ordinal.screen(*rows, specificities=(0.8,), sensitivities=(0.8,), fit=fit, net_benefit_at=(0.3,)).read()
        assert _close(fitted["ordinal"]["cuts"], applied["cuts"]) and "fitted" in fitted["ordinal"]["cuts"][0] and "calibration" in fitted
        assert "ci" not in fitted and fitted["ordinal"]["cuts"][0]["fitted"][0]["tp"] == fitted["ordinal"]["cuts"][0]["operating_points"][0]["tp"]


@pytest.mark.timeout(900)
def test_trainer_fit_operating_points_and_evaluate_selective(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to(DEV)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    loader = _cine_loader(4, 3, 70)
    logs = []
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda s, *_: logs.append(str(s)))
    with pytest.raises(ValueError, match="fit_operating_points"):
        t.evaluate_selective("test", ordinal="fitted")
    state = (t.current_epoch, t.current_iteration, m.training)
    got = t.fit_operating_points("val", specificities=(0.7,), sensitivities=(0.7,))
    assert (t.current_epoch, t.current_iteration, m.training) == state and any("operating points (cine)" in s for s in logs)
    assert got == t.operating_fit.read() and got["K"] == 3 and got["kinds"] == ["specificity", "sensitivity", "youden"]
    sel = selective.SelectiveEvaluator(m, abstain_class=True)
    with torch.no_grad():
        for b in loader:
            lg, sim, _ = m(b["cine"].to(DEV))
            sel.update(lg, sim, b["target_AS"].to(DEV), b["filename"])
    ev = sel.ev
    gp = selective.group_predictions(ev.probs[: ev.rows], selective.uncertainty(ev.logits[: ev.rows], True), ev.labels[: ev.rows],
                                     selective.build_groups(sel.keys))
    want = oc.screen_ref(gp.p_conf.float().cpu().numpy(), gp.labels.cpu().numpy(), (0.7,), (0.7,))["op_theta"][0]
    assert _same_bits(t.operating_fit.thresholds.cpu().numpy(), want)
    res = t.evaluate_selective("test", level="cine", ordinal="fitted")
    assert _close(res, sel.finish(level="cine", ordinal=t.operating_fit)) and any("| ordinal (cine) |" in s for s in logs)
    assert len(res["ordinal"]["cuts"]) == 2 and len(res["ordinal"]["cuts"][0]["fitted"]) == 3
    assert "ordinal" not in t.evaluate_selective("test", level="clip")
    # with a temperature the fit is made on the rows evaluate_selective(temperature=) scores: applied to them, a fitted threshold
    # gives the tallies of its own operating point
    t.fit_operating_points("val", specificities=(0.7,), sensitivities=(0.7,), temperature=1.7)
    res = t.evaluate_selective("test", level="cine", ordinal="fitted", temperature=1.7)
    assert _close(res["ordinal"], sel.finish(level="cine", ordinal=t.operating_fit, temperature=1.7)["ordinal"])
    for c in res["ordinal"]["cuts"]:
        for f, o in zip(c["fitted"], c["operating_points"]):
            assert (f["tp"], f["fp"]) == (o["tp"], o["fp"]), c["cut"]
    assert "ordinal" in t.evaluate_selective("test", level="clip", ordinal=True)
