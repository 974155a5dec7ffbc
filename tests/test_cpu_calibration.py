"""CPU: calibration -- the numpy restatement of tests/calibration_cases.py (what the GPU tests hold the kernels to) against cases worked
out by hand, the fit's restatement on the cases the GPU tests call interior, and the C-ABI / Python surface with its argument checks."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import calibration_cases as cc
import protoasnet_amd
from protoasnet_amd import _lib, bootstrap, calibration, selective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_calibration_workspace_bytes", "pasn_calibration_bins", "pasn_temperature_workspace_bytes", "pasn_temperature_fit",
               "pasn_temperature_probs")

# eighths: exact in fp32, and every product below is exact in fp64
HAND_PROBS = np.array([[0.75, 0.125, 0.125], [0.125, 0.75, 0.125], [0.375, 0.375, 0.25], [0.25, 0.375, 0.375]], dtype=np.float32)
HAND_LABELS = np.array([0, 0, 0, 2])


# ---- the restatement by hand ---------------------------------------------------------------------------------------------------------------
def test_four_rows_into_two_bins_by_hand():
    """Predictions (first largest) 0, 1, 0, 1 against labels 0, 0, 0, 2: hit, miss, hit (the tie goes to class 0), miss.  Confidences
    0.75, 0.75 (bin 1) and 0.375, 0.375 (bin 0)."""
    r = cc.bins_of_weights(HAND_PROBS, HAND_LABELS, [1, 1, 1, 1], 2)
    assert r["n"].tolist() == [2, 2] and r["hit"].tolist() == [1, 1] and r["skipped"] == 0
    assert r["qsum"].tolist() == [3 << 30, 3 << 31]  # 0.75 and 1.5 times 2^32
    # conf_j - hit_j: 0.75 - 1 and 1.5 - 1
    ece, mce, cw, brier, nll, gap = r["stats"]
    assert ece == (0.25 + 0.5) / 4 and mce == 0.25 and gap == (-0.25 + 0.5) / 4
    # class 0: column 0.75 | 0.125 0.375 0.25, positives rows 0 1 2: bin 0 |2 - 0.75|, bin 1 |1 - 0.75|; class 1: no positive, 0.875 and
    # 0.75 of confidence; class 2: all four in bin 0, one positive, 0.875 of confidence
    assert r["cn"].tolist() == [[3, 1], [3, 1], [4, 0]] and r["cpos"].tolist() == [[2, 1], [0, 0], [1, 0]]
    assert cw == (1.25 + 0.25 + 0.875 + 0.75 + 0.125) / 4 / 3
    assert brier == (0.09375 + 1.34375 + 0.59375 + 0.59375) / 4
    assert np.isclose(nll, -(np.log(0.75) + np.log(0.125) + 2 * np.log(0.375)) / 4, rtol=1e-15, atol=0)
    # a replicate: row 0 twice, row 1 not at all; a padding row never counts, whatever its weight
    labels = np.append(HAND_LABELS, [-1, 3])
    probs = np.concatenate([HAND_PROBS, HAND_PROBS[:2]])
    r = cc.bins_of_weights(probs, labels, [2, 0, 1, 1, 5, 5], 2)
    assert r["n"].tolist() == [2, 2] and r["hit"].tolist() == [1, 2] and r["qsum"].tolist() == [3 << 30, 3 << 31]
    assert r["stats"][0] == (0.25 + 0.5) / 4 and r["stats"][5] == (-0.25 - 0.5) / 4 and r["stats"][3] == (2 * 0.09375 + 2 * 0.59375) / 4
    # nothing enters: every statistic is NaN
    r = cc.bins_of_weights(probs, labels, [0, 0, 0, 0, 1, 1], 2)
    assert r["n"].sum() == 0 and np.isnan(r["stats"]).all()


def test_bin_edges_and_skipped_confidences():
    """(double)0.3f * 10 = 3.0000001... and (double)0.7f * 10 = 6.9999999...: bins 3 and 6.  1.0 lands in the last bin; NaN, 1.5 and a
    negative confidence are counted in `skipped`, weighted."""
    assert [cc.bin_of(c, 10) for c in (0.3, 0.7, 0.0, 1.0, 0.1)] == [3, 6, 0, 9, 1]
    assert float(np.float32(0.3)) * 10 > 3 and float(np.float32(0.7)) * 10 < 7
    assert cc.q_of(1.0) == 1 << 32 and cc.q_of(0.0) == 0 and cc.q_of(0.5) == 1 << 31 and cc.bin_of(1.0, 1) == 0 and cc.bin_of(1.0, 64) == 63
    probs = np.tile(HAND_PROBS[:1], (7, 1))
    conf = np.array([0.3, 0.7, 1.0, 0.0, np.nan, 1.5, -0.25], dtype=np.float32)
    r = cc.bins_of_weights(probs, np.zeros(7, int), [1, 1, 1, 1, 2, 3, 4], 10, conf)
    assert r["n"].tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 0, 1] and r["skipped"] == 9 and r["hit"].tolist() == r["n"].tolist()
    assert r["qsum"][9] == 1 << 32 and r["qsum"][3] == cc.q_of(0.3)
    assert r["cn"].sum() == 3 * 13  # the class-wise bins come from probs, never from the override: every row, skipped or not
    # Wv counts the skipped rows: the Brier score is the row's own 0.09375 whatever the override
    assert r["stats"][3] == 0.09375 and np.isclose(r["stats"][0], (0.7 + 0.3 + 0.0 + 1.0) / 4, rtol=1e-7, atol=0)  # |1 - c| of the four binned rows
    # the vectorised histogram is the row-by-row one
    probs, labels = cc.prob_case(300, 4, seed=1, pad=True)
    conf = cc.conf_case(300, seed=2, bad=True)
    w = np.random.default_rng(3).integers(0, 4, 300)
    r = cc.bins_of_weights(probs, labels, w, 15, conf)
    n, qsum, skipped = [0] * 15, [0] * 15, 0
    for i in range(300):
        if 0 <= labels[i] < 4 and w[i]:
            if 0 <= conf[i] <= 1:
                n[cc.bin_of(conf[i], 15)] += int(w[i])
                qsum[cc.bin_of(conf[i], 15)] += int(w[i]) * cc.q_of(conf[i])
            else:
                skipped += int(w[i])
    assert r["n"].tolist() == n and r["qsum"].tolist() == qsum and r["skipped"] == skipped > 0


def test_reliability_ref_rows_and_groups():
    probs, labels = cc.prob_case(37, 3, seed=4, pad=True)
    r = cc.reliability_ref(probs, labels, 10, B=3, seed=5)
    assert r["stats"].shape == (4, 6) and r["n"].shape == (4, 10) and r["cn"].shape == (4, 3, 10) and r["skipped"].shape == (4,)
    point = cc.bins_of_weights(probs, labels, np.ones(37, int), 10)
    assert all(np.array_equal(r[k][3], point[k], equal_nan=True) for k in point)
    import bootstrap_cases as bc

    one = cc.bins_of_weights(probs, labels, bc.counts_ref(37, 3, 5)[1], 10)  # the resamples are the bootstrap's
    assert all(np.array_equal(r[k][1], one[k]) for k in one)
    groups = selective.build_groups(["all"] * 37)  # G = 1: every replicate is the sample
    g = cc.reliability_ref(probs, labels, 10, groups=groups, B=2, seed=5)
    assert all(np.array_equal(g[k][0], g[k][2]) and np.array_equal(g[k][2], point[k]) for k in point)
    part = (groups[0][:1].tolist() + [20], groups[1][:20])  # rows past the 20th are listed nowhere: out of every row, the point's too
    g = cc.reliability_ref(probs, labels, 10, groups=(np.array(part[0]), part[1]), B=1)
    assert g["n"][1].sum() == ((labels[:20] >= 0) & (labels[:20] < 3)).sum() < point["n"].sum()
    s = cc.summary_ref({k: v[3] for k, v in r.items()}, 10)
    assert list(s)[:6] == list(cc.STAT_NAMES) and len(s["bins"]) == 10 and s["bins"][3]["lo"] == 0.3 and s["bins"][9]["hi"] == 1.0
    empty = [b for b in s["bins"] if b["n"] == 0]
    assert empty and all(np.isnan(b["accuracy"]) and np.isnan(b["confidence"]) for b in empty)


# ---- the fit's restatement -----------------------------------------------------------------------------------------------------------------
def test_the_fit_restatement_finds_an_interior_root_on_every_interior_case():
    """Otherwise a GPU test could silently exercise only the bounds.  The root of logits = scale x (the true logits) lies near 1 / scale."""
    for M, K, scale in cc.FIT_CASES:
        logits, labels = cc.logit_case(M, K, scale)
        beta, before, after, status = cc.temperature_ref(logits, labels, K)
        assert status == 0 and cc.BETA_MIN < beta < cc.BETA_MAX, (M, K, beta, status)
        assert after <= before and abs(cc._moments(logits.astype(np.float64), labels, beta)[1]) <= 1e-9 * M, (M, K)
        if M >= 5000:
            assert abs(beta * scale - 1) < 0.1, (M, K, beta)
        padded = np.concatenate([labels, [-1, K]]), np.concatenate([logits, 50 * np.ones((2, K), np.float32)])
        assert cc.temperature_ref(padded[1], padded[0], K)[0] == beta  # padding rows never enter
        wide, _ = cc.logit_case(M, K, scale, extra=1)  # an abstention column is not read
        assert np.array_equal(wide[:, :K], logits) and cc.temperature_ref(wide, labels, K)[0] == beta
    assert cc.temperature_ref(*cc.separable_case(257, 4), 4)[::3] == [64.0, 2]
    assert cc.temperature_ref(*cc.all_wrong_case(257, 4), 4)[::3] == [1 / 64, 1]
    assert cc.temperature_ref(np.zeros((5, 3), np.float32), np.array([0, 1, 2, 0, 1]), 3)[::3] == [1 / 64, 1]  # flat rows: g' = 0 everywhere
    fit = cc.temperature_ref(np.ones((5, 3), np.float32), -np.ones(5, int), 3)
    assert fit[0] == 1.0 and fit[3] == 3 and np.isnan(fit[1]) and np.isnan(fit[2])
    p = cc.scaled_probs_ref(np.array([[0.0, np.log(3.0), 7.0]], np.float32), 2, 1.0)
    assert p.dtype == np.float32 and np.allclose(p, [[0.25, 0.75]], rtol=1e-6) and np.allclose(
        cc.scaled_probs_ref(np.array([[0.0, np.log(3.0)]], np.float32), 2, 2.0), [[0.1, 0.9]], rtol=1e-6)


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------
def test_intervals_of_takes_other_column_names():
    stats = np.zeros((6, 6))
    stats[:5, 0] = [0.1, 0.5, 0.2, 0.4, 0.3]
    stats[5, 0] = 0.3
    ci = bootstrap.intervals_of(stats, 0.5, names=calibration.STAT_NAMES)
    assert list(ci) == ["ece", "mce", "cw_ece", "brier", "nll", "conf_gap"] == list(cc.STAT_NAMES)
    assert ci["ece"] == bootstrap.intervals_of(stats, 0.5)["acc"] and np.isclose(ci["ece"]["lo"], 0.2, rtol=1e-15)
    assert list(bootstrap.intervals_of(stats)) == list(bootstrap.STAT_NAMES)  # the default is the call as it was
    with pytest.raises(ValueError, match="stats"):
        bootstrap.intervals_of(stats, names=("a", "b"))


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        raw = f.read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pasn_\w+)", nm))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
        assert getattr(lib, name) is not None
    assert "calibration" in protoasnet_amd.__all__ and protoasnet_amd.calibration is calibration  # exported lazily, like its neighbours
    assert int(re.search(r"#define PASN_TEMPERATURE_STEPS (\d+)", header).group(1)) == cc.STEPS == 48
    with open(os.path.join(REPO, "protoasnet_amd", "build.py")) as f:
        assert '"calibration.hip"' in f.read()


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def bins(M=100, G=100, K_real=3, n_bins=15, B=5, **null):
        a = dict(probs=fake, labels=fake, conf=0, row_unit=0, counts=fake)
        p = dict(n=fake, hit=fake, qsum=fake, cn=fake, cpos=fake, cq=fake, skipped=fake, stats=fake, workspace=fake)
        a.update({k: v for k, v in null.items() if k in a})
        p.update({k: v for k, v in null.items() if k in p})
        return lib.pasn_calibration_bins(*a.values(), M, G, K_real, n_bins, B, *p.values(), 0)

    size = lib.pasn_calibration_workspace_bytes
    for K_real in (1, 17):
        assert bins(K_real=K_real) == 1 and size(100, 100, K_real, 15, 5) == 0
    with pytest.raises(ValueError, match="K_real"):
        _lib.check(bins(K_real=17))
    for M in (0, (1 << 20) + 1):
        assert bins(M=M, G=M) == 1 and size(M, M, 3, 15, 5) == 0
    for G in (0, 101):
        assert bins(G=G, row_unit=fake) == 1 and size(100, G, 3, 15, 5) == 0
    for n_bins in (0, 65):
        assert bins(n_bins=n_bins) == 1 and size(100, 100, 3, n_bins, 5) == 0
    with pytest.raises(ValueError, match="n_bins"):
        _lib.check(bins(n_bins=65))
    for B in (-1, 65537):
        assert bins(B=B) == 1 and size(100, 100, 3, 15, B) == 0
    assert bins(B=0) == 1 and bins(B=5, counts=0) == 1  # counts is NULL exactly when B == 0
    assert bins(G=50) == 1  # without row_unit every row is its own unit
    with pytest.raises(ValueError, match="G must equal M"):
        _lib.check(bins(G=50))
    for k in ("probs", "labels", "n", "hit", "qsum", "cn", "cpos", "cq", "skipped", "stats", "workspace"):
        assert bins(**{k: 0}) == 1, k
    assert bins(workspace=264) == 1  # misaligned
    # the workspace: per row a 64-bit word for the top label and one per class, the two fp64 terms and the unit -- whatever G, n_bins, B
    assert size(2500, 2500, 3, 15, 100) == size(2500, 7, 3, 64, 0) == 2500 * (8 + 3 * 8 + 16 + 4)

    def fit(M=100, K=4, K_real=3, **null):
        p = dict(logits=fake, labels=fake, fit=fake, workspace=fake)
        p.update(null)
        return lib.pasn_temperature_fit(p["logits"], p["labels"], M, K, K_real, p["fit"], p["workspace"], 0)

    def probs(M=100, K=4, K_real=3, **null):
        p = dict(logits=fake, beta=fake, probs=fake, u=0)
        p.update(null)
        return lib.pasn_temperature_probs(p["logits"], M, K, K_real, p["beta"], p["probs"], p["u"], 0)

    tsize = lib.pasn_temperature_workspace_bytes
    assert tsize(100, 3) > 0 and tsize(100, 3) == tsize(1 << 20, 16)
    for call in (fit, probs):
        for bad in (dict(K_real=1, K=1), dict(K_real=17, K=17), dict(K=2), dict(K=18, K_real=16), dict(M=0), dict(M=(1 << 20) + 1)):
            assert call(**bad) == 1, (call.__name__, bad)
    assert tsize(0, 3) == 0 and tsize((1 << 20) + 1, 3) == 0 and tsize(100, 1) == 0 and tsize(100, 17) == 0
    for k in ("logits", "labels", "fit", "workspace"):
        assert fit(**{k: 0}) == 1, k
    for k in ("logits", "beta", "probs"):
        assert probs(**{k: 0}) == 1, k
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(fit(workspace=0))
    assert fit(workspace=264) == 1


def test_python_surface_checks_its_arguments():
    probs, labels, logits = torch.rand(4, 3), torch.zeros(4, dtype=torch.int64), torch.rand(4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        calibration.reliability(probs, labels)
    with pytest.raises(RuntimeError, match="GPU only"):
        calibration.fit_temperature(logits, labels, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        calibration.scaled_probs(logits, 3, 1.5)
    for bad in (dict(n_bins=0), dict(n_bins=65), dict(n_bins=2.5), dict(n_bins=True), dict(B=-1), dict(B=65537), dict(B=1.5), dict(seed=-1),
                dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            calibration.reliability(probs, labels, **bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "fitted", None, True):
        with pytest.raises(ValueError, match="temperature"):
            calibration.scaled_probs(logits, 3, bad)
    for K in (1, 17, 2.0):
        with pytest.raises(ValueError, match="num_real_classes"):
            calibration.fit_temperature(logits, labels, K)
        with pytest.raises(ValueError, match="num_real_classes"):
            calibration.scaled_probs(logits, K, 1.0)
    # the groups are checked on the host, before anything addresses device memory with them
    for groups, word in (((np.array([0, 2, 4]), np.array([0, 1, 1, 2])), "one group only"), ((np.array([0, 2]), np.array([0, 4])), "lie in"),
                         ((np.array([1, 2]), np.array([0, 1])), "offsets"), ((np.arange(6), np.array([0, 1, 2, 3, 3])), "groups for")):
        with pytest.raises(ValueError, match=word):
            calibration._row_units(groups, 4)
    unit, G = calibration._row_units((np.array([0, 2, 3]), np.array([3, 0, 1])), 4)
    assert unit.tolist() == [0, 1, -1, 0] and G == 2 and unit.dtype == np.int32
    assert unit.tolist() == cc.row_units(4, (np.array([0, 2, 3]), np.array([3, 0, 1]))).tolist()
    assert calibration.STAT_NAMES == cc.STAT_NAMES and calibration.STATUS_NAMES == ("ok", "lower_bound", "upper_bound", "empty")
    assert calibration.CHUNK_BYTES == 64 << 20

    # finish checks its own arguments before it looks at the rows
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    for bad in (dict(calibration=-1), dict(calibration=65), dict(calibration=1.5), dict(calibration=True), dict(temperature=0.0),
                dict(temperature="fitted"), dict(calibration=15, temperature=-2.0)):
        with pytest.raises(ValueError):
            sel.finish(**bad)
    # a summary is host arithmetic on the one vector that was read
    host = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, -0.05, 3, 4, 0, 3, 0, 2.5, 0], dtype=torch.float64)
    s = calibration.Reliability.unpack(host, 2)
    assert [s[k] for k in calibration.STAT_NAMES] == [0.1, 0.2, 0.3, 0.4, 0.5, -0.05] and s["skipped"] == 3
    assert s["bins"][0] == {"lo": 0.0, "hi": 0.5, "n": 4, "accuracy": 0.75, "confidence": 0.625}
    assert s["bins"][1]["n"] == 0 and np.isnan(s["bins"][1]["accuracy"]) and np.isnan(s["bins"][1]["confidence"]) and s["bins"][1]["hi"] == 1.0


def test_the_default_call_is_unchanged(monkeypatch):
    """``calibration=0, temperature=None`` (the defaults) add no key and call nothing of the new module: ``finish`` on stubbed device
    functions, each of which is reached exactly as often as before."""
    sig = inspect.signature(selective.SelectiveEvaluator.finish)
    assert [sig.parameters[k].default for k in ("bootstrap", "seed", "confidence", "unit", "calibration", "temperature")] == [0, 0, 0.95, "cine", 0, None]
    from protoasnet_amd.trainer import DPTrainer

    sig = inspect.signature(DPTrainer.evaluate_selective)
    assert [sig.parameters[k].default for k in ("bootstrap", "seed", "confidence", "unit", "calibration", "temperature")] == [0, 0, 0.95, "cine", 0, None]
    assert inspect.signature(DPTrainer.fit_temperature).parameters["mode"].default == "val"
    cs = [1.0, 0.5]
    calls = []

    class RC:
        def packed(self, coverages):
            return torch.tensor([0.5, 1.0, 0.4, 0.9, 0.3, 0.8, 0.75, 0.25, 6, 3, 0.25, 0.7, 6, 1], dtype=torch.float64)

    class Ev:
        K_real, rows = 2, 6
        probs, labels, logits = torch.zeros(6, 2), torch.zeros(6, dtype=torch.int32), torch.zeros(6, 3)

    def counted(name, result):
        def f(*a, **k):
            calls.append(name)
            return result
        return f

    def not_reached(*a, **k):
        raise AssertionError("the defaults must not reach the calibration module")

    monkeypatch.setattr(selective, "uncertainty", counted("uncertainty", torch.zeros(6)))
    monkeypatch.setattr(selective, "risk_coverage", counted("risk_coverage", RC()))
    monkeypatch.setattr(_lib, "lib", counted("lib", None))  # any library call of finish itself would go through here
    for name in ("reliability", "scaled_probs", "fit_temperature"):
        monkeypatch.setattr(calibration, name, not_reached)
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    sel.ev, sel.keys, sel.abstain, sel.score, sel.ab_logitpath = Ev(), list("aabbcc"), True, "auto", "joined"
    res = sel.finish(cs, level="clip")
    assert calls == ["uncertainty", "risk_coverage"]  # the two device steps of the call as it was, once each, and no other library call
    assert "calibration" not in res and "ci" not in res and sorted(res) == sorted(
        ["aurc", "error_auroc", "rows", "nan_rows"] + [f"{n}@{c}" for n in ("accuracy", "bal_accuracy", "f1_mean", "threshold") for c in ("1", "0.5")])
    assert res == sel.finish(cs, level="clip", calibration=0, temperature=None)
    with pytest.raises(AssertionError, match="must not reach"):
        sel.finish(cs, level="clip", calibration=15)
    with pytest.raises(AssertionError, match="must not reach"):
        sel.finish(cs, level="clip", temperature=2.0)
