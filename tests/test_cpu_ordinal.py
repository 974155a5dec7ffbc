"""CPU: the ordinal evaluation's restatement (tests/ordinal_cases.py) by hand and against scikit-learn, the surface of
protoasnet_amd.ordinal (symbols, argument checks, host readings) and the unchanged default of SelectiveEvaluator.finish."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bootstrap_cases as bc
import ordinal_cases as oc
import protoasnet_amd
from protoasnet_amd import _lib, ordinal, selective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_ordinal_agreement", "pasn_ordinal_confusion", "pasn_ordinal_cut_scores", "pasn_ordinal_workspace_bytes",
               "pasn_ordinal_screen")


def _pack(ref):
    """A restatement result as the fp64 vector ``Screening.packed()`` reads back."""
    return np.concatenate([np.asarray(ref[k], dtype=np.float64).ravel() for k in ("pn", "u2", "stats", "op_theta", "op_tally", "fix_tally")])


def test_eight_rows_three_grades_by_hand():
    """Probabilities in eighths (every sum exact), labels 0 0 1 0 1 2 2 0:

        row   p * 8     label  pred   s_1 * 8 = (p1 + p2) * 8
        0     6 1 1     0      0      2
        1     4 3 1     0      0      4
        2     4 2 2     1      0      4      under by one grade
        3     4 1 3     0      0      4
        4     2 5 1     1      1      6
        5     2 2 4     2      2      6
        6     1 5 2     2      1      7      under by one grade
        7     1 2 5     0      2      7      over by two grades

    Agreement.  cm = [[3 0 1] [1 1 0] [0 1 1]], n = 8, r = c = (4, 2, 2).  mae = (2 + 1 + 1) / 8 = 1/2; within_one = 7/8; under = 2/8;
    over = 1/8.  Linear: A = 2 + 1 + 1 = 4, E = 8 + 16 + 8 + 4 + 16 + 4 = 56, kappa = 1 - 8 * 4 / 56 = 3/7.  Quadratic: A = 4 + 1 + 1 = 6,
    E = 8 + 32 + 8 + 4 + 32 + 4 = 88, kappa = 1 - 48 / 88 = 5/11.

    Cut 1 (grade >= 1): positives are rows 2 4 5 6, P = N = 4.  Tie groups, ascending: 2/8 (tp 0, fp 1), 4/8 (1, 2), 6/8 (2, 0),
    7/8 (1, 1); at scores >= v: (TP, FP) = (4, 4), (4, 3), (3, 1), (1, 1), and (0, 0) at +inf.
    U2 = sum over positives of 2 [negatives below] + [negatives tied] = (2 + 2) + 6 + 6 + (6 + 1) = 23, auc = 23 / 32.
    ap = (1/4)(1/2) + (2/4)(3/4) + (1/4)(4/7) = 1/2 + 1/7; the group at 2/8 holds no positive and adds nothing.
    Specificity 0.5: (4 - FP) / 4 >= 0.5 needs FP <= 2: the smallest such candidate is 6/8 -> (3, 1).  Specificity 0.9 needs FP = 0: only
    +inf -> (0, 0).  Sensitivity 0.75: TP >= 3, the largest such candidate is 6/8.  Sensitivity 0.8: TP = 4, met at 2/8 and 4/8 (a tie
    in TP): the larger, 4/8 -> (4, 3).  Youden: J = 4 (TP - FP) = 0, 4, 8, 0, 0 -> 6/8.
    Fixed 0.5 -> s >= 4/8: (4, 3); fixed 0.625 lies between two groups: (3, 1).
    Net benefit at pt = 0.5 (threshold 0.5 on the score): 4/8 - (3/8) * 1 = 1/8; treat all: 4/8 - 4/8 = 0."""
    p = np.array([[6, 1, 1], [4, 3, 1], [4, 2, 2], [4, 1, 3], [2, 5, 1], [2, 2, 4], [1, 5, 2], [1, 2, 5]], dtype=np.float32) / 8
    y = np.array([0, 0, 1, 0, 1, 2, 2, 0], dtype=np.int32)
    cm = oc.confusion_ref(p, y)
    assert cm.tolist() == [[3, 0, 1], [1, 1, 0], [0, 1, 1]]
    assert oc.agreement_ref(cm).tolist() == [0.5, 7 / 8, 2 / 8, 1 / 8, 1.0 - (8.0 * 4.0) / 56.0, 1.0 - (8.0 * 6.0) / 88.0]
    assert abs(oc.agreement_ref(cm)[4] - 3 / 7) < 1e-15 and abs(oc.agreement_ref(cm)[5] - 5 / 11) < 1e-15
    assert np.isnan(oc.agreement_ref(np.zeros((3, 3)))).all()
    one = np.zeros((3, 3), dtype=np.int64)
    one[1, 1] = 5
    assert oc.agreement_ref(one)[:4].tolist() == [0.0, 1.0, 0.0, 0.0] and np.isnan(oc.agreement_ref(one)[4:]).all()  # E = 0
    s = oc.cut_scores_ref(p)
    assert (s[0] * 8).tolist() == [2, 4, 4, 4, 6, 6, 7, 7] and (s[1] * 8).tolist() == [1, 1, 2, 3, 1, 4, 2, 5]
    r = oc.cut_ref(s[0], y >= 1, np.ones(8), (0.5, 0.9), (0.75, 0.8), (0.5, 0.625))
    assert (r["P"], r["N"], r["u2"], r["auc"]) == (4, 4, 23, 23 / 32)
    assert abs(r["ap"] - (0.5 + 1 / 7)) < 1e-15
    assert r["theta"].tolist() == [0.75, np.inf, 0.75, 0.5, 0.75]
    assert r["tally"].tolist() == [[3, 1], [0, 0], [3, 1], [4, 3], [3, 1]] and r["fix"].tolist() == [[4, 3], [3, 1]]
    # a replicate is the sample with weights: row 7 twice, row 0 never -> N stays 4, the group at 2/8 is no candidate any more
    w = np.array([0, 1, 1, 1, 1, 1, 1, 2])
    rw = oc.cut_ref(s[0], y >= 1, w, (0.5,), (0.8,))
    pe, ye = oc.expand(p, y, w)
    re_ = oc.cut_ref(oc.cut_scores_ref(pe)[0], ye >= 1, np.ones(len(ye)), (0.5,), (0.8,))
    assert (rw["u2"], rw["ap"], rw["theta"].tolist(), rw["tally"].tolist()) == (re_["u2"], re_["ap"], re_["theta"].tolist(), re_["tally"].tolist())
    assert (rw["P"], rw["N"], rw["u2"]) == (4, 4, 2 + 4 + 4 + 6) and rw["theta"].tolist() == [0.75, 0.5, 0.75]
    # the host readings of the packed vector: ratios and net benefit of the tallies
    ref = oc.screen_ref(p, y, (0.5, 0.9), (0.75, 0.8), fixed=np.array([[0.75, 0.5, 0.75, 0.5], [0.5, 0.5, 0.5, 0.5]], dtype=np.float32))
    fit = ordinal.OperatingFit(torch.tensor([[0.75, 0.5, 0.75], [0.5, 0.5, 0.5]]), (0.5,), (0.8,))
    res = ordinal.Screening.unpack(_pack(ref), 3, 0, (0.5, 0.9), (0.75, 0.8), fit, (0.5,))
    c1 = res["cuts"][0]
    assert (c1["cut"], c1["P"], c1["N"], c1["prevalence"], c1["auc"], c1["u2"]) == (1, 4, 4, 0.5, 23 / 32, 23) and "ci" not in res
    assert c1["operating_points"][0] == {"kind": "specificity", "target": 0.5, "theta": 0.75, "tp": 3, "fp": 1, "sensitivity": 0.75,
                                         "specificity": 0.75, "ppv": 0.75, "npv": 0.75}
    inf = c1["operating_points"][1]
    assert inf["theta"] == np.inf and (inf["tp"], inf["fp"], inf["sensitivity"], inf["specificity"], inf["npv"]) == (0, 0, 0.0, 1.0, 0.5)
    assert np.isnan(inf["ppv"])
    assert [f["kind"] for f in c1["fitted"]] == ["specificity", "sensitivity", "youden"] and c1["fitted"][1]["tp"] == 4 and "theta" not in c1["fitted"][0]
    assert c1["net_benefit"] == [{"pt": 0.5, "net_benefit": 1 / 8, "treat_all": 0.0}]


def test_the_restatement_against_scikit_learn():
    """777 rows, K = 4, probabilities in sixteenths (many ties): once on the sample, once on a replicate expanded with np.repeat.  kappa
    and AUC within 1e-12, ap within M 2^-50, the operating-point tallies equal as integers."""
    pytest.importorskip("sklearn")
    from sklearn.metrics import average_precision_score, cohen_kappa_score, roc_auc_score, roc_curve

    M, K = 777, 4
    probs, labels = oc.ordinal_case(M, K, seed=5, pad=0.1)
    counts = bc.counts_ref(M, 1, seed=9)[0]
    spec, sens = (0.5, 0.8, 0.9, 0.95), (0.5, 0.8, 0.9, 0.99)
    for w in (oc.weights_ref(np.ones(M), labels, K), oc.weights_ref(counts, labels, K)):
        pe, ye = oc.expand(probs, labels, w)
        assert len(ye) > 600 and ((ye >= 0) & (ye < K)).all()
        got = oc.agreement_ref(oc.confusion_ref(probs, labels, w))
        pred = pe.argmax(1)
        assert abs(got[0] - np.abs(pred - ye).mean()) < 1e-12 and abs(got[2] - (pred < ye).mean()) < 1e-12
        for j, kind in ((4, "linear"), (5, "quadratic")):
            assert abs(got[j] - cohen_kappa_score(ye, pred, weights=kind, labels=list(range(K)))) < 1e-12, kind
        s = oc.cut_scores_ref(probs)
        se = oc.cut_scores_ref(pe)
        for c in range(K - 1):
            r = oc.cut_ref(s[c], labels >= c + 1, w, spec, sens)
            yb = (ye >= c + 1).astype(int)
            assert abs(r["auc"] - roc_auc_score(yb, se[c])) < 1e-12
            err = abs(r["ap"] - average_precision_score(yb, se[c]))
            print(f"cut {c + 1}: |ap - sklearn| = {err:.3g}")
            assert err <= len(ye) * 2.0 ** -50
            fpr, tpr, thr = roc_curve(yb, se[c], drop_intermediate=False)  # descending thresholds, the first one +inf
            tp, fp = np.rint(tpr * r["P"]).astype(np.int64), np.rint(fpr * r["N"]).astype(np.int64)
            for t, tau in enumerate(spec):  # the smallest threshold that reaches the specificity: the LAST such point of the curve
                i = np.flatnonzero((r["N"] - fp) / r["N"] >= tau)[-1]
                assert r["tally"][t].tolist() == [tp[i], fp[i]] and r["theta"][t] == np.float32(thr[i]), (c, tau)
            for t, tau in enumerate(sens):  # the largest threshold that reaches the sensitivity: the FIRST such point
                i = np.flatnonzero(tp / r["P"] >= tau)[0]
                assert r["tally"][len(spec) + t].tolist() == [tp[i], fp[i]] and r["theta"][len(spec) + t] == np.float32(thr[i]), (c, tau)
            J = tp * r["N"] - fp * r["P"]
            i = np.flatnonzero(J == J.max())[0]  # ties to the larger threshold
            assert r["tally"][-1].tolist() == [tp[i], fp[i]]


def test_the_replicate_draws_are_the_bootstraps_own():
    """A replicate's weights are the multiplicities of ``bootstrap_cases.replicate_rows`` for the same (seed, b, G), groups included."""
    M, K = 300, 3
    _, labels = oc.ordinal_case(M, K, seed=2, pad=0.2)
    groups = selective.build_groups(bc.random_groups(M, seed=3))[:2]
    G = len(groups[0]) - 1
    for b, counts in enumerate(bc.counts_ref(G, 3, seed=11)):
        w = oc.weights_ref(counts, labels, K, groups)
        assert np.array_equal(w, np.bincount(bc.replicate_rows(counts, labels, K, groups), minlength=M)), b
    ref = oc.screen_ref(*oc.ordinal_case(M, K, seed=2, pad=0.2), groups=groups, B=2, seed=11)
    fed = oc.screen_ref(*oc.ordinal_case(M, K, seed=2, pad=0.2), groups=groups, B=2, seed=11, counts=bc.counts_ref(G, 2, seed=11))
    assert all(np.array_equal(ref[k], fed[k], equal_nan=True) for k in ("pn", "u2", "op_tally")) and ref["pn"].shape == (3, 2, 2)


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
    assert "ordinal" in protoasnet_amd.__all__ and protoasnet_amd.ordinal is ordinal  # exported lazily, like its neighbours
    assert int(re.search(r"#define PASN_ORDINAL_MAX_TARGETS (\d+)", header).group(1)) == ordinal.MAX_TARGETS == 8
    assert int(re.search(r"#define PASN_ORDINAL_MAX_FIXED (\d+)", header).group(1)) == ordinal.MAX_FIXED == 32
    assert ordinal.AGREEMENT_NAMES == oc.AGREEMENT_NAMES
    with open(os.path.join(REPO, "protoasnet_amd", "build.py")) as f:
        assert '"ordinal.hip"' in f.read()
    with open(os.path.join(REPO, "protoasnet_amd", "csrc", "ordinal.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "asm" not in src  # plain C++: no inline assembly in this file


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first
    half = (ctypes.c_double * 8)(*([0.5] * 8))

    def screen(M=100, G=100, K_real=3, B=2, spec=half, n_spec=1, sens=half, n_sens=1, n_fixed=0, groups=(0, 0), **null):
        p = dict(probs=fake, labels=fake, fixed=0, pn=fake, u2=fake, stats=fake, op_theta=fake, op_tally=fake, fix_tally=0, workspace=fake)
        p.update(null)
        return lib.pasn_ordinal_screen(p["probs"], p["labels"], groups[0], groups[1], M, G, K_real, B, 7, spec, n_spec, sens, n_sens, p["fixed"],
                                       n_fixed, p["pn"], p["u2"], p["stats"], p["op_theta"], p["op_tally"], p["fix_tally"], p["workspace"], 0)

    size = lib.pasn_ordinal_workspace_bytes
    assert size(100, 100, 3, 0) > 0 and size(100, 100, 3, 0) == size(100, 100, 3, 1000)  # counts in LDS: B costs nothing
    bound = lib.pasn_bootstrap_lds_max_groups()
    assert size(bound + 1, bound + 1, 3, 5) - size(bound + 1, bound + 1, 3, 0) == 5 * (bound + 1) * 4  # a slice per further block
    for bad in (dict(K_real=1), dict(K_real=17), dict(M=0), dict(M=(1 << 20) + 1), dict(G=0), dict(G=101), dict(B=-1), dict(B=65537),
                dict(G=50), dict(n_spec=-1), dict(n_spec=9), dict(n_sens=9), dict(n_fixed=33), dict(n_fixed=1), dict(spec=None),
                dict(groups=(fake, 0)), dict(workspace=264)):
        assert screen(**bad) == 1, bad
    for k in ("probs", "labels", "pn", "u2", "stats", "op_theta", "op_tally", "workspace"):
        assert screen(**{k: 0}) == 1, k
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert screen(spec=(ctypes.c_double * 8)(0.5, bad), n_spec=2) == 1 and screen(sens=(ctypes.c_double * 8)(bad), n_sens=1) == 1, bad
    with pytest.raises(ValueError, match="specificity"):
        _lib.check(screen(spec=(ctypes.c_double * 8)(1.0)))
    with pytest.raises(ValueError, match="misaligned"):
        _lib.check(screen(workspace=264))
    assert size(100, 100, 1, 0) == 0 and size(100, 100, 17, 0) == 0 and size(0, 0, 3, 0) == 0 and size(100, 101, 3, 0) == 0
    assert size(100, 100, 3, -1) == 0 and size(100, 100, 3, 65537) == 0
    for bad in (dict(K=1), dict(K=17), dict(R=0), dict(R=65538), dict(cm=0), dict(out=0)):
        p = dict(cm=fake, R=3, K=3, out=fake)
        p.update(bad)
        assert lib.pasn_ordinal_agreement(p["cm"], p["R"], p["K"], p["out"], 0) == 1, bad
    for M, K in ((0, 3), ((1 << 20) + 1, 3), (10, 1), (10, 17)):
        assert lib.pasn_ordinal_confusion(fake, fake, M, K, fake, 0) == 1 and lib.pasn_ordinal_cut_scores(fake, M, K, fake, 0) == 1
    assert lib.pasn_ordinal_confusion(fake, fake, 10, 3, 0, 0) == 1 and lib.pasn_ordinal_cut_scores(0, 10, 3, fake, 0) == 1


def test_python_surface_checks_its_arguments():
    probs, labels = torch.rand(4, 3), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: ordinal.agreement(probs, labels), lambda: ordinal.agreement_of(torch.zeros(3, 3, dtype=torch.int64)),
                 lambda: ordinal.cut_scores(probs), lambda: ordinal.screen(probs, labels), lambda: ordinal.fit_operating_points(probs, labels)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for name in ("specificities", "sensitivities", "net_benefit_at"):
        for bad in ((0.0,), (1.0,), (0.5, 1.5), (float("nan"),), [0.5] * (33 if name == "net_benefit_at" else 9), 0.5, None):
            with pytest.raises(ValueError, match=name):
                ordinal._check_screen_args(**{**dict(specificities=(0.9,), sensitivities=(0.9,), B=0, seed=0, fit=None, net_benefit_at=()),
                                              name: bad})
    for bad in (dict(B=-1), dict(B=65537), dict(B=1.5), dict(B=True), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)):
        with pytest.raises(ValueError, match="B must|seed must"):
            ordinal._check_screen_args(**{**dict(specificities=(), sensitivities=(), B=0, seed=0, fit=None, net_benefit_at=()), **bad})
    with pytest.raises(ValueError, match="OperatingFit"):
        ordinal._check_screen_args((0.9,), (0.9,), 0, 0, {"thresholds": 1.0}, ())
    fit = ordinal.OperatingFit(torch.full((2, 4), 0.5), (0.8, 0.9), (0.9,))
    assert fit.K == 3 and fit.kind == ["specificity", "specificity", "sensitivity", "youden"] and fit.targets == [0.8, 0.9, 0.9, None]
    assert fit.read() == {"K": 3, "kinds": fit.kinds, "targets": fit.targets, "thresholds": [[0.5] * 4] * 2}
    with pytest.raises(ValueError, match="made on 3 classes"):
        ordinal._check_screen_args((0.9,), (0.9,), 0, 0, fit, (), K=4)
    full = ordinal.OperatingFit(torch.zeros(2, 17), [0.1 * j for j in range(1, 9)], [0.1 * j for j in range(1, 9)])
    assert len(ordinal._check_screen_args((), (), 0, 0, full, [0.5] * 15, K=3)[2]) == 15  # 17 + 15 = PASN_ORDINAL_MAX_FIXED
    with pytest.raises(ValueError, match="fixed thresholds"):
        ordinal._check_screen_args((), (), 0, 0, full, [0.5] * 16, K=3)
    for bad in (torch.zeros(2, 3), torch.zeros(4), torch.zeros(16, 4)):
        with pytest.raises(ValueError, match="thresholds"):
            ordinal.OperatingFit(bad, (0.8, 0.9), (0.9,))
    # shapes and sizes are checked on the host, after the device check
    assert ordinal._check_rows(probs, labels, "screen") == (4, 3)
    for p, l in ((torch.rand(4), None), (probs, labels[:3]), (torch.rand(4, 1), None), (torch.rand(4, 17), None), (torch.rand(0, 3), None)):
        with pytest.raises(ValueError):
            ordinal._check_rows(p, l, "screen")
    assert ordinal.cut_names(3, ["No AS", "Early AS", "Significant AS"]) == [">= Early AS", ">= Significant AS"] and ordinal.cut_names(3) == [">= 1", ">= 2"]
    with pytest.raises(ValueError, match="class_labels"):
        ordinal.cut_names(4, ["a", "b"])
    with pytest.raises(ValueError, match="packed"):
        ordinal.Screening.split(np.zeros(5), 3, 0, 3, 0)
    with pytest.raises(ValueError, match="intervals"):
        ordinal.intervals({"stats": 1})
    # finish and the trainer check their own arguments before they look at the rows
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    for bad in (dict(ordinal="fitted"), dict(ordinal=0.9), dict(ordinal=False), dict(ordinal=True, ordinal_net_benefit_at=(1.0,))):
        with pytest.raises(ValueError, match="ordinal|net_benefit_at"):
            sel.finish(**bad)
    from protoasnet_amd.trainer import DPTrainer

    t = DPTrainer.__new__(DPTrainer)
    t.operating_fit = t.conformal_fit = t.temperature_fit = None
    with pytest.raises(ValueError, match="fit_operating_points"):
        t.evaluate_selective("test", ordinal="fitted")
    with pytest.raises(ValueError, match="ordinal"):
        t.evaluate_selective("test", ordinal="fit")
    for bad in (dict(level="study"), dict(specificities=(1.0,)), dict(sensitivities=0.9), dict(temperature="fitted"), dict(temperature="x")):
        with pytest.raises(ValueError):
            t.fit_operating_points("val", **bad)


def test_the_default_call_is_unchanged(monkeypatch):
    """``ordinal=None`` (the default) adds no key and reaches nothing of the new module: ``finish`` on stubbed device functions, each of
    which is reached exactly as often as before; the trainer passes the keyword on only when it is given."""
    sig = inspect.signature(selective.SelectiveEvaluator.finish)
    assert [sig.parameters[k].default for k in ("ordinal", "ordinal_net_benefit_at")] == [None, ()]
    from protoasnet_amd.trainer import DPTrainer

    sig = inspect.signature(DPTrainer.evaluate_selective)
    assert [sig.parameters[k].default for k in ("ordinal", "ordinal_net_benefit_at")] == [None, ()]
    sig = inspect.signature(DPTrainer.fit_operating_points)
    assert [sig.parameters[k].default for k in ("mode", "level", "specificities", "sensitivities", "temperature")] == ["val", "cine", (0.9,), (0.9,), None]
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
        raise AssertionError("the defaults must not reach the ordinal module")

    monkeypatch.setattr(selective, "uncertainty", counted("uncertainty", torch.zeros(6)))
    monkeypatch.setattr(selective, "risk_coverage", counted("risk_coverage", RC()))
    monkeypatch.setattr(_lib, "lib", counted("lib", None))  # any library call of finish itself would go through here
    for name in ("agreement", "agreement_of", "screen", "cut_scores", "fit_operating_points"):
        monkeypatch.setattr(ordinal, name, not_reached)
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    sel.ev, sel.keys, sel.abstain, sel.score, sel.ab_logitpath = Ev(), list("aabbcc"), True, "auto", "joined"
    res = sel.finish(cs, level="clip")
    assert calls == ["uncertainty", "risk_coverage"]  # the two device steps of the call as it was, once each, and no other library call
    assert "ordinal" not in res and sorted(res) == sorted(
        ["aurc", "error_auroc", "rows", "nan_rows"] + [f"{n}@{c}" for n in ("accuracy", "bal_accuracy", "f1_mean", "threshold") for c in ("1", "0.5")])
    assert res == sel.finish(cs, level="clip", ordinal=None, ordinal_net_benefit_at=())
    with pytest.raises(AssertionError, match="must not reach"):
        sel.finish(cs, level="clip", ordinal=True)
    with pytest.raises(ValueError, match="fitted on 3 classes"):
        sel.finish(cs, level="clip", ordinal=ordinal.OperatingFit(torch.zeros(2, 3), (0.9,), (0.9,)))
    # the trainer hands finish exactly the keywords it handed it before
    seen = []

    class Sweep:
        def finish(self, *a, **k):
            seen.append(sorted(k))
            return {"aurc": 0.0, "error_auroc": 0.0}

    t = DPTrainer.__new__(DPTrainer)
    t.operating_fit = t.conformal_fit = t.temperature_fit = None
    t.config, t.current_epoch, t.log = {}, 0, lambda *a, **k: None
    t._selective_sweep = lambda mode, score="auto": Sweep()
    t.evaluate_selective("test", level="clip")
    assert seen == [["bootstrap", "calibration", "confidence", "seed", "temperature", "unit"]]
