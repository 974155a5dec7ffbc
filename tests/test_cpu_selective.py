"""CPU: selective prediction -- the C-ABI surface and its argument checks, ``build_groups``, the coverage index arithmetic, and the numpy
restatements of tests/selective_cases.py (what the GPU tests hold the kernels to) against cases worked out by hand."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import selective_cases as sc
import protoasnet_amd
from protoasnet_amd import _lib, selective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_uncertainty_scores", "pasn_group_predictions", "pasn_risk_coverage_workspace_bytes", "pasn_risk_coverage")


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pasn_\w+)", nm))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
        assert getattr(lib, name) is not None
    assert "selective" in protoasnet_amd.__all__ and protoasnet_amd.selective is selective  # exported lazily, like its neighbours


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def scores(M=300, K=4, K_real=3, mode=0, logits=fake, u=fake):
        return lib.pasn_uncertainty_scores(logits, M, K, K_real, mode, u, 0)

    def groups(G=5, K_real=3, **null):
        a = dict(probs=fake, u=fake, labels=fake, offsets=fake, rows=fake, G=G, K_real=K_real, p_mean=fake, p_conf=fake, u_mean=fake,
                 g_label=fake, g_count=fake, status=fake)
        a.update(null)
        return lib.pasn_group_predictions(*a.values(), 0)

    def curve(M=100, K_real=3, ws=fake, **null):
        a = dict(probs=fake, labels=fake, u=fake, M=M, K_real=K_real, order=fake, acc=fake, bal_acc=fake, f1_mean=fake, threshold=fake,
                 aurc=fake, counts=fake, workspace=ws)
        a.update(null)
        return lib.pasn_risk_coverage(*a.values(), 0)

    for K_real in (1, 17):
        assert scores(K=K_real + 1, K_real=K_real) == 1
        assert groups(K_real=K_real) == 1
        assert curve(K_real=K_real) == 1
        assert lib.pasn_risk_coverage_workspace_bytes(100, K_real) == 0
    with pytest.raises(ValueError, match="K_real"):
        _lib.check(curve(K_real=17))
    for K in (3, 5):  # mode 1 reads the joined softmax: exactly one abstention column
        assert scores(K=K, K_real=3, mode=1) == 1
    with pytest.raises(ValueError, match=r"K == K_real \+ 1"):
        _lib.check(scores(K=5, K_real=3, mode=1))
    assert scores(K=3, K_real=3, mode=2) == 1 and scores(K=18, K_real=16) == 1 and scores(mode=3) == 1 and scores(mode=-1) == 1
    for M in (0, (1 << 20) + 1):
        assert curve(M=M) == 1
        assert lib.pasn_risk_coverage_workspace_bytes(M, 3) == 0
    assert scores(M=0) == 1 and groups(G=0) == 1
    assert curve(ws=0) == 1  # a NULL workspace
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(curve(ws=0))
    assert curve(ws=260) == 1  # misaligned
    assert scores(logits=0) == 1 and scores(u=0) == 1
    for k in ("probs", "u", "labels", "offsets", "rows", "p_mean", "p_conf", "u_mean", "g_label", "g_count", "status"):
        assert groups(**{k: 0}) == 1, k
    for k in ("probs", "labels", "u", "order", "acc", "bal_acc", "f1_mean", "threshold", "aurc", "counts"):
        assert curve(**{k: 0}) == 1, k
    # the workspace: rank and cell per row, three counters per class and a partial sum per scan block of 1024 positions
    assert lib.pasn_risk_coverage_workspace_bytes(2500, 3) == 2500 * 8 + 3 * (3 * 3 * 4 + 8)
    assert lib.pasn_risk_coverage_workspace_bytes(1 << 20, 16) == (1 << 20) * 8 + 1024 * (3 * 16 * 4 + 8)


def test_python_surface_checks_its_arguments():
    with pytest.raises(RuntimeError, match="GPU only"):
        selective.uncertainty(torch.zeros(4, 4), abstain_class=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        selective.risk_coverage(torch.rand(4, 3), torch.zeros(4, dtype=torch.int64), torch.rand(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        selective.group_predictions(torch.rand(4, 3), torch.rand(4), torch.zeros(4, dtype=torch.int64), selective.build_groups("aabb"))
    assert selective.score_mode(True) == 1 and selective.score_mode(False) == 0  # auto
    assert selective.score_mode(True, "maxprob") == 0 and selective.score_mode(True, "alpha", "separate") == 2
    for bad in (dict(score="entropy"), dict(ab_logitpath="split"), dict(abstain_class=False, score="alpha")):
        with pytest.raises(ValueError):
            selective.score_mode(**{"abstain_class": True, **bad})


def test_trainer_entry_refuses_cpu_and_non_xproto_models(tmp_path):
    from protoasnet_amd import model_builder
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG, Toy, _batches
    from util import CFG_PUSH_XIMG

    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    t = DPTrainer(Toy(), cfg, {"train": _batches(1, 2), "test": _batches(3, 2)}, log=lambda *_: None)
    with pytest.raises(NotImplementedError):
        t.evaluate_selective("test")
    t = DPTrainer(model_builder.build(CFG_PUSH_XIMG), cfg, {"train": [], "test": []}, log=lambda *_: None)
    with pytest.raises(RuntimeError, match="GPU only"):
        t.evaluate_selective("test")
    assert not os.listdir(tmp_path)


def test_build_groups_on_interleaved_keys():
    offsets, rows, names = selective.build_groups(["b", "a", "b", "c", "a", "b"])
    assert names == ["b", "a", "c"]  # order of first appearance
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 3, 5, 6]
    assert rows.dtype == np.int32 and rows.tolist() == [0, 2, 5, 1, 4, 3]  # ascending within a group, not contiguous
    offsets, rows, names = selective.build_groups([])
    assert offsets.tolist() == [0] and rows.size == 0 and names == []
    offsets, rows, names = selective.build_groups(["x"] * 4)
    assert offsets.tolist() == [0, 4] and rows.tolist() == [0, 1, 2, 3] and names == ["x"]


def test_coverage_index_arithmetic():
    rows = selective.coverage_rows
    assert rows([1.0, 0.9, 0.8, 0.7, 0.5], 10).tolist() == [10, 9, 8, 7, 5]  # 0.7 * 10 = 7.000000000000001 in fp64 still means 7 rows
    assert rows([1.0, 0.9, 0.5, 0.1], 7).tolist() == [7, 7, 4, 1]  # ceil: 6.3 -> 7, 3.5 -> 4, 0.7 -> 1
    assert rows([0.001], 10).tolist() == [1]  # lands below one row: one row is kept
    assert rows([1.0, 0.5], 1).tolist() == [1, 1]
    assert rows([1.0, 0.3], 1 << 20).tolist() == [1 << 20, 314573]
    for Mv in (1, 7, 10, 2500, 99999):  # the device form takes the same steps
        cs = [1.0, 0.9, 0.8, 0.7, 0.5, 0.123, 1e-6]
        assert rows(cs, torch.tensor(Mv)).tolist() == rows(cs, Mv).tolist()
    for bad in ((), (0.0,), (1.5,), (float("nan"),)):
        with pytest.raises(ValueError):
            selective._check_coverages(bad)
    # the packed vector of .at(): [acc, bal_acc, f1_mean, threshold, rows (per coverage), aurc, error_auroc, Mv, NaN rows]
    got = selective.RiskCoverage.unpack(torch.tensor([0.5, 1.0, 0.4, 0.9, 0.3, 0.8, 0.75, 0.25, 6, 3, 0.25, 0.7, 6, 1], dtype=torch.float64), [1.0, 0.5])
    assert got == {"coverage": [1.0, 0.5], "accuracy": [0.5, 1.0], "bal_accuracy": [0.4, 0.9], "f1_mean": [0.3, 0.8], "threshold": [0.75, 0.25],
                   "rows": [6, 3], "aurc": 0.25, "error_auroc": 0.7, "valid_rows": 6, "nan_rows": 1}
    empty = selective.RiskCoverage.unpack(torch.tensor([0.0, 0.0, 0.0, 0.0, 1, float("nan"), float("nan"), 0, 0], dtype=torch.float64), [1.0])
    assert empty["rows"] == [0] and np.isnan(empty["accuracy"][0]) and empty["valid_rows"] == 0


# ---- the restatement against hand cases --------------------------------------------------------------------------------------------------
HAND_LABELS = np.array([0, 1, 1, 0, 1, 0, -1])
HAND_PRED = [0, 1, 0, 0, 0, 1, 1]
HAND_U = np.array([0.3, 0.1, 0.2, 0.1, np.nan, 0.5, 0.0], dtype=np.float32)


def _hand_probs(K):
    p = np.full((7, K), 0.1, dtype=np.float32)
    p[np.arange(7), HAND_PRED] = 0.6
    return p


def test_six_row_curve_by_hand():
    """Order: u = 0.1 twice (rows 1 and 3, the lower index first), 0.2 (row 2), 0.3 (row 0), 0.5 (row 5), NaN last (row 4); row 6 is
    padding.  Right / wrong in that order: R R W R W W."""
    r = sc.risk_coverage_ref(_hand_probs(2), HAND_LABELS, HAND_U)
    assert r["order"].tolist() == [1, 3, 2, 0, 5, 4] and r["counts"].tolist() == [6, 1]
    assert r["acc"].tolist() == [1.0, 1.0, 2 / 3, 3 / 4, 3 / 5, 3 / 6]
    # balanced accuracy: m = 1 sees class 1 only (absent classes do not count); then (recall_0 + recall_1) / 2
    assert np.allclose(r["bal_acc"], [1.0, 1.0, (1 + 1 / 2) / 2, (1 + 1 / 2) / 2, (2 / 3 + 1 / 2) / 2, (2 / 3 + 1 / 3) / 2], rtol=1e-15, atol=0)
    # F1: m = 1 has nothing of class 0 among labels or predictions: 0 / 0 counts as 0, and the mean is still over both classes
    f1_6 = (2 * 2 / (3 + 4) + 2 * 1 / (3 + 2)) / 2
    assert np.allclose(r["f1_mean"], [0.5, 1.0, 2 / 3, (4 / 5 + 2 / 3) / 2, (2 * 2 / (3 + 3) + 2 * 1 / (2 + 2)) / 2, f1_6], rtol=1e-15, atol=0)
    assert r["threshold"][:5].tolist() == [np.float32(0.1), np.float32(0.1), np.float32(0.2), np.float32(0.3), 0.5] and np.isnan(r["threshold"][5])
    assert np.isclose(r["aurc"], (0 + 0 + 1 / 3 + 1 / 4 + 2 / 5 + 1 / 2) / 6, rtol=1e-15, atol=0)
    # u as a detector of the wrong rows: NaN poisons it; without the NaN row, wrong u = {0.2, 0.5}, right u = {0.1, 0.1, 0.3}: 5 of 6 pairs
    assert np.isnan(sc.error_auroc_ref(_hand_probs(2), HAND_LABELS, HAND_U))
    lab = HAND_LABELS.copy()
    lab[4] = -1
    assert sc.error_auroc_ref(_hand_probs(2), lab, HAND_U) == 5 / 6
    assert np.isnan(sc.error_auroc_ref(_hand_probs(2)[:2], HAND_LABELS[:2], HAND_U[:2]))  # every row right


def test_balanced_accuracy_with_an_absent_class_and_f1_with_a_zero_denominator():
    # three classes, class 2 never a label and never predicted: it leaves balanced accuracy alone and brings an F1 of 0
    r2, r3 = sc.risk_coverage_ref(_hand_probs(2), HAND_LABELS, HAND_U), sc.risk_coverage_ref(_hand_probs(3), HAND_LABELS, HAND_U)
    assert r3["order"].tolist() == r2["order"].tolist() and r3["acc"].tolist() == r2["acc"].tolist()
    assert r3["bal_acc"].tolist() == r2["bal_acc"].tolist()
    assert np.allclose(r3["f1_mean"], r2["f1_mean"] * 2 / 3, rtol=1e-15, atol=0)
    acc, bal, f1 = sc.confusion_metrics([[2, 1, 0], [0, 0, 0], [1, 0, 3]])
    assert acc == 5 / 7 and bal == (2 / 3 + 3 / 4) / 2 and np.isclose(f1, (4 / 6 + 0 + 6 / 7) / 3, rtol=1e-15, atol=0)
    assert sc.confusion_metrics([[0, 0], [0, 0]])[1:] == (0.0, 0.0)
    # ... and it is trainer.confusion_to_metrics
    from protoasnet_amd.trainer import confusion_to_metrics

    rng = np.random.default_rng(4)
    for K in (2, 3, 16):
        cm = rng.integers(0, 5, (K, K))
        cm[rng.integers(0, K)] = 0
        want = confusion_to_metrics(torch.from_numpy(cm))
        _, bal, f1 = sc.confusion_metrics(cm)
        assert np.isclose(bal, want["accuracy"], rtol=1e-14, atol=0) and np.isclose(f1, want["f1_mean"], rtol=1e-14, atol=0)


def test_order_rule():
    u = np.array([0.5, np.nan, -0.0, 0.0, 0.5, -1.0, np.inf, np.nan, 0.25], dtype=np.float32)
    lab = np.array([0, 0, 1, 1, -1, 0, 1, 1, 3])  # row 4 is padding, row 8's label lies outside the classes
    assert sc.order_ref(u, lab, 2).tolist() == [5, 2, 3, 0, 6, 1, 7]


def test_group_restatement_by_hand():
    probs = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [0.0, 1.0], [0.5, 0.5]], dtype=np.float32)
    u = np.array([0.5, 1.0, 0.0, 1.0, np.nan], dtype=np.float32)
    labels = np.array([1, 0, 1, 0, 1], dtype=np.int32)
    offsets, rows, names = selective.build_groups(["a", "b", "a", "b", "c"])
    r = sc.group_ref(probs, u, labels, offsets, rows)
    assert r["p_mean"].tolist() == [[0.375, 0.625], [0.5, 0.5], [0.5, 0.5]]
    # a: weights 0.5 and 1: (0.5 * [0.5, 0.5] + [0.25, 0.75]) / 1.5; b: the weights sum to 0, so the plain mean
    assert np.allclose(r["p_conf"][0], [0.5 / 1.5, 1.0 / 1.5], rtol=1e-15, atol=0) and r["p_conf"][1].tolist() == [0.5, 0.5]
    assert np.isnan(r["p_conf"][2]).all() and np.isnan(r["u_mean"][2])
    assert r["u_mean"][:2].tolist() == [0.25, 1.0] and r["label"].tolist() == [1, 0, 1] and r["count"].tolist() == [2, 2, 1]
    assert r["status"].tolist() == [0, 1]
    labels[3] = 1
    assert sc.group_ref(probs, u, labels, offsets, rows)["status"].tolist() == [1, 1]


def test_uncertainty_restatement_by_hand():
    z = np.array([[0.0, 0.0, 0.0, 0.0], [np.log(2.0), 0.0, 0.0, np.log(4.0)]])
    assert np.allclose(sc.uncertainty_ref(z, 3, 0), [2 / 3, 0.5], rtol=1e-15, atol=0)
    assert np.allclose(sc.uncertainty_ref(z, 3, 1), [0.25, 0.5], rtol=1e-15, atol=0)
    assert np.allclose(sc.uncertainty_ref(z, 3, 2), [0.5, 0.8], rtol=1e-15, atol=0)


def test_case_generators_are_seeded_and_full_of_ties():
    a, b = sc.curve_case(600, 3, 11), sc.curve_case(600, 3, 11)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    probs, labels, u = a
    assert len(np.unique(u)) == 8 and (labels == -1).sum() > 20 and probs.dtype == np.float32 and u.dtype == np.float32
    assert np.isnan(sc.curve_case(600, 3, 11, "nan")[2]).sum() == 2 and len(np.unique(sc.curve_case(600, 3, 11, "equal")[2])) == 1
    lg = sc.score_logits(300, 17, 5)
    assert lg.dtype == np.float32 and lg.min() >= -4 and lg.max() <= 4
    _, u, labels, keys = sc.group_case(2)
    offsets, rows, names = selective.build_groups(keys)
    sizes = np.diff(offsets)
    assert (sizes == 1).sum() == 50 and sizes.max() == 700 and len(names) == 92
    big = rows[offsets[names.index("big")]: offsets[names.index("big") + 1]]
    assert (np.diff(big) > 1).any() and (np.diff(big) > 0).all()  # not contiguous, ascending
    assert (u[rows[offsets[names.index("sure")]: offsets[names.index("sure") + 1]]] == 1.0).all()
