"""CPU: evaluation metrics -- the C-ABI surface and its argument checks, the numpy restatements (tests/metric_cases.py) against the G9
fixture made by running the reference's own code, the prediction CSV byte for byte, and the trainer's CPU path left as it was."""
import os
import re

import numpy as np
import pytest
import torch

import metric_cases as mc
from protoasnet_amd import _lib, metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_eval_batch_stats", "pasn_roc_auc_workspace_bytes", "pasn_roc_auc_ovr")


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def stats(**kw):
        a = dict(logits=fake, sim=fake, target=fake, N=4, K=4, K_real=3, P=40, P_cls=30, k_cls=5, k_abs=2, level=0.8, row_offset=0,
                 capacity=4, probs=fake, labels=fake, logits_out=0, sparsity=fake, div_counts=fake, sim_sums=fake)
        a.update(kw)
        return lib.pasn_eval_batch_stats(*a.values(), 0)

    assert stats(K_real=5) == 1  # K_real > K
    assert stats(P_cls=41) == 1  # P_cls > P
    assert stats(sim=0) == 1
    assert stats(logits=0) == 1
    assert stats(target=0) == 1
    assert stats(row_offset=2) == 1  # rows past the capacity
    assert stats(probs=0, labels=0, sparsity=0, div_counts=0, sim_sums=0) == 1
    assert stats(P=4097, P_cls=4000) == 3  # PASN_ERR_UNSUPPORTED: no slow path
    with pytest.raises(RuntimeError, match="4096"):
        _lib.check(stats(P=5000, P_cls=30))
    ws = lib.pasn_roc_auc_workspace_bytes(1000, 3)
    assert ws > 0 and lib.pasn_roc_auc_workspace_bytes(0, 3) == 0
    assert lib.pasn_roc_auc_ovr(fake, fake, 1000, 1, fake, fake, fake, 0) == 1  # K_real < 2
    assert lib.pasn_roc_auc_ovr(fake, fake, 1000, 17, fake, fake, fake, 0) == 1
    assert lib.pasn_roc_auc_ovr(fake, fake, (1 << 24) + 1, 3, fake, fake, fake, 0) == 1
    assert lib.pasn_roc_auc_ovr(fake, fake, 0, 3, fake, fake, fake, 0) == 1
    assert lib.pasn_roc_auc_ovr(fake, 0, 10, 3, fake, fake, fake, 0) == 1
    assert lib.pasn_roc_auc_ovr(fake, fake, 10, 3, fake, fake, 0, 0) == 1


def test_python_surface_refuses_cpu_tensors():
    m = metrics.SparsityMetric(level=0.8, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.rand(2, 40))
    with pytest.raises(RuntimeError, match="GPU only"):
        metrics.roc_auc_ovr_weighted(torch.rand(4, 3), torch.zeros(4, dtype=torch.int64), 3)


def test_sparsity_restatement_reproduces_the_reference(golden):
    g = golden("g9_metrics.npz")
    for case, batches in mc.sparsity_batches().items():
        tot, cnt = 0, 0
        for b, ref in zip(batches, g[f"sparsity_{case}_batch"]):
            res, _ = mc.sparsity_rows(b.numpy())
            assert np.float32(res.sum() / res.size) == ref, case
            tot, cnt = tot + int(res.sum()), cnt + res.size
        assert [tot, cnt] == g[f"sparsity_{case}_sum"].tolist()
        assert np.float32(tot) / np.float32(cnt) == g[f"sparsity_{case}_epoch"]


def test_sparsity_rules_by_hand():
    res, _ = mc.sparsity_rows(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0.5, 0.5, 0, 0], [0.1, 0.1, 0.1, 0.7], [0.2, 0.2, 0.3, 0.3]],
                                       dtype=np.float32))
    # all-zero: 0 (no prefix); one-hot: index 0; 0.5 + 0.5 at index 1; 0.7 + 0.1 >= 0.8 at index 1; 0.3 + 0.3 + 0.2 at index 2
    assert res.tolist() == [0, 0, 1, 1, 2]


def test_diversity_restatement_by_hand():
    sim = np.array([[0.9, 0.1, 0.5, 0.5, 0.2, 0.3, 0.8], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.6]], dtype=np.float32)
    # classes [0, 5) top 2, abstention [5, 7) top 1; ties to the lower index
    assert mc.diversity_counts(sim, 5, k_cls=2, k_abs=1).tolist() == [1, 0, 1, 1, 1, 1, 1]


def test_auc_restatement_reproduces_sklearn(golden):
    g = golden("g9_metrics.npz")
    cases = mc.auc_cases()
    if not any(k.startswith("auc_") for k in g.files):
        pytest.skip("the fixture was made without sklearn")  # (the generator reports it; the hand cases below still run)
    for case, (p, y) in cases.items():
        a, _ = mc.auc_ovr_weighted(p, y, 3)
        assert abs(a - float(g[f"auc_{case}"])) <= 1e-12, case


def test_auc_hand_cases():
    y = np.array([0, 0, 1, 1, 2, 2])
    perfect = np.eye(3, dtype=np.float32)[y]
    assert mc.auc_ovr_weighted(perfect, y, 3)[0] == 1.0
    assert mc.auc_ovr_weighted(1 - perfect, y, 3)[0] == 0.0  # reversed
    assert mc.auc_ovr_weighted(np.full((6, 3), 1 / 3, np.float32), y, 3)[0] == 0.5  # all tied
    a, per = mc.auc_ovr_weighted(perfect[:4], y[:4], 3)  # class 2 missing
    assert a == 0.0 and np.isnan(per[2]) and per[0] == 1.0
    bad = perfect.copy()
    bad[1, 2] = np.nan
    assert mc.auc_ovr_weighted(bad, y, 3)[0] == 0.0
    padded = np.concatenate([perfect, np.zeros((2, 3), np.float32)])
    assert mc.auc_ovr_weighted(padded, np.concatenate([y, [-1, -1]]), 3)[0] == 1.0
    # binary: the weighted mean of the two one-vs-rest AUCs of complementary scores is the binary AUC
    s = np.array([0.1, 0.4, 0.35, 0.8], np.float32)
    yb = np.array([0, 0, 1, 1])
    assert mc.auc_ovr_weighted(np.stack([1 - s, s], 1), yb, 2)[0] == 0.75


def _rows(optional):
    b, logits = mc.pred_log_batch(optional)
    return metrics.prediction_rows([metrics.batch_log_meta(b)], logits.numpy(), mc.LOGIT_NAMES[:3] + ["abstain"])


def test_prediction_log_reproduces_the_reference_csv(tmp_path):
    path = tmp_path / "e00_f1_50%.csv"
    metrics.write_prediction_log(str(path), _rows(optional=True))
    with open(os.path.join(REPO, "tests", "golden", "g9_pred_log.csv"), "rb") as f:
        assert path.read_bytes() == f.read()


def test_prediction_log_without_optional_keys(tmp_path):
    path = tmp_path / "log.csv"
    metrics.write_prediction_log(str(path), _rows(optional=False))
    lines = path.read_text().splitlines()
    assert lines[0] == ",filename,target_AS,logit_No AS,logit_Early AS,logit_Significant AS,logit_abstain"
    assert lines[1] == "0,a.mat,0,0.1,-1.5,2.25,1e-08"
    assert lines[2] == '1,"b, c.mat",2,123456.79,-0.0,3.0,'
    assert len(lines) == 4


def test_logit_names():
    assert metrics.logit_names(3, True) == ["No AS", "Early AS", "Significant AS", "abstain"]
    assert metrics.logit_names(3, False, ["a", "b", "c"]) == ["a", "b", "c"]
    with pytest.raises(ValueError):
        metrics.logit_names(3, False, ["a", "b"])


def test_real_prototype_count():
    from test_cpu_trainer import Toy

    m = Toy(P=8, K=4)  # 2 prototypes per class; with an abstain class the last 2 are abstention prototypes
    assert metrics.real_prototype_count(m, 3) == 6 and metrics.real_prototype_count(m, 4) == 8
    m.prototype_class_identity = m.prototype_class_identity.flip(0)
    with pytest.raises(ValueError, match="precede"):
        metrics.real_prototype_count(m, 3)


def test_cpu_trainer_epoch_dict_is_unchanged(tmp_path):
    """A CPU model gets the confusion-matrix dict of before and no CSV, in every mode."""
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG, Toy, _batches

    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    t = DPTrainer(Toy(), cfg, {"train": _batches(1, 2), "val": _batches(2, 2), "test": _batches(3, 2)}, log=lambda *_: None)
    for mode in ("val", "val_push", "test"):
        m = t.evaluate(mode)
        assert sorted(m) == ["accuracy", "f1", "f1_mean", "loss", "loss_terms"]
    assert not os.path.exists(tmp_path / "csv_test") and not os.path.exists(tmp_path / "csv_val_push")
    with pytest.raises(ValueError):
        t.evaluate("train")
