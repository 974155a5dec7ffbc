"""GPU: selective prediction (csrc/selective.hip through protoasnet_amd.selective) against the float64 numpy restatements of
tests/selective_cases.py; SelectiveEvaluator on a bare head and DPTrainer.evaluate_selective on the HIP Video ProtoASNet."""
import csv
import os

import numpy as np
import pytest
import torch

import selective_cases as sc
from protoasnet_amd import metrics, selective, synth
from test_cpu_trainer import TRAIN_CFG
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _log(name, err, gate):
    """The largest observed error next to its gate (profiles/selective_parity_observed.tsv); never changes the verdict."""
    if os.environ.get("PASN_PARITY_LOG"):
        with open(os.environ["PASN_PARITY_LOG"], "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{name}\tmax_err={err:.3g}\tgate={gate:.3g}\n")


# ---- scores ------------------------------------------------------------------------------------------------------------------------------
# Gate of modes 1 and 2 against float64: the argument of expf lies in [-8, 0], so its rounding adds <= 2^-22 absolute = 2.4e-7 relative
# after exp; expf itself <= 2 ulp; the sum of <= 17 positive terms <= 16 * 2^-24; the division 2^-24.  On numerator and denominator
# together <= 2e-6 (the results are <= 1, so relative bounds absolute); the gate is twice that.
SCORE_GATE = 4e-6


@pytest.mark.parametrize("K,K_real", [(4, 3), (17, 16)])
def test_uncertainty_scores(K, K_real):
    M = 300  # crosses one 256-thread block
    lg = sc.score_logits(M, K, seed=K)
    (d_lg,) = _dev(lg)
    probs = torch.empty(M, K_real, dtype=torch.float32, device=DEV)
    metrics._batch_stats(d_lg, None, None, K_real, 0, 0.8, 0, M, probs=probs)
    u0 = selective.uncertainty(d_lg, abstain_class=True, score="maxprob")
    assert u0.dtype == torch.float32 and u0.shape == (M,)
    assert torch.equal(u0, 1 - probs.max(1).values)  # bitwise: the same expf / division sequence as the stored probabilities
    assert torch.equal(selective.uncertainty(d_lg[:, :K_real].contiguous(), abstain_class=False), u0)  # auto without an abstention class
    assert float(np.abs(u0.cpu().numpy() - sc.uncertainty_ref(lg, K_real, 0)).max()) <= SCORE_GATE
    for mode, kw in ((1, dict(score="auto")), (2, dict(score="alpha", ab_logitpath="separate"))):
        u = selective.uncertainty(d_lg, abstain_class=True, **kw)
        err = float(np.abs(u.cpu().numpy().astype(np.float64) - sc.uncertainty_ref(lg, K_real, mode)).max())
        _log(f"uncertainty mode {mode} K={K}", err, SCORE_GATE)
        assert err <= SCORE_GATE, (mode, err)
    # sigmoid at the ends of the fp32 range: no overflow, no NaN
    ends = torch.tensor([[0.0, 0.0, 0.0, 200.0], [0.0, 0.0, 0.0, -200.0]], device=DEV)
    assert selective.uncertainty(ends, True, "alpha", "separate").tolist() == [1.0, 0.0]


# ---- curve -------------------------------------------------------------------------------------------------------------------------------
def _curve(probs, labels, u):
    rc = selective.risk_coverage(*_dev(probs, labels, u))
    Mv = int(rc.counts[0])
    return rc, {"order": rc.order[:Mv].cpu().numpy(), "acc": rc.acc[:Mv].cpu().numpy(), "bal_acc": rc.bal_acc[:Mv].cpu().numpy(),
                "f1_mean": rc.f1_mean[:Mv].cpu().numpy(), "threshold": rc.threshold[:Mv].cpu().numpy(), "aurc": float(rc.aurc),
                "counts": rc.counts.cpu().numpy()}


def _check_curve(probs, labels, u):
    want = sc.risk_coverage_ref(probs, labels, u)  # from the same fp32 arrays the kernel reads
    rc, got = _curve(probs, labels, u)
    assert got["counts"].tolist() == want["counts"].tolist()
    assert got["order"].dtype == np.int32 and np.array_equal(got["order"], want["order"])
    assert np.array_equal(got["threshold"], want["threshold"], equal_nan=True)
    for k in ("acc", "bal_acc", "f1_mean"):  # the gate test_gpu_eval_metrics.py uses for its fp64 sums
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    np.testing.assert_allclose(got["aurc"], want["aurc"], rtol=1e-12, atol=0)
    _, again = _curve(probs, labels, u)  # two calls are bitwise equal
    for k in ("order", "acc", "bal_acc", "f1_mean", "counts"):
        assert np.array_equal(got[k], again[k]), k
    assert np.array_equal(got["threshold"].view(np.int32), again["threshold"].view(np.int32)) and (got["aurc"] == again["aurc"] or np.isnan(got["aurc"]))
    ea, want_ea = float(rc.error_auroc), sc.error_auroc_ref(probs, labels, u)
    assert (np.isnan(ea) and np.isnan(want_ea)) or abs(ea - want_ea) <= 1e-12
    return rc, want


@pytest.mark.parametrize("K", [2, 3, 16])
@pytest.mark.parametrize("M", [1, 257, 600, 2500])  # 257 and 600 cross the rank tiles in both directions, 2500 the scan block
def test_risk_coverage_matches_the_restatement(M, K):
    _check_curve(*sc.curve_case(M, K, seed=100 * K + M % 97))


def test_risk_coverage_all_equal_and_nan_uncertainties():
    rc, want = _check_curve(*sc.curve_case(600, 3, 7, "equal"))
    assert np.array_equal(want["order"], np.nonzero(sc.curve_case(600, 3, 7, "equal")[1] >= 0)[0])  # all tied: the row order
    rc, want = _check_curve(*sc.curve_case(600, 3, 8, "nan"))
    assert want["counts"][1] == 2 and np.isnan(want["threshold"][-2:]).all() and want["order"][-2] < want["order"][-1]
    assert np.isnan(float(rc.error_auroc))
    at = rc.at([1.0, 0.5, 1e-9])
    m = selective.coverage_rows([1.0, 0.5, 1e-9], int(want["counts"][0]))
    assert at["rows"] == m.tolist() and at["valid_rows"] == want["counts"][0] and at["nan_rows"] == 2
    for k, name in (("acc", "accuracy"), ("bal_acc", "bal_accuracy"), ("f1_mean", "f1_mean")):
        np.testing.assert_allclose(at[name], want[k][m - 1], rtol=1e-12, atol=0)
    assert np.isnan(at["threshold"][0]) and at["threshold"][1:] == want["threshold"][m[1:] - 1].tolist()
    # signed zeros tie, an out-of-range label is ignored like padding, and the first of two equal probabilities is the prediction
    probs = np.array([[0.5, 0.5], [0.2, 0.8], [0.5, 0.5], [0.9, 0.1]], dtype=np.float32)
    _, got = _curve(probs, np.array([1, 1, 0, 2], dtype=np.int32), np.array([0.0, -1.0, -0.0, -2.0], dtype=np.float32))
    assert got["order"].tolist() == [1, 0, 2] and got["acc"].tolist() == [1.0, 0.5, 2 / 3]


@pytest.mark.parametrize("M", [70001, 1 << 20])
def test_risk_coverage_past_one_chunk_of_rows(M):
    """70 001 rows: the row chunks of the rank launch are longer than their 1024-row minimum; 2^20 rows: the largest call (64 chunks of
    16 384 rows, 1024 scan blocks).  Order, counts and accuracy against the vectorised forms (the per-prefix loop of the restatement
    would take seconds here)."""
    probs, labels, u = sc.curve_case(M, 3, 5)
    _, got = _curve(probs, labels, u)
    order = sc.order_ref(u, labels, 3)
    assert got["counts"].tolist() == [order.size, 0] and np.array_equal(got["order"], order)
    lab, prd = labels[order], probs.argmax(1)[order]
    eye = np.eye(3)
    sup, pre, tp = eye[lab].cumsum(0), eye[prd].cumsum(0), (eye[lab] * (lab == prd)[:, None]).cumsum(0)
    np.testing.assert_allclose(got["acc"], tp.sum(1) / np.arange(1, order.size + 1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["bal_acc"], np.where(sup > 0, tp / np.maximum(sup, 1), 0).sum(1) / (sup > 0).sum(1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["f1_mean"], np.where(sup + pre > 0, 2 * tp / np.maximum(sup + pre, 1), 0).mean(1), rtol=1e-12, atol=0)
    assert np.array_equal(got["threshold"], u[order])
    np.testing.assert_allclose(got["aurc"], np.mean(1.0 - got["acc"]), rtol=1e-12, atol=0)


# ---- groups ------------------------------------------------------------------------------------------------------------------------------
def _groups(probs, u, labels, keys, **kw):
    groups = selective.build_groups(keys)
    gp = selective.group_predictions(*_dev(probs, u, labels), groups, **kw)
    return groups, {"p_mean": gp.p_mean.cpu().numpy(), "p_conf": gp.p_conf.cpu().numpy(), "u_mean": gp.u_mean.cpu().numpy(),
                    "label": gp.labels.cpu().numpy(), "count": gp.counts.cpu().numpy(), "status": gp.status.cpu().numpy()}


def _check_groups(probs, u, labels, keys):
    (offsets, rows, names), got = _groups(probs, u, labels, keys)
    want = sc.group_ref(probs, u, labels, offsets, rows)  # fp64, the same row order
    for k in ("p_mean", "p_conf", "u_mean"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    for k in ("label", "count", "status"):
        assert got[k].tolist() == want[k].tolist(), k
    _, again = _groups(probs, u, labels, keys)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k  # bitwise
    return names, got


def test_group_predictions_match_the_restatement():
    probs, u, labels, keys = sc.group_case(2)
    names, got = _check_groups(probs, u, labels, keys)  # 50 groups of one row, 700 scattered rows in one group, a group with u = 1
    sure = names.index("sure")
    assert np.array_equal(got["p_conf"][sure], got["p_mean"][sure]) and got["u_mean"][sure] == 1.0 and got["count"][names.index("big")] == 700
    one = [g for g, n in enumerate(names) if n.startswith("one")]
    first_row = {k: i for i, k in reversed(list(enumerate(keys)))}
    assert np.array_equal(got["p_mean"][one], probs[[first_row[names[g]] for g in one]].astype(np.float64))
    _check_groups(probs[:9], u[:9], np.zeros(9, np.int32), ["only"] * 9)  # G = 1
    u_nan = u[:9].copy()
    u_nan[[2, 5]] = np.nan  # counted in status[1]; the group's weighted mean and mean uncertainty are NaN, its plain mean is not
    _, got = _check_groups(probs[:9], u_nan, np.zeros(9, np.int32), ["only"] * 9)
    assert got["status"].tolist() == [0, 2] and np.isnan(got["p_conf"]).all() and np.isfinite(got["p_mean"]).all()
    _check_groups(probs[:300], u[:300], np.ones(300, np.int32), ["only"] * 300)  # G = 1 on the block path
    _check_groups(sc.softmax64(sc.score_logits(400, 16, 3)).astype(np.float32), u[:400], labels[:400] * 0, [i % 3 for i in range(400)])  # 16 classes


def test_group_label_conflict_raises():
    probs, u, labels, keys = sc.group_case(4)
    labels = labels.copy()
    labels[[i for i, k in enumerate(keys) if k == "big"][3]] += 1
    labels[[i for i, k in enumerate(keys) if k == "cine7"][1]] += 1
    with pytest.raises(ValueError, match="2 group"):
        selective.group_predictions(*_dev(probs, u, labels), selective.build_groups(keys))
    _, got = _groups(probs, u, labels, keys, check=False)  # nothing branches on the status: the groups are still averaged
    assert got["status"].tolist() == [2, 0] and np.isfinite(got["p_conf"]).all()
    with pytest.raises(ValueError, match="lie in"):
        selective.group_predictions(*_dev(probs[:10], u[:10], labels[:10]), selective.build_groups(keys))  # rows past the tensors


# ---- evaluator ---------------------------------------------------------------------------------------------------------------------------
class _Head(torch.nn.Module):
    """The model surface EpochEvaluator reads."""

    def __init__(self, P=8, K=4):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.num_classes, self.num_prototypes, self.prototype_shape = K, P, (P, 8, 1, 1, 1)
        self.prototype_class_identity = torch.zeros(P, K)
        for j in range(P):
            self.prototype_class_identity[j, j // (P // K)] = 1


def test_selective_evaluator_on_a_bare_head():
    rng = np.random.default_rng(12)
    B, nb, K = 7, 9, 4
    names = [f"cine{g}" for g in range(11)]
    keys = [names[int(g)] for g in rng.integers(0, len(names), B * nb)]
    label_of = {n: g % 3 for g, n in enumerate(names)}
    y = np.array([label_of[k] for k in keys])
    lg = sc.score_logits(B * nb, K, 21)
    sel = selective.SelectiveEvaluator(_Head().to(DEV), abstain_class=True, capacity=8)
    for b in range(nb):
        s = slice(b * B, (b + 1) * B)
        sel.update(torch.from_numpy(lg[s]).to(DEV), torch.rand(B, 8, device=DEV), torch.from_numpy(y[s]).to(DEV), keys[s])
    probs, u = sel.ev.probs[: sel.ev.rows].cpu().numpy(), selective.uncertainty(torch.from_numpy(lg).to(DEV), True).cpu().numpy()
    cs = (1.0, 0.9, 0.8, 0.7, 0.5)

    def check(res, want, ea):
        m = selective.coverage_rows(cs, int(want["counts"][0]))
        for j, c in enumerate(cs):
            for name, k in (("accuracy", "acc"), ("bal_accuracy", "bal_acc"), ("f1_mean", "f1_mean")):
                np.testing.assert_allclose(res[f"{name}@{c:g}"], want[k][m[j] - 1], rtol=1e-12, atol=0)
            assert res[f"threshold@{c:g}"] == float(want["threshold"][m[j] - 1])
        np.testing.assert_allclose(res["aurc"], want["aurc"], rtol=1e-12, atol=0)
        assert abs(res["error_auroc"] - ea) <= 1e-12 and res["rows"] == want["counts"][0] and res["nan_rows"] == 0

    clip = sel.finish(cs, level="clip")
    check(clip, sc.risk_coverage_ref(probs, y, u), sc.error_auroc_ref(probs, y, u))
    assert "groups" not in clip
    cine = sel.finish(cs, level="cine")
    offsets, rows, gnames = selective.build_groups(keys)
    g = sc.group_ref(probs, u, y, offsets, rows)
    p32, u32 = g["p_conf"].astype(np.float32), g["u_mean"].astype(np.float32)
    check(cine, sc.risk_coverage_ref(p32, g["label"], u32), sc.error_auroc_ref(p32, g["label"], u32))
    assert cine["groups"] == len(gnames) == len(cine["cines"]) and [c["filename"] for c in cine["cines"]] == gnames
    cm = np.zeros((3, 3), np.int64)
    np.add.at(cm, (g["label"], p32.argmax(1)), 1)
    _, bal, f1 = sc.confusion_metrics(cm)
    np.testing.assert_allclose([cine["accuracy"], cine["f1_mean"]], [bal, f1], rtol=1e-12, atol=0)
    import metric_cases as mc

    assert abs(cine["auc"] - mc.auc_ovr_weighted(p32, g["label"], 3)[0]) <= 1e-12 and len(cine["auc_per_class"]) == 3
    for c, n in zip(cine["cines"], range(len(gnames))):
        assert c["target_AS"] == g["label"][n] and c["n_clips"] == g["count"][n] and c["pred"] == int(p32[n].argmax())
        np.testing.assert_allclose(c["probs"], g["p_conf"][n], rtol=1e-12, atol=0)
        np.testing.assert_allclose(c["uncertainty"], g["u_mean"][n], rtol=1e-12, atol=0)
    assert sel.finish(cs, level="cine") == cine  # finish reads; it consumes nothing
    sel.update(torch.from_numpy(lg[:1]).to(DEV), torch.rand(1, 8, device=DEV), torch.tensor([(label_of[keys[0]] + 1) % 3], device=DEV), keys[:1])
    with pytest.raises(ValueError, match="different labels"):
        sel.finish(cs, level="cine")


# ---- trainer -----------------------------------------------------------------------------------------------------------------------------
def _cine_loader(n, B, seed):
    """n batches of B clips of three cines, each cine's clips spread over several batches."""
    class L(list):
        batch_size = B

    out = L()
    for b in range(n):
        which = [(b + 2 * i) % 3 for i in range(B)]
        out.append({"cine": synth.echo_clips((B, 3, 4, 64, 64), seed=seed + b), "target_AS": torch.tensor(which),
                    "filename": [f"cine{w}.mat" for w in which], "interval_idx": torch.arange(B) + 10 * b})
    return out


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


@pytest.mark.timeout(900)
def test_trainer_evaluate_selective(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to(DEV)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    loader = _cine_loader(4, 3, 70)
    logs = []
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda s, *_: logs.append(str(s)))
    before = t.evaluate("test")
    state = (t.current_epoch, t.current_iteration, m.training)
    res = t.evaluate_selective("test", level="cine")
    assert any("AURC" in s for s in logs) and (t.current_epoch, t.current_iteration, m.training) == state
    # the same sweep fed by hand
    sel = selective.SelectiveEvaluator(m, abstain_class=True)
    with torch.no_grad():
        for b in loader:
            lg, sim, _ = m(b["cine"].to(DEV))
            sel.update(lg, sim, b["target_AS"].to(DEV), b["filename"])
    assert _same(res, sel.finish(level="cine"))
    assert res["groups"] == 3 and res["rows"] == 3 and sorted(c["n_clips"] for c in res["cines"]) == [4, 4, 4]
    assert all(f"{n}@{c}" in res for n in ("accuracy", "bal_accuracy", "f1_mean", "threshold") for c in ("1", "0.9", "0.8", "0.7", "0.5"))
    with open(tmp_path / "csv_test_cine" / "e00.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["filename", "target_AS", "n_clips", "prob_No AS", "prob_Early AS", "prob_Significant AS", "uncertainty", "pred"]
    assert len(rows) == 4 and [r[0] for r in rows[1:]] == [c["filename"] for c in res["cines"]] and sorted(r[0] for r in rows[1:]) == [f"cine{w}.mat" for w in range(3)]
    for r, c in zip(rows[1:], res["cines"]):
        assert [int(r[1]), int(r[2]), int(r[7])] == [c["target_AS"], 4, c["pred"]] and [float(v) for v in r[3:7]] == c["probs"] + [c["uncertainty"]]
        assert c["target_AS"] == int(c["filename"][4]) and abs(sum(c["probs"]) - 1) < 1e-6 and 0 < c["uncertainty"] < 1
    clip = t.evaluate_selective("test", level="clip", coverages=(1.0, 0.5))
    assert clip["rows"] == 12 and "groups" not in clip and "accuracy@0.5" in clip and sorted(os.listdir(tmp_path)) == ["csv_test", "csv_test_cine"]
    assert _same(t.evaluate("test"), before)  # the new entry left no state behind
