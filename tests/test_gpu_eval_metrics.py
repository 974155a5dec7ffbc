"""GPU: evaluation metrics (csrc/eval_metrics.hip through protoasnet_amd.metrics) against the G9 fixture of the reference's own code and
the numpy restatements of tests/metric_cases.py; DPTrainer.evaluate("test") on the HIP Video ProtoASNet; two gloo ranks on one card."""
import csv
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metric_cases as mc
from protoasnet_amd import metrics, synth
from test_cpu_trainer import TRAIN_CFG, Toy, _free_port
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_sparsity_metric_matches_the_reference(golden):
    g = golden("g9_metrics.npz")
    for case, batches in mc.sparsity_batches().items():
        m = metrics.SparsityMetric(level=0.8, device=DEV)
        vals = [m(b.to(DEV)) for b in batches]
        assert all(v.is_cuda for v in vals)
        assert torch.stack(vals).cpu().numpy().tolist() == g[f"sparsity_{case}_batch"].tolist(), case
        assert [int(m.percentage_expl), int(m.total)] == g[f"sparsity_{case}_sum"].tolist()
        assert float(m.compute()) == float(g[f"sparsity_{case}_epoch"])
        m.reset()
        assert int(m.total) == 0


def test_sparsity_rows_match_the_restatement():
    gen = torch.Generator().manual_seed(31)
    sim = torch.cat([torch.rand(64, 40, generator=gen) ** e for e in (1, 3, 9)])
    sim[7] = 0.0
    want, margin = mc.sparsity_rows(sim.numpy())
    m = metrics.SparsityMetric(level=0.8, device=DEV)
    got = [int(m(sim[i: i + 1].to(DEV)).item()) for i in range(sim.shape[0])]
    keep = margin > 1e-6
    assert keep.sum() > 150
    assert np.array(got)[keep].tolist() == want[keep].tolist()


class _Head(torch.nn.Module):
    """The model surface EpochEvaluator reads: num_classes, prototype_class_identity, prototype_shape (video: 5-D)."""

    def __init__(self, P=40, K=4, video=True):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.num_classes, self.num_prototypes = K, P
        self.prototype_shape = (P, 8, 1, 1, 1) if video else (P, 8, 1, 1)
        self.prototype_class_identity = torch.zeros(P, K)
        for j in range(P):
            self.prototype_class_identity[j, j // (P // K)] = 1


def _batches(n, B, P=40, K=4, seed=0):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        sim = torch.randperm(B * P, generator=gen).float().view(B, P) / (B * P)  # tie-free
        out.append((torch.randn(B, K, generator=gen) * 3, sim, torch.randint(0, K - 1, (B,), generator=gen)))
    return out


def test_batch_stats_probs_diversity_and_similarity_sums():
    head = _Head().to(DEV)
    data = _batches(5, 7)
    row = data[2][1][3]  # a planted tie at the top-5 boundary of the class prototypes: the lower index takes the last place
    row[:4] = torch.tensor([3.0, 2.9, 2.8, 2.7])
    row[4] = row[9] = 2.0
    results = []
    for _ in range(3):
        ev = metrics.EpochEvaluator(head, abstain_class=True, keep_logits=True, capacity=8)  # capacity 8: grows twice
        for lg, sim, y in data:
            ev.update(lg.to(DEV), sim.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        results.append((ev.probs[: ev.rows].cpu(), ev.labels[: ev.rows].cpu(), ev.logits[: ev.rows].cpu(), ev.div_counts.cpu(),
                        ev.sim_sums.cpu(), ev.finish()))
    probs, labels, logits, counts, sums, res = results[0]
    lg = torch.cat([d[0] for d in data])
    sim = torch.cat([d[1] for d in data])
    y = torch.cat([d[2] for d in data])
    assert ev.capacity == 64 and ev.rows == 35
    assert (probs - torch.softmax(lg[:, :3], dim=1)).abs().max() <= 1e-6
    assert labels.tolist() == y.tolist() and torch.equal(logits, lg)
    assert counts.tolist() == mc.diversity_counts(sim.numpy(), 30).tolist()
    assert counts[:30].sum() == 35 * 5 and counts[30:].sum() == 35 * 2
    assert mc.diversity_counts(sim[17:18].numpy(), 30)[[4, 9]].tolist() == [1, 0]  # (row 3 of batch 2)
    ref = sim.double().sum(0)
    assert ((sums - ref).abs() <= 1e-12 * ref.abs()).all()
    for r in results[1:]:  # bitwise reproducible
        assert torch.equal(r[4], sums) and torch.equal(r[3], counts) and torch.equal(r[0], probs)
    sp, _ = mc.sparsity_rows(sim.numpy())
    assert res["sparsity"] == sp.sum() / sp.size
    thr = 0.05 * 35
    assert res["diversity"] == int((counts[:30] > thr).sum()) and res["diversity_abstain"] == int((counts[30:] > thr).sum())
    a, per = mc.auc_ovr_weighted(probs.numpy(), labels.numpy(), 3)
    assert res["auc_per_class"] == per.tolist(), (res["auc_per_class"], per.tolist())
    assert res["auc"] == a, (res["auc"], a)
    assert metrics.EpochEvaluator(_Head(video=False).to(DEV)).diversity_threshold == 0.3


def test_auc_matches_sklearn(golden):
    g = golden("g9_metrics.npz")
    if not any(k.startswith("auc_") for k in g.files):
        pytest.skip("the fixture was made without sklearn")
    for case, (p, y) in mc.auc_cases().items():
        a = metrics.roc_auc_ovr_weighted(torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV), 3)
        assert a.is_cuda and a.dtype == torch.float64
        assert abs(float(a) - float(g[f"auc_{case}"])) <= 1e-12, case


def test_auc_exact_on_heavy_ties_and_padding():
    rng = np.random.default_rng(5)
    M = 20000
    y = rng.integers(0, 3, M)
    p = (np.round(rng.random((M, 3)) * 64) / 64).astype(np.float32)  # quantised to 1/64: heavy ties
    p[: M // 2, 0] += (y[: M // 2] == 0) * np.float32(1 / 64)
    a, per = metrics.roc_auc_ovr_weighted(torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV), 3, per_class=True)
    ra, rper = mc.auc_ovr_weighted(p, y, 3)
    assert per.cpu().numpy().tolist() == rper.tolist()
    assert float(a) == ra, (float(a), ra, per.cpu().tolist())
    yp = np.concatenate([y[:777], -np.ones(300, np.int64), y[777:]])
    pp = np.concatenate([p[:777], rng.random((300, 3)).astype(np.float32), p[777:]])
    assert float(metrics.roc_auc_ovr_weighted(torch.from_numpy(pp).to(DEV), torch.from_numpy(yp).to(DEV), 3)) == ra


def test_auc_hand_cases():
    def auc(p, y, K=3):
        return metrics.roc_auc_ovr_weighted(torch.tensor(p, dtype=torch.float32, device=DEV), torch.tensor(y, device=DEV), K, per_class=True)

    y = [0, 0, 1, 1, 2, 2]
    perfect = np.eye(3, dtype=np.float32)[y]
    assert float(auc(perfect, y)[0]) == 1.0
    assert float(auc(1 - perfect, y)[0]) == 0.0
    assert float(auc(np.full((6, 3), 1 / 3), y)[0]) == 0.5
    a, per = auc(perfect[:4], y[:4])
    assert float(a) == 0.0 and torch.isnan(per[2]) and float(per[0]) == 1.0
    bad = perfect.copy()
    bad[1, 2] = np.nan
    a, per = auc(bad, y)
    assert float(a) == 0.0 and torch.isnan(per).all()
    assert float(auc(perfect, y[:5] + [3])[0]) == 0.0  # a label outside range(K_real): sklearn raises
    s = np.array([0.1, 0.4, 0.35, 0.8], np.float32)
    assert float(auc(np.stack([1 - s, s], 1), [0, 0, 1, 1], K=2)[0]) == 0.75  # K_real = 2: the binary AUC
    assert float(auc(np.concatenate([perfect, np.zeros((3, 3))]), y + [-1, -1, -1])[0]) == 1.0


def _video_loader(n, B, seed):
    class L(list):
        batch_size = B

    out = L()
    for b in range(n):
        out.append({"cine": synth.echo_clips((B, 3, 4, 64, 64), seed=seed + b), "target_AS": (torch.arange(B) + b) % 3,
                    "filename": [f"c{b}_{i}" for i in range(B)], "interval_idx": torch.arange(B) + 10 * b})
    return out


@pytest.mark.timeout(900)
def test_trainer_evaluate_test_split(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": TRAIN_CFG}
    loader = _video_loader(4, 3, 70)
    logs = []
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda s, *_: logs.append(str(s)))
    res = t.evaluate("test")
    assert any("AUC" in s and "sparsity" in s for s in logs)
    # restatement from a separate pass over the same loader
    with torch.no_grad():
        outs = [m(b["cine"].to(DEV)) for b in loader]
    lg = torch.cat([o[0] for o in outs]).float().cpu()
    sim = torch.cat([o[1] for o in outs]).float().cpu()
    y = torch.cat([b["target_AS"] for b in loader])
    sp, _ = mc.sparsity_rows(sim.numpy())
    assert res["sparsity"] == sp.sum() / sp.size
    counts = mc.diversity_counts(sim.numpy(), 30)
    assert res["diversity"] == int((counts > 0.05 * 12).sum()) and res["diversity_abstain"] is None
    assert np.allclose(res["simscore_sum"], sim.double().sum(0).numpy(), rtol=1e-12, atol=0)
    a, _ = mc.auc_ovr_weighted(torch.softmax(lg, 1).numpy(), y.numpy(), 3)
    assert abs(res["auc"] - a) <= 1e-12 and len(res["auc_per_class"]) == 3
    files = os.listdir(tmp_path / "csv_test")
    assert files == [f"e00_f1_{res['f1_mean']:.0%}.csv"]
    with open(tmp_path / "csv_test" / files[0]) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["", "filename", "target_AS", "interval_idx", "logit_No AS", "logit_Early AS", "logit_Significant AS"]
    assert len(rows) == 13 and [r[1] for r in rows[1:]] == [f"c{b}_{i}" for b in range(4) for i in range(3)]
    assert np.abs(np.array([[float(v) for v in r[4:]] for r in rows[1:]]) - lg.numpy()).max() <= 1e-6
    assert "auc" in t.run_epoch(0, "val") and not os.path.exists(tmp_path / "csv_val")  # every mode has the metrics, CSV only in val_push / test


# ---- two gloo ranks on one card: every metric equals one process over the union of the shards ------------------------------------------
def _toy_shards():
    g = torch.Generator().manual_seed(3)

    def batch(B, tag):
        return {"cine": torch.randn(B, 3, 2, 6, 6, generator=g), "target_AS": torch.arange(B) % 3, "filename": [f"{tag}_{i}" for i in range(B)]}

    return [[batch(4, "r0b0"), batch(4, "r0b1"), batch(3, "r0b2")], [batch(4, "r1b0"), batch(4, "r1b1"), batch(1, "r1b2")]]


def _run(rank, world, loader, save_dir):
    from protoasnet_amd.trainer import DPTrainer

    cfg = {"abstain_class": True, "save_dir": save_dir, "train": TRAIN_CFG}
    t = DPTrainer(Toy(P=40, K=4).to(DEV), cfg, {"train": loader, "test": loader}, rank=rank, world_size=world, log=lambda *_: None)
    return t.evaluate("test")


def _gloo_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _run(rank, world, _toy_shards()[rank], os.path.join(out_dir, "dp"))
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_gloo_ranks_equal_one_process_over_the_union(tmp_path):
    port = _free_port()
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    shards = _toy_shards()
    one = _run(0, 1, shards[0] + shards[1], str(tmp_path / "single"))
    for r in range(2):
        res = torch.load(tmp_path / f"rank{r}.pt")
        for k in ("auc", "auc_per_class", "sparsity", "diversity", "diversity_abstain"):
            assert res[k] == one[k] or (k == "auc_per_class" and np.array_equal(res[k], one[k], equal_nan=True)), (r, k)
        assert np.allclose(res["simscore_sum"], one["simscore_sum"], rtol=1e-12, atol=0)
    (name,) = os.listdir(tmp_path / "dp" / "csv_test")
    with open(tmp_path / "dp" / "csv_test" / name) as f:
        dp_rows = list(csv.reader(f))
    with open(tmp_path / "single" / "csv_test" / os.listdir(tmp_path / "single" / "csv_test")[0]) as f:
        one_rows = list(csv.reader(f))
    assert len(dp_rows) == 1 + 20 and [r[:3] for r in dp_rows] == [r[:3] for r in one_rows]  # rank-major: rank 0's clips, then rank 1's
    assert np.abs(np.array([[float(v) for v in r[3:]] for r in dp_rows[1:]]) - np.array([[float(v) for v in r[3:]] for r in one_rows[1:]])).max() <= 1e-6
