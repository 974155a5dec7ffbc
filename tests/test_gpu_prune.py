"""GPU: the pruning kernels against the float64 / int64 restatement (prune_cases.py) -- integer tallies exact, margin sums, trace and z
bit for bit --, the surgery on real models against the unpruned model's outputs, and the trainer entry."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import prune_cases as pc
from conftest import TOL_LOGITS, assert_close
from protoasnet_amd import synth
from util import CFG_PUSH_PPNET, CFG_PUSH_XIMG, CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = pc.CHUNK


def _dev(sim, w, labels, cls):
    return (torch.from_numpy(sim).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(cls).to(DEV))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _run(case, K_real, rounds, floors, accept, max_extra=0, margin_fraction=None):
    from protoasnet_amd import prune

    res = prune._run(*_dev(*case)[:3], K_real, _dev(*case)[3], rounds, floors if rounds else None, accept, max_extra, margin_fraction)
    return res, res.read()


def _check(case, K_real, rounds, floors, accept, max_extra=0, margin_fraction=None):
    """One elimination on the device against the restatement; returns (restatement, device read)."""
    sim, w, labels, cls = case
    ref = pc.eliminate(sim, w, labels, K_real, cls, rounds, floors, accept, max_extra, margin_fraction)
    res, out = _run(case, K_real, rounds, floors, accept, max_extra, margin_fraction)
    wrong, flips, per, ms = ref["table"]
    P = sim.shape[1]
    t = out["table"]
    assert np.array_equal(np.append(t["wrong"], t["wrong_0"]), wrong) and np.array_equal(t["flips"], flips[:P])
    assert np.array_equal(np.vstack([t["wrong_per_class"], t["wrong_per_class_0"][None]]), per)
    assert np.array_equal(_bits(np.append(t["margin_sum"], t["margin_sum_0"])), _bits(ms))  # bit for bit
    assert out["removed"] == ref["removed"].tolist()
    assert np.array_equal(out["kept_mask"], ref["kept"])
    if rounds:
        assert np.array_equal(out["trace_wrong"], ref["trace_wrong"]) and np.array_equal(_bits(out["trace_margin"]), _bits(ref["trace_margin"]))
    assert np.array_equal(_bits(res.z.cpu().numpy()), _bits(ref["z"]))
    return ref, out


def test_chunk_constant():
    from protoasnet_amd import prune

    assert prune.chunk() == C


@pytest.mark.parametrize("M,P,K,K_real,g", [
    (1, 8, 3, 2, 1),                # one row; the abstention column and its prototypes are present and ignored
    (C - 1, 72, 4, 4, 16),          # one chunk short of full; more than one wave of candidates
    (C + 1, 8, 3, 2, 2),            # a second chunk of one row
    (3 * C + 5, 72, 3, 2, 22),      # several chunks, a tail, unlabelled rows, abstention prototypes in the second wave of lanes
    (C + 1, 256, 4, 4, 62),         # the widest table
    (3 * C + 5, 8, 4, 4, 1),
])
def test_kernel_equals_restatement_at_every_shape(M, P, K, K_real, g):
    case = pc.make_case(M, P, K, K_real, seed=M * 7 + P, unlabeled=0.15 if M > 1 else 0.0, wide=True)  # (sums that round: the order shows)
    floors = pc.floors_for(K_real, g)
    ref, out = _check(case, K_real, pc.rounds_for(case[3], K_real, floors), floors, False)
    assert (ref["removed"] >= 0).all()
    assert (case[3][ref["kept"] == 0] < K_real).all()  # an abstention prototype is never removed
    _check(case, K_real, 0, None, False)  # importance alone: the same table without a loop


def test_importance_is_the_round_zero_table():
    from protoasnet_amd import prune

    case = pc.make_case(2 * C + 9, 40, 5, 4, seed=11, unlabeled=0.1, informative=0.5)
    t = prune.importance(*_dev(*case)[:3], 4, _dev(*case)[3]).read()
    z = pc.base_logits(case[0], case[1], np.ones(40), 4)
    wrong, flips, per, ms = pc.round_table(z, *case[:3], np.ones(40), 4)
    assert np.array_equal(t["d_wrong"], wrong[:40] - wrong[40]) and np.array_equal(t["flips"], flips[:40])
    assert np.array_equal(t["d_wrong_per_class"], per[:40] - per[40]) and np.array_equal(_bits(t["d_margin"]), _bits(ms[:40] - ms[40]))


def test_ties_identical_prototypes_tied_rows_and_a_class_at_its_floor():
    sim, w, labels, _ = pc.make_case(2 * C + 3, 9, 3, 3, seed=5, unlabeled=0.1)
    cls = np.array([0, 0, 1, 1, 1, 1, 2, 2, 2], np.int32)
    sim[:, 4], w[:, 4] = sim[:, 3], w[:, 3]  # two identical prototypes of class 1: equal keys, the lower index goes first
    sim[::5] = 0  # rows whose logits are all equal (and stay so under every ablation): the lowest class is predicted
    labels[5], labels[10] = 1, 0
    ref, out = _check((sim, w, labels, cls), 3, 3, [2, 2, 2], False)  # class 0 stands at its floor from the start
    assert out["table"]["wrong"][3] == out["table"]["wrong"][4] and out["table"]["margin_sum"][3] == out["table"]["margin_sum"][4]
    assert all(cls[p] != 0 for p in out["order"]) and len(out["order"]) == 3
    # the two copies alone are candidates: class 2 at its floor as well, one round -- the lower index must go
    cls2 = np.array([0, 0, 2, 1, 1, 2, 2, 0, 0], np.int32)
    ref, out = _check((sim, w, labels, cls2), 3, 1, [4, 1, 3], False)
    assert out["order"] == [3]
    z = pc.base_logits(sim, w, np.ones(9), 3)
    assert (z[5] == 0).all() and ref["table"][2][9, 1] >= 1  # the tied row of class 1 is predicted 0: wrong


def test_acceptance_test_stops_the_loop_and_later_rounds_record_minus_one():
    case = pc.make_case(2 * C + 40, 16, 4, 4, seed=2, unlabeled=0.05, informative=0.6)
    ref, out = _check(case, 4, 12, [1, 1, 1, 1], True, 0, None)
    rm = ref["removed"]
    first = int(np.flatnonzero(rm < 0)[0])
    assert 1 <= first < 11 and (rm[first:] == -1).all() and out["stopped"]  # it stops early, after at least one removal
    assert (ref["trace_wrong"][first:] == ref["trace_wrong"][first]).all()
    # ... and with a margin condition and an error allowance
    ref2, _ = _check(case, 4, 12, [1, 1, 1, 1], True, 3, 0.9)
    assert not np.array_equal(ref2["removed"], rm)


def test_keep_per_class_three_classes_times_four_down_to_two():
    from protoasnet_amd import prune

    case = pc.make_case(C + 17, 12, 3, 3, seed=9, informative=0.5)
    ref = pc.eliminate(*case[:3], 3, case[3], 6, [2, 2, 2], False)
    out = prune.eliminate(*_dev(*case)[:3], 3, _dev(*case)[3], keep_per_class=2).read()
    assert out["removed"] == ref["removed"].tolist() and len(out["order"]) == 6 and not out["stopped"]
    assert np.bincount(case[3][out["kept"]], minlength=3).tolist() == [2, 2, 2]
    assert np.array_equal(_bits(out["trace_margin"]), _bits(ref["trace_margin"]))


def test_two_calls_are_bitwise_equal():
    case = pc.make_case(5 * C + 3, 72, 4, 4, seed=21, unlabeled=0.1, wide=True)
    outs = []
    for _ in range(2):
        res, out = _run(case, 4, 6, [17] * 4, False)
        outs.append((out, res.z.cpu().numpy()))
    (a, za), (b, zb) = outs
    assert a["removed"] == b["removed"] and np.array_equal(a["trace_wrong"], b["trace_wrong"])
    assert np.array_equal(_bits(a["trace_margin"]), _bits(b["trace_margin"])) and np.array_equal(_bits(za), _bits(zb))
    assert np.array_equal(_bits(a["table"]["margin_sum"]), _bits(b["table"]["margin_sum"])) and np.array_equal(a["table"]["flips"], b["table"]["flips"])


def test_interleaved_unlabelled_rows_move_only_the_chunk_cut():
    sim, w, labels, cls = pc.make_case(2 * C + 50, 24, 3, 3, seed=4)
    M = sim.shape[0]
    _, a = _run((sim, w, labels, cls), 3, 0, None, False)
    sim2, lab2 = np.zeros((2 * M, 24), np.float32), np.full(2 * M, -1, np.int32)
    sim2[::2], lab2[::2] = sim, labels
    sim2[1::2] = sim[::-1]  # rows that would count if the label were read wrongly
    _, b = _run((sim2, w, lab2, cls), 3, 0, None, False)
    ta, tb = a["table"], b["table"]
    for k in ("wrong", "flips", "wrong_per_class", "wrong_0", "wrong_per_class_0"):
        assert np.array_equal(ta[k], tb[k]), k
    err = np.abs(np.append(ta["margin_sum"] - tb["margin_sum"], ta["margin_sum_0"] - tb["margin_sum_0"])).max()
    print(f"margin sums, cut moved: max |difference| {err:.3e} over {M} labelled rows")
    assert err <= 1e-9 * M


@pytest.mark.parametrize("kind", ["wide", "large"])
def test_subtract_chain_stays_within_1e_9_after_a_full_elimination_at_256_prototypes(kind):
    """``wide``: magnitudes over many binades (the order of every sum shows).  ``large``: the worst case the header's bound is derived
    for -- sim in [0.5, 1), w in [1, 2) and all positive, so that z grows to 2P = 2^9 and every subtraction rounds at ulp(2^8 .. 2^9)."""
    sim, w, labels, cls = pc.make_case(C + 1, 256, 4, 4, seed=13, unlabeled=0.1, wide=kind == "wide")
    if kind == "large":
        sim, w = (0.5 + sim / 2).astype(np.float32), (1 + np.abs(w) / 2).astype(np.float32)
        assert sim.min() >= 0.5 and w.min() >= 1 and pc.base_logits(sim, w, np.ones(256), 4).min() > 192
    assert np.abs(w).max() <= 2 and np.abs(sim).max() <= 1
    res, out = _run((sim, w, labels, cls), 4, 252, [1, 1, 1, 1], False)
    assert len(out["order"]) == 252 and len(out["kept"]) == 4
    drift = np.abs(res.z.cpu().numpy() - pc.base_logits(sim, w, out["kept_mask"], 4)).max()
    print(f"{kind}: z after 252 chained subtractions vs the in-order sum over the kept set: max |difference| {drift:.3e}")
    assert drift <= 1e-9


# ---- model level ----------------------------------------------------------------------------------------------------------------------------
# The gates are those of the head-B parity tests of test_gpu_models.py: fp32 from test_video_models_fp32_vs_oracle (similarity and logits
# 1e-3 absolute; occurrence map 1e-3 * max(1, largest entry) absolute + 1e-3 relative), bf16 from test_bf16_compute_tolerance (BF16_SIM 1e-3,
# BF16_LOGITS 2e-3, mean relative occurrence-map error below BF16_OCC_REL 2e-2).
GATES = {torch.float32: (1e-3, 1e-3), torch.bfloat16: (1e-3, 2e-3)}


def _occ_gate(occ, ref, dtype, name):
    if dtype == torch.bfloat16:
        rel = (occ - ref).abs().mean() / ref.abs().mean()
        assert float(rel) < 2e-2, f"{name}: mean relative error {float(rel):.3g}"
    else:
        assert_close(occ, ref, 1e-3 * max(1.0, float(ref.max())), 1e-3, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg,shape,g", [(CFG_PUSH_XIMG, (4, 3, 64, 64), 2), (CFG_VIDEO_X3D, (2, 3, 4, 64, 64), 7)], ids=["XProtoNet", "Video_XProtoNet"])
def test_pruned_head_b_model_is_the_kept_part_of_the_unpruned_one(cfg, shape, g, dtype):
    from protoasnet_amd import prune

    m = synth_model(cfg).to(DEV)
    if dtype == torch.bfloat16:
        m.set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips(shape).to(DEV)
    K = m.num_classes
    labels = (torch.arange(shape[0], device=DEV) % K).to(torch.int32)
    with torch.no_grad():
        logits0, sim0, occ0 = m(x)
    W = m.last_layer.weight.detach().clone()
    res = prune.eliminate(sim0, W, labels, K, prune.proto_classes(m).to(DEV), keep_per_class=g)
    out = res.read()
    keep = prune.apply(m, out["order"])
    assert keep == out["kept"] and len(keep) == K * g == m.num_prototypes
    with torch.no_grad():
        logits1, sim1, occ1 = m(x)  # (on the parent commit: the occurrence conv still has the old width and the head refuses the shapes)
        feats, pdist, occ2, logits2 = m.push_forward(x)
        occ3 = m.compute_occurence_map(x)
    sim_tol, logit_tol = GATES[dtype]
    assert_close(sim1, sim0[:, keep], sim_tol, 0, "similarities of the pruned model vs sim[:, keep]")
    assert_close(logits1, sim0[:, keep] @ W[:, keep].t(), logit_tol, 0, "logits of the pruned model vs sim[:, keep] @ W[:, keep].T")
    _occ_gate(occ1, occ0[:, keep], dtype, "occurrence maps of the pruned model vs the kept channels")
    assert_close(res.z.float(), logits1, logit_tol, 0, "z of the elimination vs the pruned model's logits")
    assert tuple(feats.shape) == (shape[0], len(keep), m.prototype_shape[1]) and tuple(pdist.shape) == (shape[0], len(keep))
    assert torch.equal(occ2, occ1) and torch.equal(logits2, logits1) and occ3.shape == occ1.shape
    _occ_gate(occ3, occ0[:, keep], dtype, "compute_occurence_map of the pruned model")


def test_pruned_ppnet_through_prune_prototypes():
    """Head A: the reference's own method; gates of test_ppnet_resnet18_vs_reference_golden (min distances 1e-3 * largest / 10, logits
    TOL_LOGITS)."""
    from protoasnet_amd import prune

    m = synth_model(CFG_PUSH_PPNET).to(DEV)
    x = synth.echo_clips((4, 3, 64, 64)).to(DEV)
    labels = (torch.arange(4, device=DEV) % 3).to(torch.int32)
    with torch.no_grad():
        logits0, d0 = m(x)
        sim0 = m.distance_2_similarity(d0)
    W = m.last_layer.weight.detach().clone()
    res = prune.eliminate(sim0, W, labels, 3, prune.proto_classes(m).to(DEV), keep_per_class=1)
    out = res.read()
    m.prune_prototypes(out["order"])
    keep = out["kept"]
    with torch.no_grad():
        logits1, d1 = m(x)
        conv, dist = m.push_forward(x)
    assert_close(d1, d0[:, keep], 1e-3 * float(d0.max()) / 10, 0, "min distances of the pruned model")
    assert_close(logits1, sim0[:, keep] @ W[:, keep].t(), TOL_LOGITS, 0, "logits of the pruned model")
    assert_close(res.z.float(), logits1, TOL_LOGITS, 0, "z of the elimination vs the pruned model's logits")
    assert dist.shape[1] == 3 and prune.state(m) == sorted(out["order"])


# ---- trainer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_trainer_prunes_evaluates_explains_trains_and_round_trips_a_checkpoint(tmp_path):
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG
    from test_gpu_trainer import _loader

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    tc = dict(TRAIN_CFG, accumulation_steps=1, save_step=1)
    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": tc}
    logs = []
    loaders = {"train": _loader(1, 10), "val": _loader(3, 50)}
    t = DPTrainer(m, cfg, loaders, log=lambda s, *_: logs.append(str(s)))
    res = t.prune_prototypes("val", keep_per_class=8)
    out = res.read()
    assert m.num_prototypes == 30 and len(out["order"]) == 6 and sum("prune round" in s for s in logs) == 6
    assert tuple(res.z.shape) == (6, 3)  # three batches of two clips, kept on the device
    res2, before, after = t.prune_prototypes("val", apply=True, keep_per_class=8)
    assert res2.read()["removed"] == out["removed"] and m.num_prototypes == 24
    assert torch.isfinite(torch.tensor([before["loss"], after["loss"]])).all()
    assert t.evaluate("val")["loss"] == pytest.approx(after["loss"], rel=1e-6)
    x = loaders["val"][0]["cine"].to(DEV)
    m.eval()
    ex = m.explain(x)
    assert ex is not None
    step = t.run_epoch(0, "train")  # one training step on the pruned model: rebuilt criterion, optimizer and launch lists
    assert torch.isfinite(torch.tensor(step["loss"]))
    t.save_checkpoint()
    ck = torch.load(tmp_path / "last.pth")
    assert len(ck["pruned_prototypes"]) == 6
    m2 = synth_model(CFG_VIDEO_X3D).to(DEV)
    t2 = DPTrainer(m2, cfg, loaders, log=lambda *_: None)
    assert t2.load_checkpoint(str(tmp_path / "last.pth")) and m2.num_prototypes == 24
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    m.eval(), m2.eval()
    with torch.no_grad():
        assert torch.equal(m(x)[0], m2(x)[0])



# ---- unequal blocks per class -----------------------------------------------------------------------------------------------------------------
def _cine_loader(n, seed, B=2):
    from test_gpu_trainer import _loader

    out = _loader(n, seed, B)
    for b, batch in enumerate(out):
        batch["filename"] = [f"cine{int(y)}" for y in batch["target_AS"]]  # one cine per label: the clips of a cine share its label
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("remove,counts", [([0, 1, 2], [7, 10, 10]), ([0, 1, 12, 25], [8, 9, 9])], ids=["27_divides_by_3", "26_does_not"])
def test_unbalanced_model_runs_forward_push_maps_evaluate_and_evaluate_selective(remove, counts, tmp_path):
    from protoasnet_amd import prune
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    x = synth.echo_clips((2, 3, 4, 64, 64)).to(DEV)
    with torch.no_grad():
        logits0, sim0, occ0 = m(x)
    W = m.last_layer.weight.detach().clone()
    loaders = {"train": _cine_loader(1, 10), "val": _cine_loader(3, 50), "test": _cine_loader(3, 50)}
    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": dict(TRAIN_CFG, accumulation_steps=1)}
    t = DPTrainer(m, cfg, loaders, log=lambda *_: None)
    keep = prune.apply(m, remove)
    t._rebuild_after_surgery()
    assert prune.class_counts(m) == counts
    with torch.no_grad():
        logits1, sim1, occ1 = m(x)
        feats, pdist, occ2, logits2 = m.push_forward(x)
        occ3 = m.compute_occurence_map(x)
    assert_close(sim1, sim0[:, keep], 1e-3, 0, "similarities")  # gates: test_video_models_fp32_vs_oracle, as above
    assert_close(logits1, sim0[:, keep] @ W[:, keep].t(), 1e-3, 0, "logits")
    _occ_gate(occ1, occ0[:, keep], torch.float32, "occurrence maps")
    _occ_gate(occ3, occ0[:, keep], torch.float32, "compute_occurence_map")
    assert tuple(feats.shape) == (2, len(keep), 256) and torch.equal(occ2, occ1) and torch.equal(logits2, logits1)
    # an eval epoch: the class-grouped costs follow the class identity -- the cluster term of the epoch is the mean over its batches of the
    # best similarity among the TRUE class's own prototypes
    ev = t.evaluate("val")
    cls = prune.proto_classes(m).to(DEV)
    want = []
    with torch.no_grad():
        for batch in loaders["val"]:
            s = m(t.prepare_input(batch["cine"].to(DEV)))[1]
            y = batch["target_AS"].to(DEV)
            best = torch.stack([s[:, cls == k].max(dim=1)[0] for k in range(3)], dim=1)
            want.append(float(-0.8 * (best * torch.nn.functional.one_hot(y, 3)).mean(dim=0).sum()))
    assert ev["loss_terms"][1] == pytest.approx(sum(want) / len(want), rel=1e-5)
    assert np.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
    sel = t.evaluate_selective("test", level="cine")
    assert np.isfinite(sel["aurc"]) and len(sel["cines"]) == 3
    with pytest.raises(ValueError, match="unbalanced prototype blocks"):
        t.run_epoch(0, "train")
    with pytest.raises(ValueError, match="unbalanced prototype blocks" if sum(counts) % 3 == 0 else "do not split into 3 class blocks"):
        m.eval().explain(x)  # (the second message is the one explain has always had for P % K)


@pytest.mark.timeout(900)
def test_trainer_apply_with_the_acceptance_test_on_leaves_a_model_that_evaluates(tmp_path):
    from protoasnet_amd import prune
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG
    from test_gpu_trainer import _loader

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": dict(TRAIN_CFG, accumulation_steps=1)}
    loaders = {"train": _loader(1, 10), "val": _loader(3, 50)}
    t = DPTrainer(m, cfg, loaders, log=lambda *_: None)
    # six rows: an allowance of six errors accepts every round, so the loop is decided by the budget and the floors -- seven removals
    # chosen by the keys alone leave 23 prototypes in unequal blocks, which the final evaluate() has to digest
    res, before, after = t.prune_prototypes("val", apply=True, budget=7, min_per_class=2, max_extra_errors=6)
    out = res.read()
    assert len(out["order"]) == 7 and not out["stopped"] and m.num_prototypes == 23 and prune.state(m) == sorted(out["order"])
    assert sum(prune.class_counts(m)) == 23 and min(prune.class_counts(m)) >= 2 and not prune.is_balanced(m)
    assert np.isfinite(before["loss"]) and np.isfinite(after["loss"]) and t.Cluster.proto_class.shape[0] == 23
    assert all(s["wrong"] <= out["table"]["wrong_0"] + 6 for s in out["trace"])
    # a refusal: no allowance and a margin that may not drop -- whatever it decides, the result and both evaluations come back
    res2, before2, after2 = t.prune_prototypes("val", apply=True, budget=3, min_per_class=2, max_extra_errors=0, margin_fraction=1.0)
    out2 = res2.read()
    assert m.num_prototypes == 23 - len(out2["order"]) and before2["loss"] == pytest.approx(after["loss"], rel=1e-6) and np.isfinite(after2["loss"])
    after = after2
    assert t.evaluate("val")["loss"] == pytest.approx(after["loss"], rel=1e-6)
    with pytest.raises(ValueError, match="acceptance test off"):
        t.prune_prototypes("val", keep_per_class=2, max_extra_errors=1)

# ---- two gloo ranks on one card: every rank computes what one process computes over the union of the shards --------------------------------
def _shards():
    g = torch.Generator().manual_seed(5)

    def batch(B, tag):
        return {"cine": torch.randn(B, 3, 2, 6, 6, generator=g), "target_AS": torch.arange(B) % 3, "filename": [f"{tag}_{i}" for i in range(B)]}

    return [[batch(4, "r0b0"), batch(4, "r0b1"), batch(3, "r0b2")], [batch(4, "r1b0"), batch(2, "r1b1")]]  # 11 and 6 rows: rank 1 is padded


def _prune_run(rank, world, loader):
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG, Toy

    cfg = {"abstain_class": True, "save_dir": "", "train": TRAIN_CFG}
    t = DPTrainer(Toy(P=40, K=4).to(DEV), cfg, {"train": loader, "test": loader}, rank=rank, world_size=world, log=lambda *_: None)
    out = t.prune_prototypes("test", keep_per_class=7).read()
    return {"removed": out["removed"], "trace_wrong": out["trace_wrong"], "trace_margin": out["trace_margin"], "kept": out["kept"],
            "wrong_0": out["table"]["wrong_0"], "margin_sum": out["table"]["margin_sum"]}


def _prune_worker(rank, world, out_dir):
    # (a file rendezvous: no port to find, release and hope to get back)
    dist.init_process_group("gloo", init_method=f"file://{os.path.join(out_dir, 'rendezvous')}", rank=rank, world_size=world)
    torch.save(_prune_run(rank, world, _shards()[rank]), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_gather_their_rows_and_compute_the_same_result(tmp_path):
    mp.spawn(_prune_worker, args=(2, str(tmp_path)), nprocs=2, join=True)
    shards = _shards()
    one = _prune_run(0, 1, shards[0] + shards[1])
    assert len(one["removed"]) == 9 and min(one["removed"]) >= 0 and len(one["kept"]) == 31
    for r in range(2):
        res = torch.load(tmp_path / f"rank{r}.pt", weights_only=False)
        assert res["removed"] == one["removed"] and res["kept"] == one["kept"] and res["wrong_0"] == one["wrong_0"], r
        assert np.array_equal(res["trace_wrong"], one["trace_wrong"])
        # the padding rows carry no label and all rows share one chunk: the sums are the same additions in the same order
        assert np.array_equal(_bits(res["trace_margin"]), _bits(one["trace_margin"])) and np.array_equal(_bits(res["margin_sum"]), _bits(one["margin_sum"]))
