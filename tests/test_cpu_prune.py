"""CPU: the restatement of the pruning definitions (prune_cases.py) against a brute-force recomputation, the model surgery on the three
model classes, the checkpoint key, and the refusals of an unbalanced model."""
import numpy as np
import pytest
import torch

import prune_cases as pc
from test_cpu_trainer import TRAIN_CFG
from util import CFG_PUSH_PPNET, CFG_PUSH_XIMG, CFG_VIDEO_X3D


# ---- the restatement against brute force: dyadic inputs, every fp64 sum exact -----------------------------------------------------------
@pytest.mark.parametrize("M,P,K,K_real,chunk,kw", [
    (37, 8, 3, 2, 16, dict(g=1)),                                    # abstention column and prototypes present, several chunks
    (50, 12, 4, 4, 16, dict(g=2)),
    (41, 12, 3, 3, 128, dict(accept=True, informative=0.75)),        # the acceptance test decides
    (29, 9, 3, 3, 8, dict(accept=True, margin_fraction=0.5, max_extra=3)),
])
def test_restatement_equals_in_order_recomputation_on_dyadic_inputs(M, P, K, K_real, chunk, kw):
    sim, w, labels, cls = pc.make_case(M, P, K, K_real, seed=M + P, dyadic=True, unlabeled=0.2, informative=kw.get("informative", 0.0))
    assert np.all(sim * 8 == np.round(sim * 8)) and np.all(w * 8 == np.round(w * 8)) and np.abs(w).max() <= 2 and np.abs(sim).max() <= 1
    floors = pc.floors_for(K_real, kw.get("g", 1))
    rounds = pc.rounds_for(cls, K_real, floors)
    args = (sim, w, labels, K_real, cls, rounds, floors, kw.get("accept", False), kw.get("max_extra", 0), kw.get("margin_fraction"))
    a, b = pc.eliminate(*args, chunk=chunk), pc.eliminate(*args, chunk=chunk, brute=True)
    for x, y in zip(a["table"], b["table"]):
        assert np.array_equal(x, y)  # tallies as integers, margin sums bit for bit
    assert np.array_equal(a["removed"], b["removed"]) and np.array_equal(a["kept"], b["kept"])
    assert np.array_equal(a["trace_wrong"], b["trace_wrong"]) and np.array_equal(a["trace_margin"], b["trace_margin"])
    assert np.array_equal(a["z"], b["z"])  # the subtract chain IS the recomputation here
    if not kw.get("accept"):
        assert (a["removed"] >= 0).all() and len(set(a["removed"])) == rounds
        kept_cls = np.bincount(cls[a["kept"] == 1], minlength=K)
        assert kept_cls[:K_real].tolist() == floors and (kept_cls[K_real:] == np.bincount(cls, minlength=K)[K_real:]).all()
    # the order of the chunk cut is part of the definition but, with exact sums, not of the value
    c = pc.eliminate(*args, chunk=5)
    assert np.array_equal(a["removed"], c["removed"]) and np.array_equal(a["trace_margin"], c["trace_margin"])


def test_restatement_hand_case():
    """Two classes, three prototypes, worked by hand: prototype 1 carries class 0, prototypes 0 and 2 are redundant."""
    sim = np.array([[0.5, 1.0, 0.25], [0.5, 0.0, 1.0], [0.5, 0.75, 0.5], [0.25, 0.25, 0.25]], np.float32)
    w = np.array([[0.5, 1.0, 0.0], [0.5, 0.0, 1.0]], np.float32)
    labels = np.array([0, 1, 0, -1], np.int32)
    cls = np.array([0, 0, 1], np.int32)
    z = pc.base_logits(sim, w, [1, 1, 1], 2)
    assert z.tolist() == [[1.25, 0.5], [0.25, 1.25], [1.0, 0.75], [0.375, 0.375]]
    wrong, flips, per, ms = pc.round_table(z, sim, w, labels, [1, 1, 1], 2, chunk=2)
    assert wrong.tolist() == [0, 2, 1, 0] and flips.tolist() == [0, 2, 1, 0]  # (the unlabelled row counts nowhere)
    assert per.tolist() == [[0, 0], [2, 0], [0, 1], [0, 0]]
    assert ms.tolist() == [2.0, 0.25, 1.75, 2.0]  # removing prototype 0 moves both logits alike
    # without prototype 1, row 0 is (0.25, 0.5): wrong; without prototype 2, row 1 is (0.25, 0.25): a tie, class 0 wins, wrong
    r = pc.eliminate(sim, w, labels, 2, cls, 1, [1, 1], True)
    assert r["removed"].tolist() == [0] and r["trace_wrong"].tolist() == [[0, 0, 0]] and r["kept"].tolist() == [0, 1, 1]
    r = pc.eliminate(sim, w, labels, 2, cls, 1, [2, 1], True)  # class 0 stands at its floor, class 1 as well: nothing to remove
    assert r["removed"].tolist() == [-1] and r["trace_margin"].tolist() == [2.0]


def test_restatement_ties_and_stop():
    sim, w, labels, _ = pc.make_case(60, 8, 2, 2, seed=3, dyadic=True)
    sim[:, 5], w[:, 5] = sim[:, 4], w[:, 4]  # two identical prototypes: equal keys, the lower index goes first
    sim[::7] = 0  # rows whose logits are all equal: the lowest class is predicted
    cls = np.array([0, 0, 0, 0, 1, 1, 0, 0], np.int32)  # the two copies are class 1; class 0 stands at its floor: they alone are candidates
    r = pc.eliminate(sim, w, labels, 2, cls, 1, [6, 1], False)
    assert r["removed"].tolist() == [4]
    tab = r["table"]
    assert tab[0][4] == tab[0][5] and tab[3][4] == tab[3][5]
    z = pc.base_logits(sim, w, np.ones(8), 2)
    assert (z[::7, 0] == z[::7, 1]).all() and labels[7] == 1 and tab[2][8, 1] >= 1  # ... and a tied row of class 1 counts as wrong
    # a model that is right on every row, with redundant prototypes: removals are accepted until one costs an error, then nothing more
    case = pc.make_case(2 * pc.CHUNK + 40, 16, 4, 4, seed=2, unlabeled=0.05, informative=0.6)
    s = pc.eliminate(*case[:3], 4, case[3], 12, [1, 1, 1, 1], True, 0, None)
    assert s["removed"].tolist() == [4, 3, 11, 15, 7, 0, 12, 8, -1, -1, -1, -1]  # (as drawn; the GPU test runs the same case)
    assert s["table"][0][16] == 0 and (s["trace_wrong"][:, 0] == 0).all() and (s["trace_margin"][8:] == s["trace_margin"][8]).all()
    t = pc.eliminate(*case[:3], 4, case[3], 12, [1, 1, 1, 1], True, 0, None, brute=True)
    assert (t["removed"][8:] == -1).all() and (t["removed"][:8] >= 0).all()  # the in-order recomputation stops at the same round


def test_class_grouped_losses_follow_the_class_identity_of_unequal_blocks():
    """The costs that group prototypes by class, on [7, 10, 10] (27 divides by 3: a reshape would mis-index silently) and on [2, 3, 3]
    of 8 (does not divide), against loops over each class's own prototypes."""
    from protoasnet_amd import losses

    g = torch.Generator().manual_seed(0)
    for counts in ([7, 10, 10], [2, 3, 3], [4, 0, 2]):
        K, P = len(counts), sum(counts)
        cls = torch.repeat_interleave(torch.arange(K), torch.tensor(counts))
        sims, target = torch.rand(5, P, generator=g), torch.tensor([0, 1, 2, 1, 0])
        protos = torch.randn(P, 6, 1, 1, 1, generator=g)
        best = torch.stack([sims[:, cls == k].max(dim=1)[0] if counts[k] else torch.zeros(5) for k in range(K)], dim=1)
        worst = torch.stack([sims[:, cls == k].min(dim=1)[0] if counts[k] else torch.zeros(5) for k in range(K)], dim=1)
        own = torch.nn.functional.one_hot(target, K)
        c, s, o = losses.ClusterRoiFeat(0.8, K, "sum"), losses.SeparationRoiFeat(0.08, K, "sum", abstain_class=False), losses.OrthogonalityLoss(0.01, K)
        cp = losses.ClusterPatch(0.5, K, "sum")
        for obj in (c, s, o, cp):
            obj.proto_class = cls
        assert torch.allclose(c.compute(sims, target), -0.8 * (best * own).sum(), rtol=1e-6, atol=0)
        assert torch.allclose(s.compute(sims, target), 0.08 * (best * (1 - own)).sum(), rtol=1e-6, atol=0)
        assert torch.allclose(cp.compute(sims, target), 0.5 * (worst * own).sum(), rtol=1e-6, atol=0)
        p2 = torch.nn.functional.normalize(protos.flatten(1), dim=1)
        want = sum(float(p2[i] @ p2[j]) for i in range(P) for j in range(i + 1, P) if cls[i] == cls[j])
        assert float(o.compute(protos)) == pytest.approx(0.01 * want, rel=1e-5, abs=1e-7)
        with pytest.raises(ValueError, match="rebuild the criterion after pruning"):
            c.compute(sims[:, :-1], target)
    # equal blocks: the grouping by identity IS the reshape
    cls = torch.repeat_interleave(torch.arange(3), 4)
    sims, target = torch.rand(5, 12, generator=g), torch.tensor([0, 1, 2, 1, 0])
    a, b = losses.ClusterRoiFeat(0.8, 3, "mean"), losses.ClusterRoiFeat(0.8, 3, "mean")
    b.proto_class = cls
    assert torch.equal(a.compute(sims, target), b.compute(sims, target))


# ---- the surgery --------------------------------------------------------------------------------------------------------------------------
def _build(cfg):
    from protoasnet_amd import model_builder

    torch.manual_seed(0)
    return model_builder.build(cfg).eval()


@pytest.mark.parametrize("cfg,remove", [(CFG_PUSH_PPNET, [1, 4]), (CFG_PUSH_XIMG, [0, 5, 11]), (CFG_VIDEO_X3D, [3, 4, 17, 29])],
                         ids=["PPNet", "XProtoNet", "Video_XProtoNet"])
def test_surgery_slices_every_tensor_and_round_trips_through_a_checkpoint(cfg, remove):
    from protoasnet_amd import prune

    m = _build(cfg)
    P, K = m.num_prototypes, m.num_classes
    head_b = hasattr(m, "occurrence_module")
    with torch.no_grad():
        m.last_layer.weight.copy_(torch.arange(K * P, dtype=torch.float32).view(K, P))
        m.prototype_vectors.copy_(torch.arange(P, dtype=torch.float32).view((P,) + (1,) * (m.prototype_vectors.dim() - 1)).expand_as(m.prototype_vectors))
        if head_b:
            oc = m.occurrence_module.convs()[-1]
            oc.weight.copy_(torch.arange(P, dtype=torch.float32).view((P,) + (1,) * (oc.weight.dim() - 1)).expand_as(oc.weight))
    ident = m.prototype_class_identity.clone()
    tail = tuple(m.prototype_vectors.shape[1:])
    assert prune.state(m) == []
    keep = prune.apply(m, remove)
    assert keep == [p for p in range(P) if p not in remove]
    Q = len(keep)
    assert m.num_prototypes == Q and list(m.prototype_shape) == [Q] + list(tail)
    assert tuple(m.prototype_vectors.shape) == (Q,) + tail and tuple(m.ones.shape) == (Q,) + tail and not m.ones.requires_grad
    assert m.prototype_vectors.requires_grad and m.prototype_vectors.flatten(1)[:, 0].tolist() == [float(p) for p in keep]
    assert tuple(m.last_layer.weight.shape) == (K, Q) and m.last_layer.in_features == Q
    assert torch.equal(m.last_layer.weight.detach(), torch.arange(K * P, dtype=torch.float32).view(K, P)[:, keep])
    assert torch.equal(m.prototype_class_identity, ident[keep])  # the rows that remain, in order
    if head_b:
        oc = m.occurrence_module.convs()[-1]
        assert oc.weight.shape[0] == Q and oc.out_channels == Q and oc.bias is None and oc.weight.is_contiguous()
        assert oc.weight.flatten(1)[:, 0].tolist() == [float(p) for p in keep]
        assert m.last_layer.weight.is_contiguous()
    # a second removal is relative to the model as it stands; the state is relative to the model as built
    prune.apply(m, [0])
    removed = sorted(remove + [keep[0]])
    assert prune.state(m) == removed
    m2 = _build(cfg)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m2.load_state_dict(m.state_dict())
    prune.restore(m2, removed)
    m2.load_state_dict(m.state_dict())
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert torch.equal(m2.prototype_class_identity, m.prototype_class_identity) and prune.state(m2) == removed
    with pytest.raises(ValueError, match="pruned already"):
        prune.restore(m2, [0])
    with pytest.raises(ValueError, match="distinct prototype indices"):
        prune.apply(m, [0, 0])
    with pytest.raises(ValueError, match="at least one prototype"):
        prune.apply(m, list(range(m.num_prototypes)))


def test_reference_call_on_head_b_slices_the_occurrence_module_too():
    m = _build(CFG_PUSH_XIMG)
    m.prune_prototypes([2, 3])  # the reference's method name (ProtoPNet.py): on head B it used to leave the occurrence conv at 12 channels
    assert m.occurrence_module.convs()[-1].weight.shape[0] == 10 == m.num_prototypes == m.last_layer.weight.shape[1]


def test_an_index_out_of_range_does_not_corrupt_the_recorded_state():
    from protoasnet_amd import prune

    m = _build(CFG_PUSH_PPNET)
    m.prune_prototypes([1, 99])  # the reference's method ignores an index the model does not have
    assert m.num_prototypes == 5 and prune.state(m) == [1] and m._built_prototypes == 6


def test_checkpoint_key_is_written_only_for_a_pruned_model_and_applied_on_load(tmp_path):
    from protoasnet_amd import prune
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG, _batches

    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": dict(TRAIN_CFG)}
    b = _batches(3, 2)
    t = DPTrainer(_build(CFG_VIDEO_X3D), cfg, {"train": b, "val": b}, log=lambda *_: None)
    assert "pruned_prototypes" not in t.get_state()
    prune.apply(t.model, [0, 1, 10, 11, 20, 21])
    t._rebuild_after_surgery()
    assert t.Lnorm_fc.mask.shape == (3, 24)
    t.save_checkpoint()
    ck = torch.load(tmp_path / "last.pth")
    assert ck["pruned_prototypes"] == [0, 1, 10, 11, 20, 21] and sorted(ck) == ["epoch", "iteration", "optimizer", "pruned_prototypes", "state_dict"]
    t2 = DPTrainer(_build(CFG_VIDEO_X3D), cfg, {"train": b, "val": b}, log=lambda *_: None)
    assert t2.load_checkpoint(str(tmp_path / "last.pth")) and t2.model.num_prototypes == 24
    for k, v in t.model.state_dict().items():
        assert torch.equal(t2.model.state_dict()[k], v), k
    assert any(p is t2.model.prototype_vectors for g in t2.optimizer.param_groups for p in g["params"])  # the optimizer was rebuilt
    assert t2.load_checkpoint(str(tmp_path / "last.pth"))  # loading again into the already pruned model is the same model


# ---- unequal blocks -------------------------------------------------------------------------------------------------------------------------
def test_unbalanced_model_refuses_training_and_class_reshapes_by_name():
    from protoasnet_amd import losses, prune

    m = _build(CFG_VIDEO_X3D)
    prune.apply(m, [0, 1, 2])  # class 0 keeps 7 prototypes, the others 10: 27 still divides by 3
    assert prune.class_counts(m) == [7, 10, 10]
    m.train()
    with pytest.raises(ValueError, match=r"unbalanced prototype blocks: the classes own \[7, 10, 10\]"):
        m(torch.zeros(1, 3, 4, 64, 64))
    with pytest.raises(ValueError, match="unbalanced prototype blocks"):
        m.compute_occurence_map(torch.zeros(1, 3, 4, 64, 64))
    m.eval()
    with pytest.raises(ValueError, match="unbalanced prototype blocks: 26 prototypes"):
        losses.ClusterRoiFeat(1.0, num_classes=3).compute(torch.zeros(2, 26), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="unbalanced prototype blocks: 26 prototypes"):
        losses.OrthogonalityLoss(1.0, num_classes=3).compute(torch.zeros(26, 4, 1, 1, 1))
    from protoasnet_amd import explain

    with pytest.raises(ValueError, match=r"unbalanced prototype blocks: the classes own \[7, 10, 10\]"):
        explain._dimensions(m, False)  # 27 divides by 3: the real counts are checked, not P % K
    with pytest.raises(ValueError, match="unbalanced prototype blocks"):
        losses.FusedCriterion.from_config(TRAIN_CFG["criterion"], m, False)
    b = _build(CFG_VIDEO_X3D)
    prune.apply(b, [0, 10, 20])
    prune.require_balanced(b, "anything")  # equal blocks pass
    assert explain._dimensions(b, False) == (27, 3, 9, 3)


def test_trainer_criterion_groups_by_class_identity_on_an_unbalanced_model():
    from protoasnet_amd import prune
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import _batches

    m = _build(CFG_VIDEO_X3D)
    b = _batches(3, 2)
    t = DPTrainer(m, {"abstain_class": False, "save_dir": "", "train": dict(TRAIN_CFG)}, {"train": b, "val": b}, log=lambda *_: None)
    assert t.Cluster.proto_class is None and t.Orthogonality.proto_class is None  # the model as built: the reshape, as before
    prune.apply(m, [0, 1, 2])
    t._rebuild_after_surgery()
    assert t.Cluster.proto_class.tolist() == [0] * 7 + [1] * 10 + [2] * 10 and t.Separation.proto_class is t.Orthogonality.proto_class
    sims, target = torch.rand(4, 27), torch.tensor([0, 1, 2, 0])
    got = t.Cluster.compute(sims, target)
    own = torch.nn.functional.one_hot(target, 3)
    best = torch.stack([sims[:, :7].max(1)[0], sims[:, 7:17].max(1)[0], sims[:, 17:].max(1)[0]], 1)
    assert torch.allclose(got, -0.8 * (best * own).mean(dim=0).sum(), rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="unbalanced prototype blocks"):
        DPTrainer(m, {"abstain_class": False, "save_dir": "", "train": dict(TRAIN_CFG, fused_loss=True)}, {"train": b, "val": b}, log=lambda *_: None)


def test_plan_rounds_and_argument_checks():
    from protoasnet_amd import prune

    cls = [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4  # class 3: abstention
    assert prune.plan_rounds(cls, 3, keep_per_class=2) == (6, [2, 2, 2], False)
    assert prune.plan_rounds(cls, 3) == (9, [1, 1, 1], True)
    assert prune.plan_rounds(cls, 3, budget=4, min_per_class=3) == (3, [3, 3, 3], True)
    with pytest.raises(ValueError, match="keep_per_class=5"):
        prune.plan_rounds(cls, 3, keep_per_class=5)
    with pytest.raises(ValueError, match="budget can not be given"):
        prune.plan_rounds(cls, 3, budget=1, keep_per_class=2)
    with pytest.raises(ValueError, match="acceptance test off"):
        prune.eliminate(None, None, None, 3, None, keep_per_class=2, max_extra_errors=1)
    with pytest.raises(ValueError, match="acceptance test off"):
        prune.eliminate(None, None, None, 3, None, keep_per_class=2, margin_fraction=0.9)
    with pytest.raises(RuntimeError, match="GPU only"):
        prune.importance(torch.zeros(4, 3), torch.zeros(2, 3), torch.zeros(4, dtype=torch.int32), 2, torch.zeros(3, dtype=torch.int32))
