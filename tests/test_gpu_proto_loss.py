"""GPU: the fused loss criterion (csrc/proto_loss.hip under losses.FusedCriterion) against the reference's fixtures, against the eager
classes of losses.py on tensors of the real models, its epoch statistics, the trainer switch and its repeatability.

Gates.  The project's own gates of the loss classes against the reference's fixture (tests/test_cpu_losses.py): loss rtol 1e-6 / atol
1e-7, gradient rtol 1e-5 / atol 1e-7.  Where today's path -- losses.py evaluated by torch on the device -- itself lands further than
that from the expected values, the fused call is allowed 4 x that distance (a factor for a different summation order, nothing else);
``_gate`` applies that rule and logs the expected values' scale, both observed errors and the gate to the file named by
PASN_LOSS_PARITY_TSV (profiles/loss_parity_observed.tsv).  A bf16 gradient is judged after rounding: 2^-8 relative."""
import os
import socket

import numpy as np
import pytest
import torch

from loss_cases import CASES as G6_CASES, make_inputs as g6_inputs
from proto_loss_cases import (BF16_RTOL, CASES, GRAD_ATOL, GRAD_RTOL, LOSS_ATOL, LOSS_RTOL, OUTPUTS, build_losses, eager_terms, make_inputs)
from util import CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gate(name, fused, eager, expected, rtol, atol):
    """fused within atol + rtol |expected| of expected, or within 4 x the largest distance of the eager path from it."""
    f, e, x = (torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).detach().double().cpu() for t in (fused, eager, expected))
    assert f.shape == x.shape, f"{name}: shape {tuple(f.shape)} != {tuple(x.shape)}"
    err_f, err_e = (f - x).abs(), (e - x).abs()
    tol = torch.maximum(atol + rtol * x.abs(), 4.0 * err_e.max())
    log = os.environ.get("PASN_LOSS_PARITY_TSV")
    line = (f"{name}\tmax|expected|={float(x.abs().max()):.3g}\tfused_err={float(err_f.max()):.3g}\teager_device_err={float(err_e.max()):.3g}\t"
            f"gate={atol:.3g}+{rtol:.3g}*|expected| or 4*eager_device_err={4 * float(err_e.max()):.3g}")
    print(line)
    if log:
        with open(log, "a") as fh:
            fh.write(line + "\n")
    bad = err_f > tol
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} off, worst {float((err_f - tol).max()):.3g} over the gate ({line})"


def _dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


# ---- the reference's per-class fixture (tests/golden/g6_losses.npz): only that term's weight non-zero ---------------------------------
def _g6_call(cls_name, kwargs, kind, leaf, target):
    """(FusedCriterion, compute arguments, index of the live term) that evaluates one loss class of tests/loss_cases.py on ``leaf``.
    The fixture's two L_norm cases call ``compute(tensor)`` with ``dim=None``: the norm of the WHOLE tensor, which is the definition of
    the last-layer slot (no mask) -- the maps enter it as a (rows, P) view; for p = 1 the sum of the per-row norms is the same number,
    so that case also runs through the map slot (``l1_sum_rows``)."""
    from protoasnet_amd import losses as L

    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    off = dict(ce=L.CeLoss(0), cluster=L.ClusterRoiFeat(0, 4), separation=L.SeparationRoiFeat(0, 4))
    args = dict(logit=z(6, 5), similarities=z(6, 40), occurrence_map=None, prototype_vectors=None, fc_weight=None, target=target)
    if cls_name in ("CeLoss", "CeLossAbstain"):
        return L.FusedCriterion(**dict(off, ce=getattr(L, cls_name)(**kwargs))), dict(args, logit=leaf), 0
    if cls_name.startswith("Cluster"):
        sep = L.SeparationPatch(0, 4) if cls_name == "ClusterPatch" else off["separation"]
        return L.FusedCriterion(**dict(off, cluster=getattr(L, cls_name)(**kwargs), separation=sep)), dict(args, similarities=leaf), 1
    if cls_name.startswith("Separation"):
        cl = L.ClusterPatch(0, 4) if cls_name == "SeparationPatch" else off["cluster"]
        return L.FusedCriterion(**dict(off, cluster=cl, separation=getattr(L, cls_name)(**kwargs))), dict(args, similarities=leaf), 2
    if cls_name == "OrthogonalityLoss":
        return L.FusedCriterion(**off, orthogonality=L.OrthogonalityLoss(**kwargs)), dict(args, prototype_vectors=leaf), 3
    assert cls_name == "L_norm"
    if kind == "rows":
        return L.FusedCriterion(**off, lnorm_occurrence=L.L_norm(**kwargs)), dict(args, occurrence_map=leaf), 4
    return L.FusedCriterion(**off, lnorm_fc=L.L_norm(**kwargs)), dict(args, fc_weight=leaf.view(-1, 40)), 6


G6 = [(t, c, k, kind) for t, c, k, kind in G6_CASES] + [("l1_sum_rows", "L_norm", dict(G6_CASES[10][2]), "rows")]


@pytest.mark.parametrize("tag,cls_name,kwargs,kind", G6, ids=[c[0] for c in G6])
def test_fused_term_reproduces_the_reference_fixture(golden, tag, cls_name, kwargs, kind):
    from protoasnet_amd import losses as L

    g = golden("g6_losses.npz")
    key = "l1_sum" if tag == "l1_sum_rows" else tag
    inputs = g6_inputs("maps" if kind == "rows" else kind)
    target = (inputs[1] if len(inputs) > 1 else torch.zeros(6, dtype=torch.int64)).to(DEV)
    leaf = inputs[0].to(DEV).requires_grad_()
    crit, args, slot = _g6_call(cls_name, kwargs, kind, leaf, target)
    loss, terms = crit.compute(**args)
    loss.backward()
    others = [j for j in range(7) if j != slot]
    assert torch.equal(terms[others], torch.zeros(6, device=DEV)) and float(loss.detach()) == float(terms[slot])  # a term that is off is exactly 0
    # today's path on the device, for the 4 x rule
    leaf_e = inputs[0].to(DEV).requires_grad_()
    eager = getattr(L, cls_name)(**kwargs).compute(leaf_e, *[a.to(DEV) for a in inputs[1:]])
    eager.backward()
    _gate(f"g6/{tag}/loss", loss, eager, g[key + "_loss"], LOSS_RTOL, LOSS_ATOL)
    _gate(f"g6/{tag}/grad", leaf.grad, leaf_e.grad, g[key + "_grad"], GRAD_RTOL, GRAD_ATOL)


# ---- the whole recipe (tests/golden/g11_loss_recipe.npz) ---------------------------------------------------------------------------
def _fused_recipe(tag, t, transform_term=None, stats=None):
    from protoasnet_amd import losses as L

    objs = build_losses(L, tag)
    crit = L.FusedCriterion(*objs)
    return crit.compute(t["logit"], t["scores"], t["occ"], t["protos"], t["fc_w"], t["target"], transform_term=transform_term, stats=stats)


def _leaves(t):
    return dict(t, **{k: t[k].detach().clone().requires_grad_() for k in OUTPUTS})


def _grads(t):
    return {k: (torch.zeros_like(t[k]) if t[k].grad is None else t[k].grad) for k in OUTPUTS}


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_fused_recipe_reproduces_the_reference_fixture(golden, tag):
    from protoasnet_amd import losses as L

    g = golden("g11_loss_recipe.npz")
    base = _dev(make_inputs(tag))
    t = _leaves(base)
    loss, terms = _fused_recipe(tag, t)
    loss.backward()
    assert t["occ"].grad is None or t["occ"].grad.dtype == t["occ"].dtype  # the map gradient comes in the map's dtype
    e = _leaves(dict(base, occ=base["occ"].float()))  # today's path on the device (a bf16 map enters it as the same values in fp32)
    eterms = eager_terms(build_losses(L, tag), e)
    sum(eterms).backward()
    _gate(f"g11/{tag}/loss", loss, sum(eterms), g[tag + "_loss"], LOSS_RTOL, LOSS_ATOL)
    want = g[tag + "_terms"]
    want7 = np.concatenate([want[:5], [0.0], want[5:]]).astype(np.float32)  # the transform slot sits between the map norm and the last layer
    eager7 = torch.stack([x.detach().float().reshape(()) for x in eterms[:5]] + [torch.zeros((), device=DEV)] + [eterms[5].detach().float().reshape(())])
    _gate(f"g11/{tag}/terms", terms, eager7, want7, LOSS_RTOL, LOSS_ATOL)
    fg, eg = _grads(t), _grads(e)
    for k in OUTPUTS:
        bf16 = k == "occ" and base["occ"].dtype == torch.bfloat16
        _gate(f"g11/{tag}/grad_{k}", fg[k].float(), eg[k], g[f"{tag}_grad_{k}"], BF16_RTOL if bf16 else GRAD_RTOL, GRAD_ATOL)


# ---- against the existing path at model shapes ----------------------------------------------------------------------------------------
def _model_step_tensors(kind):
    """(logit, similarities, occurrence_map) of a train-mode forward of the HIP model, its prototypes and last layer, labels."""
    from protoasnet_amd import synth

    if kind == "video":  # X3D-S at the batch of BASELINE config 3, bf16 compute
        cfg = dict(CFG_VIDEO_X3D, prototype_shape="(40, 256, 1, 1, 1)", num_classes=4)
        m = synth_model(cfg).to(DEV).train().set_compute_dtype(torch.bfloat16)
        x = synth.echo_clips((32, 3, 16, 224, 224)).to(DEV).to(torch.bfloat16)
    else:
        m = synth_model(CFG_XPROTO).to(DEV).train()
        x = synth.echo_clips((8, 3, 224, 224)).to(DEV)
    logit, sim, occ = (o.detach() for o in m(x))  # the training pass (batch statistics), its graph dropped
    n = logit.shape[0]
    target = (torch.arange(n) * 7 % 3).to(DEV)
    return dict(logit=logit.clone(), scores=sim.clone(), occ=occ.clone(), protos=m.prototype_vectors.detach().clone(),
                fc_w=m.last_layer.weight.detach().clone(), target=target, identity=m.prototype_class_identity.detach().cpu())


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,abstain", [("video", True), ("video", False), ("image", True)])
def test_fused_recipe_matches_losses_py_on_model_tensors(kind, abstain):
    """Loss, terms and the gradients that reach the prototypes, the last layer, the logits and the maps, against losses.py on the same
    tensors -- with a tied per-class maximum and an all-zero map row in the batch, every term live and a transform term fed in.  The
    expected values are losses.py in fp64 on the device; the fp32 eager path gives the 4 x distance."""
    from protoasnet_amd import losses as L

    base = _model_step_tensors(kind)
    base["scores"][0, 1] = base["scores"][0, 0] = base["scores"][0, :10].max() + 0.01  # a tie inside class 0: the first index takes it
    base["scores"][1, 12] = base["scores"][1, 17] = base["scores"][1, 10:20].max() + 0.01
    base["occ"][1, 3] = 0.0  # p = 2 norm of an all-zero row: zero gradient
    base["occ"][2, 5, 0, ..., 0] = 0.0  # sign(0) = 0 inside a live row
    K = base["logit"].shape[1]

    def objs(dtype):
        ce = L.CeLossAbstain(1, 0.3, "mean", "joined") if abstain else L.CeLoss(1, "mean")
        return (ce, L.ClusterRoiFeat(0.8, K, "mean"), L.SeparationRoiFeat(0.08, K, "mean", abstain_class=abstain), L.OrthogonalityLoss(0.01, K, "per_class"),
                L.L_norm(p=2, loss_weight=1e-3, reduction="mean"), None, L.L_norm(p=1, loss_weight=1e-4, mask=(1 - torch.t(base["identity"])).to(dtype)))

    trans = torch.tensor(0.0371, device=DEV)
    t = _leaves(base)
    tt = trans.clone().requires_grad_()
    loss, terms = L.FusedCriterion(*objs(torch.float32)).compute(t["logit"], t["scores"], t["occ"], t["protos"], t["fc_w"], t["target"], transform_term=tt)
    (2.0 * loss).backward()  # an upstream gradient that is not 1
    assert float(tt.grad) == 2.0 and float(terms[5]) == float(trans)

    def eager(dtype):
        e = _leaves({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in base.items()})
        et = eager_terms(objs(dtype), e)
        et.insert(5, trans.to(dtype))
        (2.0 * sum(et)).backward()
        return sum(et), torch.stack([x.detach().reshape(()) for x in et]), _grads(e)

    l32, t32, g32 = eager(torch.float32)
    l64, t64, g64 = eager(torch.float64)
    tag = f"model/{kind}/{'abstain' if abstain else 'plain'}"
    _gate(f"{tag}/loss", loss, l32, l64, LOSS_RTOL, LOSS_ATOL)
    _gate(f"{tag}/terms", terms, t32, t64, LOSS_RTOL, LOSS_ATOL)
    fg = _grads(t)
    for k in OUTPUTS:
        _gate(f"{tag}/grad_{k}", fg[k], g32[k], g64[k], GRAD_RTOL, GRAD_ATOL)
    # the conventions, spelled out: the tied maxima route to the first index, the zero row and the zero element get zero
    assert float(fg["scores"][0, 0]) != 0.0 and float(fg["scores"][0, 1]) == 0.0
    assert float(fg["scores"][1, 12]) != 0.0 and float(fg["scores"][1, 17]) == 0.0
    assert float(fg["occ"][1, 3].abs().max()) == 0.0 and float(fg["occ"][2, 5, 0, ..., 0].abs().max()) == 0.0 and float(fg["occ"][2, 5].abs().max()) > 0.0


def test_bf16_maps_get_a_bf16_gradient_of_the_fp32_recipe():
    from protoasnet_amd import losses as L

    base = _dev(make_inputs("ours_video_live"))
    for p, red in ((1, "sum"), (2, "mean")):
        crit = L.FusedCriterion(L.CeLoss(0), L.ClusterRoiFeat(0, 4), L.SeparationRoiFeat(0, 4), lnorm_occurrence=L.L_norm(p=p, loss_weight=1e-2, reduction=red))
        o16 = base["occ"].bfloat16().requires_grad_()
        o32 = o16.detach().float().requires_grad_()
        out = []
        for o in (o16, o32):
            loss, _ = crit.compute(base["logit"], base["scores"], o, None, None, base["target"])
            loss.backward()
            out.append(float(loss.detach()))
        assert out[0] == out[1] and o16.grad.dtype == torch.bfloat16
        assert torch.equal(o16.grad, o32.grad.bfloat16())  # the same fp32 gradient, rounded once


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ours_video_live", "baseline_video_live"])
def test_epoch_statistics_equal_the_bincount_and_stack_path(tag):
    from protoasnet_amd import losses as L

    abstain = next(c for c in CASES if c[0] == tag)[2]
    base = _dev(make_inputs(tag))
    K = base["logit"].shape[1] - (1 if abstain else 0)
    cm = torch.zeros(K * K, dtype=torch.int64, device=DEV)
    loss_sum = torch.zeros(7, dtype=torch.float32, device=DEV)
    cm_e, sum_e, sum_64 = torch.zeros_like(cm), torch.zeros_like(loss_sum), torch.zeros(7, dtype=torch.float64, device=DEV)
    g = torch.Generator().manual_seed(5)
    for b in range(3):
        t = dict(base, logit=torch.randn(base["logit"].shape, generator=g).to(DEV), scores=torch.rand(base["scores"].shape, generator=g).to(DEV),
                 target=torch.randint(0, K, (base["logit"].shape[0],), generator=g).to(DEV))
        if b == 1:
            t["logit"][0, :K] = 0.25  # every real class ties: the lowest index is the prediction
        with torch.no_grad():
            _, terms = _fused_recipe(tag, t, stats=(cm, loss_sum))
            et = eager_terms(build_losses(L, tag), t)
            e64 = eager_terms(build_losses(L, tag), {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()})
        cm_e += torch.bincount(t["target"].clamp(0, K - 1) * K + t["logit"][:, :K].argmax(dim=1), minlength=K * K)
        for dst, src in ((sum_e, et), (sum_64, e64)):
            dst += torch.stack([x.detach().to(dst.dtype).reshape(()) for x in src[:5]] + [torch.zeros((), device=DEV, dtype=dst.dtype), src[5].detach().to(dst.dtype).reshape(())])
        assert float(terms.sum()) != 0.0
    assert torch.equal(cm, cm_e) and int(cm.sum()) == 3 * base["logit"].shape[0]
    _gate(f"stats/{tag}/loss_sum", loss_sum, sum_e, sum_64, LOSS_RTOL, LOSS_ATOL)
    # labels outside [0, K) are clamped into the matrix, as target.clamp(0, K - 1) does today (counts only: the eager losses refuse such labels)
    wild = torch.tensor([-3, K, K + 5, 0, 1], device=DEV)
    before = cm.clone()
    with torch.no_grad():
        _fused_recipe(tag, dict(base, target=wild), stats=(cm, loss_sum))
    want = torch.bincount(wild.clamp(0, K - 1) * K + base["logit"][:, :K].argmax(dim=1), minlength=K * K)
    assert torch.equal(cm - before, want)


def test_argument_errors_are_status_codes_with_text():
    from protoasnet_amd import losses as L

    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    t = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="divisible"):  # 10 prototypes do not split into 4 classes
        L.FusedCriterion(L.CeLoss(1), L.ClusterRoiFeat(0.8, 4), L.SeparationRoiFeat(0.08, 4)).compute(z(2, 4), z(2, 10), None, None, None, t)
    with pytest.raises(ValueError, match=">= 2 classes not including abstention"):
        L.FusedCriterion(L.CeLossAbstain(1), L.ClusterRoiFeat(0.8, 2), L.SeparationRoiFeat(0.08, 2)).compute(z(2, 2), z(2, 4), None, None, None, t)
    from protoasnet_amd import _lib
    import ctypes

    d = _lib.ProtoLossDesc(N=2, K=4, K_real=4, P=8, C=4, ce_reduction=2, w_ce=1.0)
    out = z(8)
    rc = _lib.lib().pasn_proto_loss_fwd(z(2, 4).data_ptr(), 0, t.data_ptr(), 0, 0, 0, 0, 0, out.data_ptr(), out[7:].data_ptr(), 0, 0, 0, ctypes.byref(d), 0)
    assert rc == 1 and b"unknown reduction" in _lib.lib().pasn_last_error()
    d = _lib.ProtoLossDesc(N=2, K=4, K_real=4, P=8, C=4, S=9, map_p=3, w_map=1.0, map_reduction=1)
    rc = _lib.lib().pasn_proto_loss_fwd(0, 0, 0, 0, z(2, 8, 9).data_ptr(), 0, 0, 0, out.data_ptr(), out[7:].data_ptr(), z(32).data_ptr(), 0, 0, ctypes.byref(d), 0)
    assert rc == 1 and b"p = 1 and p = 2" in _lib.lib().pasn_last_error()


# ---- repeatability ------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal():
    base = _dev(make_inputs("other_norms"))
    runs = []
    for _ in range(2):
        t = _leaves(base)
        cm, ls = torch.zeros(9, dtype=torch.int64, device=DEV), torch.zeros(7, device=DEV)
        loss, terms = _fused_recipe("other_norms", t, stats=(cm, ls))
        loss.backward()
        runs.append([loss.detach(), terms, cm, ls] + [_grads(t)[k] for k in OUTPUTS])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- trainer ------------------------------------------------------------------------------------------------------------------------
def _loader(n, seed, B=2):
    from protoasnet_amd import synth

    class Batches(list):
        batch_size = B

    return Batches({"cine": synth.echo_clips((B, 3, 4, 64, 64), seed=seed + b), "target_AS": (torch.arange(B) + b) % 3,
                    "filename": [f"c{b}_{i}" for i in range(B)]} for b in range(n))


def _train_cfg(fused, abstain, **over):
    from test_cpu_trainer import TRAIN_CFG

    tc = dict(TRAIN_CFG, num_train_epochs=2, num_warm_epochs=99, push_start=99, accumulation_steps=2, save=False, fused_loss=fused,
              optimizer={"name": "SGD", "mode": "lr_same", "lr_same": 2e-3})
    tc["criterion"] = dict(tc["criterion"], trans_occurrence={"loss_weight": 1e-3, "reduction": "mean"})
    tc.update(over)
    return {"abstain_class": abstain, "save_dir": None, "train": tc}


def _run_trainer(fused, abstain, epochs, **over):
    import random

    from protoasnet_amd.trainer import DPTrainer

    from test_gpu_trainer import _kink_sparse

    random.seed(77)  # the affine configurations of the transform term
    # the model of test_gpu_trainer.py's parity test, prepared as there ("Training parity and ReLU kinks"): on the plain synthetic
    # weights half of the ReLU units sit at their kink, and two runs of the EAGER trainer from one seed land 1e-4 ... 4e-3 apart in the second
    # epoch's terms (measured; also with PASN_WGRAD_DET=1) -- a comparison there compares noise.  Prepared: 2.4e-7 at most over two epochs.
    m = _kink_sparse(synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)") if abstain else CFG_VIDEO_X3D)).to(DEV)
    p0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    t = DPTrainer(m, _train_cfg(fused, abstain, **over), {"train": _loader(4, 10), "val": _loader(2, 50)}, log=lambda *_: None)
    assert (t.fused is not None) == fused
    hist = []
    for e in range(epochs):
        hist.append((t.run_epoch(e, "train"), t.run_epoch(e, "val")))
    return hist, p0, {k: v.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("abstain,two_pass", [(False, False), (True, False), (False, True)])
def test_trainer_with_the_fused_criterion_follows_the_eager_trainer(monkeypatch, abstain, two_pass):
    """Two epochs (train + val) from the same seed with ``train.fused_loss`` on and off, the transform term live on each of its routes
    (the paired training pass, the second pass under PASN_NO_TRAIN_PAIR=1, ``compute_from_maps`` in the validation epochs): the same
    keys, equal confusion-matrix metrics, loss terms within the gate.  Today's path runs twice, for the 4 x rule."""
    if two_pass:
        monkeypatch.setenv("PASN_NO_TRAIN_PAIR", "1")
    on, off, again = (_run_trainer(f, abstain, 2)[0] for f in (True, False, False))
    for e in range(2):
        for a, b, b2, mode in zip(on[e], off[e], again[e], ("train", "val")):
            assert sorted(a) == sorted(b), (e, mode)
            assert a["f1"] == b["f1"] and a["accuracy"] == b["accuracy"], (e, mode, a["f1"], b["f1"])
            name = f"trainer/{'abstain' if abstain else 'plain'}{'/two_pass' if two_pass else ''}/epoch{e}/{mode}"
            f, x, x2 = (torch.tensor(d["loss_terms"], dtype=torch.float64) for d in (a, b, b2))
            _gate(name + "/loss_terms", f, x2, x, LOSS_RTOL, LOSS_ATOL)
            assert a["loss_terms"][5] != 0.0


@pytest.mark.timeout(900)
def test_one_sgd_step_agrees_within_the_gradient_gate_times_the_learning_rate():
    """One optimizer step of two micro-batches: the parameter updates of the two paths agree within the gradient gate scaled by the
    learning rate, each tensor against its own scale, above the floor fp32 storage of the parameter sets (one rounding of p per path)."""
    lr = 2e-3
    (_, p0, p_on), (_, _, p_off) = (_run_trainer(f, False, 1, accumulation_steps=4) for f in (True, False))
    moved = 0
    for k, v0 in p0.items():
        du_on, du_off = p_on[k] - v0, p_off[k] - v0
        scale = float(du_off.abs().max())
        moved += scale > 0
        tol = GRAD_RTOL * scale + lr * GRAD_ATOL + 2 * 2.0 ** -24 * float(v0.abs().max())
        err = float((du_on - du_off).abs().max())
        assert err <= tol, f"{k}: updates differ by {err:.3g} > {tol:.3g} (largest update {scale:.3g})"
    assert moved > 10


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, out_dir):
    import sys

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from protoasnet_amd.trainer import DPTrainer
    from test_gpu_trainer import _kink_sparse

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for fused in (True, False):
        m = _kink_sparse(synth_model(CFG_VIDEO_X3D)).to(torch.device("cuda", 0))
        cfg = _train_cfg(fused, False)
        cfg["train"]["criterion"] = dict(cfg["train"]["criterion"], trans_occurrence={"loss_weight": 0.0, "reduction": "mean"})
        every = _loader(4, 10)
        t = DPTrainer(m, cfg, {"train": every[rank::world], "val": every[:2]}, rank=rank, world_size=world, log=lambda *_: None)
        out[fused] = (t.run_epoch(0, "train"), t.run_epoch(0, "val"))
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_rank_gloo_rehearsal_with_the_fused_criterion(tmp_path):
    """Two ranks on the one card over gloo: the launch-made confusion matrix and term sums ride in the epoch's all-reduce as the eager
    ones do -- every rank reports the global metrics, equal to the eager trainer's."""
    import torch.multiprocessing as mp

    world, port = 2, _free_port()
    mp.spawn(_rank_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    outs = [torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(world)]
    for i, mode in enumerate(("train", "val")):
        a0, a1, b0 = outs[0][True][i], outs[1][True][i], outs[0][False][i]
        assert sorted(a0) == sorted(b0)
        assert a0["f1"] == a1["f1"] == b0["f1"] and a0["accuracy"] == b0["accuracy"]
        assert a0["loss_terms"] == a1["loss_terms"]
        want = torch.tensor(b0["loss_terms"], dtype=torch.float64)
        _gate(f"gloo/{mode}/loss_terms", torch.tensor(a0["loss_terms"], dtype=torch.float64), want, want, LOSS_RTOL, LOSS_ATOL)
