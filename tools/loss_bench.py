#!/usr/bin/env python3
"""The fused loss criterion (csrc/proto_loss.hip, losses.FusedCriterion) against the eager classes of losses.py, on one GPU.

    python tools/loss_bench.py [--reps 200] [--step-blocks 4 --step-steps 8] [--out profiles/loss_bench.jsonl]
    python tools/loss_bench.py --trace fused|eager [--reps 20]     # criterion calls only, for rocprofv3 --kernel-trace --stats

At the shapes of BASELINE config 3 (N = 32 clips, P = 40 prototypes, K = 4 logits with the abstain class, maps 16 x 7 x 7, D = 256):

1. the criterion alone, forward + backward, fused vs eager: device time (events around the call, median) and host wall time per call
   (a loop of calls ended by one synchronise), for fp32 and bf16 maps, at the shipped recipe weights (Ours_ProtoASNet_Video.yml:31-58:
   orthogonality and map norm off) and with every weight non-zero;
2. the whole training step of tools/train_bench.py --loss reference (X3D-S, 32 x 3 x 16 x 224 x 224 bf16, the paired transform pass, Adam)
   with the criterion fused and eager, alternating blocks of steps on ONE model in one process (A B A B ...): the spread of the blocks of
   one kind is the yardstick for the difference between the kinds;
3. the launches per criterion call of both paths, counted by the torch profiler (kernels between the call's first and last launch).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import losses as L  # noqa: E402

N, P, K, D, MAP = 32, 40, 4, 256, (16, 7, 7)


def recipe(identity, live):
    """The seven objects at the shipped video weights (abstain_class: True); ``live``: orthogonality and map norm switched on too."""
    return (L.CeLossAbstain(loss_weight=1, ab_weight=0.3, ab_logitpath="joined", reduction="mean"), L.ClusterRoiFeat(0.8, K, "mean"),
            L.SeparationRoiFeat(0.08, K, "mean", abstain_class=True), L.OrthogonalityLoss(0.01 if live else 0.0, K, "per_class"),
            L.L_norm(p=2, loss_weight=1e-4 if live else 0.0, reduction="mean"), None, L.L_norm(p=1, loss_weight=1e-4, mask=1 - torch.t(identity)))


def criterion_inputs(map_dtype, dev):
    g = torch.Generator().manual_seed(0)
    identity = torch.zeros(P, K)
    identity[torch.arange(P), torch.arange(P) // (P // K)] = 1
    t = {"logit": torch.randn(N, K, generator=g), "scores": torch.rand(N, P, generator=g), "protos": torch.rand(P, D, 1, 1, 1, generator=g),
         "occ": (torch.rand((N, P, 1) + MAP, generator=g)).to(map_dtype), "fc_w": torch.randn(K, P, generator=g) * 0.5}
    t = {k: v.to(dev).requires_grad_() for k, v in t.items()}
    t["target"] = torch.randint(0, K - 1, (N,), generator=g).to(dev)
    return t, identity


def make_calls(t, identity, live):
    objs = recipe(identity, live)
    fused = L.FusedCriterion(*objs)
    ce, cluster, sep, ortho, lmap, _, lfc = objs
    leaves = [t[k] for k in ("logit", "scores", "protos", "occ", "fc_w")]

    def clear():
        for x in leaves:
            x.grad = None

    def run_fused():
        clear()
        loss, _ = fused.compute(t["logit"], t["scores"], t["occ"], t["protos"], t["fc_w"], t["target"])
        loss.backward()

    def run_eager():
        clear()
        terms = [ce.compute(logits=t["logit"], target=t["target"]), cluster.compute(t["scores"], t["target"]), sep.compute(t["scores"], t["target"]),
                 ortho.compute(t["protos"]), lmap.compute(t["occ"], dim=(-3, -2, -1)), torch.zeros((), device=t["logit"].device),
                 lfc.compute(t["fc_w"])]
        loss = sum(terms)
        torch.stack([x.detach().float().reshape(()) for x in terms])  # the trainer's epoch statistics of the eager path
        loss.backward()

    return run_fused, run_eager


def device_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def host_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def launches(fn):
    """(all kernel launches, library launches) of one call, from the torch profiler's device events."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
    return len(names), sum("pasn" in n for n in names)  # (a bf16 instance keeps its mangled name)


def step_ab(blocks, steps, dev):
    """tools/train_bench.py --loss reference's step with the criterion eager (A) and fused (B), alternating blocks on one model."""
    from protoasnet_amd import model_builder, synth

    cfg = dict(checkpoint_path="", name="Video_XProtoNet", base_architecture="x3d_s", backbone_last_layer_num=-3, pretrained=False,
               prototype_shape="(30, 256, 1, 1, 1)", num_classes=3, img_size=224)
    model = model_builder.build(cfg)
    synth.load_synth(model)
    model = model.to(dev).train().set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips((32, 3, 16, 224, 224)).to(dev).to(torch.bfloat16)
    labels = torch.randint(0, 3, (32,), generator=torch.Generator().manual_seed(0)).to(dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    ce, cluster = L.CeLoss(loss_weight=1, reduction="mean"), L.ClusterRoiFeat(loss_weight=0.8, num_classes=3, reduction="mean")
    separation = L.SeparationRoiFeat(loss_weight=0.08, num_classes=3, reduction="mean", abstain_class=False)
    trans = L.TransformLoss(loss_weight=1e-3, reduction="mean")
    fc_l1 = L.L_norm(mask=1 - torch.t(model.prototype_class_identity), p=1, loss_weight=1e-4)
    fused = L.FusedCriterion(ce, cluster, separation, None, None, trans, fc_l1)
    random.seed(1234)

    def step(use_fused):
        opt.zero_grad(set_to_none=True)
        (logits, sim, occ), t_loss = trans.paired_forward(x, model)
        if use_fused:
            loss, _ = fused.compute(logits, sim, occ, model.prototype_vectors, model.last_layer.weight, labels, transform_term=t_loss)
        else:
            loss = (ce.compute(logits, labels) + cluster.compute(sim, labels) + separation.compute(sim, labels) + t_loss
                    + fc_l1.compute(model.last_layer.weight))
        loss.backward()
        opt.step()

    for f in (False, True, False, True):
        step(f)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for b in range(2 * blocks):
        f = bool(b & 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(f)
        torch.cuda.synchronize()
        ms[f].append((time.perf_counter() - t0) / steps * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-blocks", type=int, default=4, help="blocks of each kind in the whole-step A/B (0: skip it)")
    ap.add_argument("--step-steps", type=int, default=8)
    ap.add_argument("--trace", default="", choices=["", "fused", "eager"], help="only run the criterion --reps times (under a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name()
    if a.trace:
        t, identity = criterion_inputs(torch.float32, dev)
        fn = make_calls(t, identity, True)[0 if a.trace == "fused" else 1]
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"trace": a.trace, "criterion_calls": a.reps, "weights": "all"}))
        return
    rows = []
    for map_dtype in (torch.float32, torch.bfloat16):
        for live in (False, True):
            t, identity = criterion_inputs(map_dtype, dev)
            run_fused, run_eager = make_calls(t, identity, live)
            row = {"bench": "criterion fwd+bwd", "N": N, "P": P, "K": K, "map": list(MAP), "map_dtype": str(map_dtype).split(".")[1],
                   "weights": "all" if live else "shipped", "reps": a.reps, "device": name}
            for tag, fn in (("eager", run_eager), ("fused", run_fused)):
                n_all, n_lib = launches(fn)
                row[tag] = {"device_us": round(device_us(fn, a.reps), 1), "host_us_per_call": round(host_us(fn, a.reps), 1), "launches": n_all,
                            "library_launches": n_lib}
            rows.append(row)
    if a.step_blocks > 0:
        ms = step_ab(a.step_blocks, a.step_steps, dev)
        rows.append({"bench": "training step A/B (train_bench.py --loss reference recipe, X3D-S 32x3x16x224x224 bf16, Adam)",
                     "steps_per_block": a.step_steps, "eager_ms_per_step_blocks": [round(v, 2) for v in ms[False]],
                     "fused_ms_per_step_blocks": [round(v, 2) for v in ms[True]], "eager_median_ms": round(statistics.median(ms[False]), 2),
                     "fused_median_ms": round(statistics.median(ms[True]), 2),
                     "eager_spread_ms": round(max(ms[False]) - min(ms[False]), 2), "fused_spread_ms": round(max(ms[True]) - min(ms[True]), 2),
                     "device": name})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
