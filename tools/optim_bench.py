#!/usr/bin/env python3
"""The library optimizer (csrc/optim.hip, protoasnet_amd/optim.py) against torch on one GPU, the optimizer side of a step alone.

    python tools/optim_bench.py [--reps 100] [--out profiles/optim_bench.jsonl]
    python tools/optim_bench.py --trace adam-torch|adam-flat|accum-none|accum-torch|accum-flat --arch x3d_s [--reps 20]   # under rocprofv3
    python tools/optim_bench.py --stats-summary kernel_stats.csv --baseline kernel_stats_reps0.csv --reps 20   # launches per call of such a run
    bash tools/optim_trace.sh                                                                                   # all of the traced runs

For the parameter lists of the four trunks + heads (X3D-S and R(2+1)D-18[:-3] video models, ResNet-18 XProtoNet and ProtoPNet), as
tensors of the parameters' shapes with N(0, 1) values:

1. ``torch.optim.Adam.step()`` against ``optim.FlatAdam.step()``: device time per step (events around a run of 10 steps, so launch gaps
   count, as they do in training), host wall time per step to enqueue them, launches per step (torch profiler);
2. autograd's accumulation of a second micro-batch against ``GradAccumulator.absorb()``: one backward through a node that hands out its
   gradients as views of one fresh flat buffer with 64-float slots, as the training pass does -- except ``prototype_vectors`` and
   ``last_layer.weight``, which arrive as tensors of their own, as they do when the loss terms add to them -- timed with ``p.grad``
   already set (AccumulateGrad adds per tensor) and with ``p.grad = None`` followed by ``absorb()``; ``accum-none`` is that backward
   alone with its gradients dropped -- the part of both figures that is not accumulation (making 321 views costs more than adding them);
3. ``pasn_adam_step`` on ONE tensor of 2^10 ... 2^26 elements: time per call and 28 bytes per element over it, as a share of the HBM
   peak (8 TB/s).  Up to 2^23 elements the 28 n bytes fit the 256 MiB Infinity Cache, so those rows are not HBM rates.

``--trace`` runs one of the paths ``--reps`` times and nothing else: the launch counts of the log come from
``rocprofv3 --kernel-trace --stats -- python tools/optim_bench.py --trace ...`` runs of their own (no counters in them);
``--stats-summary`` subtracts the kernel_stats.csv of the same run with ``--reps 0`` (the set-up alone) from that of the run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import model_builder, optim  # noqa: E402

HBM_PEAK = 8.0e12
ARCHS = {
    "x3d_s": dict(checkpoint_path="", name="Video_XProtoNet", base_architecture="x3d_s", backbone_last_layer_num=-3, pretrained=False,
                  prototype_shape="(30, 256, 1, 1, 1)", num_classes=3, img_size=224),
    "r2plus1d_18": dict(checkpoint_path="", name="Video_XProtoNet", base_architecture="resnet2p1d_18", backbone_last_layer_num=-3,
                        pretrained=False, prototype_shape="(40, 256, 1, 1, 1)", num_classes=4, img_size=112),
    "resnet18_xprotonet": dict(checkpoint_path="", name="XProtoNet", base_architecture="resnet18", pretrained=False,
                               prototype_shape="(40, 512, 1, 1)", num_classes=4, img_size=224, add_on_layers_type="regular"),
    "resnet18_protopnet": dict(checkpoint_path="", name="ProtoPNet", base_architecture="resnet18", pretrained=False,
                               prototype_shape="(30, 512, 1, 1)", num_classes=3, img_size=224, add_on_layers_type="regular",
                               prototype_activation_function="log"),
}


def parameter_list(arch, dev):
    """(names, parameters on the device) of the model's trainable tensors, N(0, 1) values."""
    model = model_builder.build(ARCHS[arch])
    g = torch.Generator().manual_seed(0)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return [n for n, _ in named], [torch.nn.Parameter(torch.randn(p.shape, generator=g).to(dev)) for _, p in named]


class Emit(torch.autograd.Function):
    """A node whose backward hands out every parameter's gradient the way the training pass does."""

    @staticmethod
    def forward(ctx, own, *params):
        ctx.own, ctx.shapes = own, [p.shape for p in params]
        return params[0].new_zeros(())

    @staticmethod
    def backward(ctx, go):
        offs, o = [], 0
        for s in ctx.shapes:
            offs.append(o)
            o += (s.numel() + 63) // 64 * 64
        G = torch.ones(o, dtype=torch.float32, device=go.device)
        return (None,) + tuple(torch.ones(s, device=go.device) if i in ctx.own else G[f: f + s.numel()].view(s)
                               for i, (s, f) in enumerate(zip(ctx.shapes, offs)))


def timed(fn, reps, batch=10):
    """Runs of `batch` calls, each run between two events and ended by a synchronise: (median device us per call, median host wall us
    per call, spread of the runs' host figures, the fastest run's host figure).  The host is shared: the medians are the figures, the spread
    says how much to trust them, and the fastest run is the nearest to an idle host."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(max(reps // batch, 5)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3 / batch)
        host.append((t1 - t0) / batch * 1e6)
    return round(statistics.median(dev), 1), round(statistics.median(host), 1), round(max(host) - min(host), 1), round(min(host), 1)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
    return len(names)


def paths(arch, dev):
    """The callables of one parameter list: adam-torch, adam-flat, accum-none, accum-torch, accum-flat."""
    names, ps = parameter_list(arch, dev)
    own = {i for i, n in enumerate(names) if n in ("prototype_vectors", "last_layer.weight")}
    adam, flat, acc = torch.optim.Adam(ps, lr=1e-4), optim.FlatAdam(ps, lr=1e-4), optim.GradAccumulator(ps)
    grads = [torch.randn_like(p) for p in ps]

    def set_grads():
        for p, g in zip(ps, grads):
            p.grad = g

    def backward():
        Emit.apply(own, *ps).backward()

    def accum_torch():  # p.grad is set: AccumulateGrad adds tensor by tensor
        backward()

    def accum_flat():  # the window holds the first micro-batch; this is the second
        backward()
        acc.absorb()

    def accum_none():  # the baseline of the two: the backward alone, its gradients dropped
        backward()
        for p in ps:
            p.grad = None

    def prepare(kind):
        for p in ps:
            p.grad = None
        acc.reset()
        if kind.startswith("adam"):
            set_grads()
        elif kind != "accum-none":
            backward()
            if kind == "accum-flat":
                acc.absorb()

    fns = {"adam-torch": adam.step, "adam-flat": flat.step, "accum-none": accum_none, "accum-torch": accum_torch, "accum-flat": accum_flat}
    return ps, fns, prepare, (flat, acc)


def sweep(dev, reps):
    rows = []
    for e in range(10, 27, 2):
        n = 1 << e
        p = torch.nn.Parameter(torch.randn(n, device=dev))
        p.grad = torch.randn(n, device=dev)
        opt = optim.FlatAdam([p], lr=1e-4)
        us, host, spread, _ = timed(opt.step, reps)
        rows.append({"bench": "pasn_adam_step, one tensor", "elements": n, "bytes": 28 * n, "device_us": us, "host_us_per_call": host, "host_spread_us": spread,
                     "GBps": round(28 * n / us / 1e3, 1), "share_of_hbm_peak": round(28 * n / (us * 1e-6) / HBM_PEAK, 4),
                     "fits_infinity_cache": 28 * n <= 256 << 20})
    return rows


def stats_summary(path, baseline, reps):
    """Launches and kernel time per call from two traced runs that differ only in ``--reps`` (``baseline``: the run with ``--reps 0``,
    i.e. the set-up alone: parameter lists, gradients, one first call).  A kernel with fewer calls than runs of the path is a table upload or
    set-up noise between the two processes."""
    import csv

    def load(f):
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(f))}

    run, base = load(path), load(baseline)
    diff = {k: (c - base.get(k, (0, 0.0))[0], ns - base.get(k, (0, 0.0))[1]) for k, (c, ns) in run.items()}
    diff = {k: v for k, v in diff.items() if v[0] > 0}
    print(f"{sum(c for c, _ in diff.values()) / reps:.1f} launches per call, {sum(ns for _, ns in diff.values()) / reps / 1e3:.1f} us of kernel time per call")
    for k, (c, ns) in sorted(((k, v) for k, v in diff.items() if v[1] > 0), key=lambda kv: -kv[1][1])[:5]:
        print(f"  {c / reps:6.1f} x {ns / c / 1e3:8.1f} us  {k[:110]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--trace", default="", choices=["", "adam-torch", "adam-flat", "accum-none", "accum-torch", "accum-flat"])
    ap.add_argument("--arch", default="x3d_s", choices=sorted(ARCHS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-summary", default="", help="a kernel_stats.csv of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--baseline", default="", help="... and the kernel_stats.csv of the same run with --reps 0")
    a = ap.parse_args()
    if a.stats_summary:
        return stats_summary(a.stats_summary, a.baseline, a.reps)
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    if a.trace:
        _, fns, prepare, _ = paths(a.arch, dev)
        prepare(a.trace)
        fns[a.trace]()  # belongs to the set-up: the first call creates optimizer state and tables
        for _ in range(a.reps):
            fns[a.trace]()
        torch.cuda.synchronize()
        print(json.dumps({"trace": a.trace, "arch": a.arch, "calls": a.reps}))
        return
    rows = []
    for arch in ARCHS:
        ps, fns, prepare, (flat, acc) = paths(arch, dev)
        row = {"bench": "optimizer side of a step", "arch": arch, "tensors": len(ps), "elements": sum(p.numel() for p in ps), "reps": a.reps,
               "device": torch.cuda.get_device_name()}
        for kind, fn in fns.items():
            prepare(kind)
            n_launch = launches(fn)
            prepare(kind)
            calls0 = flat.library_calls + acc.library_calls
            us, host, spread, best = timed(fn, a.reps)
            row[kind] = {"device_us": us, "host_us_per_call": host, "host_spread_us": spread, "host_us_fastest_run": best, "launches": n_launch}
            if kind.endswith("flat"):
                row[kind]["library_calls_per_call"] = round((flat.library_calls + acc.library_calls - calls0) / (5 + max(a.reps // 10, 5) * 10), 3)
        rows.append(row)
    rows += sweep(dev, a.reps)
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
