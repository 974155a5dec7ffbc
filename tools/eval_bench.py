#!/usr/bin/env python3
"""Device time of the evaluation-metric kernels (csrc/eval_metrics.hip).

    python tools/eval_bench.py [--reps 50] [--out profiles/eval_bench.jsonl]

pasn_eval_batch_stats at one batch of the video configs (32 clips x 40 prototypes, 4 logits with the abstain class, every output on),
and pasn_roc_auc_ovr (both launches) at M = 4 096 / 16 384 / 65 536 rows, K_real = 3.  Device events around each call, every shape warmed
first, the median of --reps calls.  The per-batch launch is meant to stay small next to a forward; the AUC runs once per epoch.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import _lib, metrics  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    name = torch.cuda.get_device_name()
    rows = []

    N, P, K, K_real, P_cls, cap = 32, 40, 4, 3, 30, 1 << 16
    logits = torch.randn(N, K, device=dev, generator=g)
    sim = torch.rand(N, P, device=dev, generator=g)
    target = torch.randint(0, K_real, (N,), device=dev, generator=g)
    probs = torch.empty(cap, K_real, device=dev)
    labels = torch.empty(cap, dtype=torch.int32, device=dev)
    lg_out = torch.empty(cap, K, device=dev)
    sp = torch.zeros(2, dtype=torch.int64, device=dev)
    div = torch.zeros(P, dtype=torch.int64, device=dev)
    sums = torch.zeros(P, dtype=torch.float64, device=dev)

    def batch():
        metrics._batch_stats(logits, sim, target, K_real, P_cls, 0.8, 0, cap, probs, labels, lg_out, sp, div, sums)

    t = timed(batch, a.reps)
    rows.append({"kernel": "pasn_eval_batch_stats", "N": N, "P": P, "K": K, "K_real": K_real, "P_cls": P_cls, "outputs": "all",
                 "us": round(t * 1e6, 2), "reps": a.reps, "device": name})

    for M in (4096, 16384, 65536):
        p = torch.softmax(torch.randn(M, 3, device=dev, generator=g), 1)
        y = torch.randint(0, 3, (M,), device=dev, generator=g).to(torch.int32)
        ws = torch.empty(int(_lib.lib().pasn_roc_auc_workspace_bytes(M, 3)) // 4 + 1, dtype=torch.int32, device=dev)
        auc = torch.empty(1, dtype=torch.float64, device=dev)
        auc_k = torch.empty(3, dtype=torch.float64, device=dev)

        def run():
            _lib.check(_lib.lib().pasn_roc_auc_ovr(p.data_ptr(), y.data_ptr(), M, 3, auc.data_ptr(), auc_k.data_ptr(), ws.data_ptr(),
                                                   _lib.current_stream()))

        t = timed(run, a.reps)
        rows.append({"kernel": "pasn_roc_auc_ovr", "M": M, "K_real": 3, "pairs": M * M, "us": round(t * 1e6, 2),
                     "Gpairs_per_s": round(M * M / t / 1e9, 1), "reps": a.reps, "device": name})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
