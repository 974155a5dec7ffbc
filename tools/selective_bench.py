#!/usr/bin/env python3
"""``SelectiveEvaluator.finish`` (csrc/selective.hip, protoasnet_amd/selective.py) against the same product in eager torch, on one GPU.

    python tools/selective_bench.py [--reps 20] [--out profiles/selective_bench.jsonl]

Sizes: 10 000 and 100 000 clip rows at clip level; 1 000 and 10 000 cines of 10 clips each at cine level.  Side A is ``finish``: the
uncertainty scores, (cine level) the CSR group reduction, the rank-by-counting order, the prefix-count curves, AURC, the error AUROC and
(cine level) the confusion matrix and one-vs-rest AUC of the cine predictions, read with one copy.  Side B computes the same numbers with
``softmax``, ``argsort(stable=True)``, ``cumsum`` of one-hot rows, ``index_add_`` (groups), ``bincount`` (confusion matrix) and a
sort-based tie-aware AUROC, read with one copy as well; both sides build the groups with the same host function inside the timed call.

Timing: 3 warm-up calls of each side, then ``--reps`` alternating A/B repeats, each call between two events and ended by the
synchronising read it contains anyway; ``device_ms`` is the median over the repeats of the event time (it includes the host work of the
call: the launches are not queued ahead), ``wall_ms`` the median host time, and ``block_spread_ms`` the range of the medians of four
consecutive blocks of repeats -- how far the figure moves on a shared host.  No ratio is fixed in advance: the lines say which side wins
at which size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import selective  # noqa: E402

COVERAGES = (1.0, 0.9, 0.8, 0.7, 0.5)
K, P = 4, 8  # three real classes and the abstention class


class Head(torch.nn.Module):
    """The model surface EpochEvaluator reads."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.num_classes, self.num_prototypes, self.prototype_shape = K, P, (P, 8, 1, 1, 1)
        self.prototype_class_identity = torch.zeros(P, K)
        for j in range(P):
            self.prototype_class_identity[j, j // (P // K)] = 1


def filled_evaluator(rows, cines, dev, seed=0):
    """A SelectiveEvaluator holding ``rows`` clips of ``cines`` cines (a cine's clips interleaved with the others'), fed in batches."""
    g = torch.Generator().manual_seed(seed)
    key_id = torch.randperm(rows, generator=g) % cines
    labels = (key_id * 7919) % 3
    logits = torch.rand(rows, K, generator=g) * 8 - 4
    logits[torch.arange(rows), labels] += 2.0  # a model that is right more often than not
    sel = selective.SelectiveEvaluator(Head().to(dev), abstain_class=True, capacity=rows)
    names = [f"cine{i}" for i in key_id.tolist()]
    for s in range(0, rows, 1000):
        e = min(rows, s + 1000)
        sel.update(logits[s:e].to(dev), torch.rand(e - s, P, device=dev), labels[s:e].to(dev), names[s:e])
    return sel


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
def auroc(score, pos):
    """Mann-Whitney AUROC with ties counted 1/2 (fp64), NaN when a side is empty."""
    s, idx = torch.sort(score.double())
    _, inv, cnt = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    rank = (cnt.cumsum(0).double() - (cnt.double() - 1) / 2)[inv]
    p = pos[idx].double()
    npos = p.sum()
    return ((rank * p).sum() - npos * (npos + 1) / 2) / (npos * (p.numel() - npos))


def torch_curve(probs, labels, u, cs):
    Kr = probs.shape[1]
    order = torch.argsort(torch.where(torch.isnan(u), torch.full_like(u, float("inf")), u), stable=True)
    pred = probs.argmax(1)
    lab, prd = labels.long()[order], pred[order]
    sup = torch.nn.functional.one_hot(lab, Kr).cumsum(0).double()
    pre = torch.nn.functional.one_hot(prd, Kr).cumsum(0).double()
    tp = (torch.nn.functional.one_hot(lab, Kr) * (lab == prd)[:, None]).cumsum(0).double()
    m = torch.arange(1, lab.numel() + 1, device=u.device, dtype=torch.float64)
    acc = tp.sum(1) / m
    present = sup > 0
    bal = torch.where(present, tp / sup.clamp(min=1), torch.zeros_like(tp)).sum(1) / present.sum(1)
    f1 = torch.where(sup + pre > 0, 2 * tp / (sup + pre).clamp(min=1), torch.zeros_like(tp)).mean(1)
    i = selective.coverage_rows(cs, torch.tensor(lab.numel(), device=u.device)) - 1
    return torch.cat([acc[i], bal[i], f1[i], u[order][i].double(), (1 - acc).mean().reshape(1), auroc(u, pred != labels).reshape(1)])


def torch_finish(sel, cs, level):
    ev, Kr = sel.ev, sel.ev.K_real
    logits, labels = ev.logits[: ev.rows], ev.labels[: ev.rows]
    probs, u = torch.softmax(logits[:, :Kr], 1), torch.softmax(logits, 1)[:, Kr]
    if level == "clip":
        return torch_curve(probs, labels, u, cs).cpu()
    offsets, rows, names = selective.build_groups(sel.keys)
    G, dev = len(names), probs.device
    gid = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(np.diff(offsets)).to(dev))
    r = torch.from_numpy(rows).to(dev).long()
    w = 1 - u[r].double()
    num = torch.zeros(G, Kr, dtype=torch.float64, device=dev).index_add_(0, gid, w[:, None] * probs[r].double())
    den = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, gid, w)
    cnt = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, gid, torch.ones_like(w))
    um = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, gid, u[r].double()) / cnt
    pc = (num / den[:, None]).float()
    gl = labels[r[torch.from_numpy(offsets[:-1]).to(dev)]]
    cm = torch.bincount(gl.long() * Kr + pc.argmax(1), minlength=Kr * Kr).double()
    npos = torch.bincount(gl.long(), minlength=Kr).double()
    auc = (torch.stack([auroc(pc[:, k], gl == k) for k in range(Kr)]) * npos).sum() / npos.sum()
    return torch.cat([torch_curve(pc, gl, um.float(), cs), cm, auc.reshape(1), pc.double().flatten(), um]).cpu()


# ---- timing ------------------------------------------------------------------------------------------------------------------------------
def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def alternating(fa, fb, reps):
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(one(fa))
        tb.append(one(fb))

    def summary(t):
        dev, wall = [x[0] for x in t], [x[1] for x in t]
        n = max(len(dev) // 4, 1)
        blocks = [statistics.median(dev[i: i + n]) for i in range(0, len(dev) - n + 1, n)]
        return {"device_ms": round(statistics.median(dev), 3), "wall_ms": round(statistics.median(wall), 3),
                "block_spread_ms": round(max(blocks) - min(blocks), 3), "fastest_ms": round(min(dev), 3)}

    return summary(ta), summary(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    assert a.reps >= 20, "at least 20 alternating repeats"
    dev = torch.device("cuda")
    lines = []
    for level, rows, cines in (("clip", 10_000, 1_000), ("clip", 100_000, 10_000), ("cine", 10_000, 1_000), ("cine", 100_000, 10_000)):
        sel = filled_evaluator(rows, cines, dev)
        lib, ref = sel.finish(COVERAGES, level), torch_finish(sel, COVERAGES, level)
        nc = len(COVERAGES)
        agree = max(abs(lib[f"accuracy@{c:g}"] - float(ref[j])) for j, c in enumerate(COVERAGES))
        agree = max(agree, abs(lib["aurc"] - float(ref[4 * nc])), abs(lib["error_auroc"] - float(ref[4 * nc + 1])))
        t0 = time.perf_counter()
        selective.build_groups(sel.keys)
        groups_ms = (time.perf_counter() - t0) * 1e3
        sa, sb = alternating(lambda: sel.finish(COVERAGES, level), lambda: torch_finish(sel, COVERAGES, level), a.reps)
        lines.append({"bench": "SelectiveEvaluator.finish", "level": level, "clip_rows": rows, "cines": cines if level == "cine" else None,
                      "reps": a.reps, "library": sa, "eager_torch": sb, "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 3),
                      "host_build_groups_ms": round(groups_ms, 3) if level == "cine" else None, "max_abs_difference_of_the_two": agree,
                      "device": torch.cuda.get_device_name()})
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
