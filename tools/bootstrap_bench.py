#!/usr/bin/env python3
"""``bootstrap.replicates`` + ``bootstrap.intervals`` (csrc/bootstrap.hip) against the same product in eager torch, on one GPU.

    python tools/bootstrap_bench.py [--reps 20] [--out profiles/bootstrap_bench.jsonl]

Sizes: B = 1000 and 2000 replicates of M = 10 000 and 100 000 clip rows, K_real = 4, with an uncertainty; the unit is the clip (G = M)
or the cine (about 10 clips per cine, interleaved).  Side A is the library: six launches and three memsets whatever B is, one read.
Side B computes the same six statistics per replicate in eager torch: the sorted orders and their tie runs once per call, then per chunk
of replicates (sized to a fixed number of (replicate, row) elements so that it fits in memory) ``randint`` + ``bincount`` for the counts,
a matrix product for the confusion matrices, weighted ``cumsum`` rank sums gathered at the tie-run ends for the AUCs, and the
risk-coverage area of the weighted rows in closed form through ``digamma`` (the sum of 1 / (T + t) over a row's copies).  Its draws
are torch's, not Philox's: the two sides estimate the same intervals and are compared on the point row (exact on both) and on the
interval widths.

Timing: 3 warm-up calls of each side, then ``--reps`` alternating A/B repeats, each call between two events and ended by its own
synchronising read; ``device_ms`` is the median event time, ``block_spread_ms`` the range of the medians of four consecutive blocks of
repeats.  No ratio is fixed in advance.  ``--trainer``: what ``evaluate_selective(bootstrap=1000)`` adds on the synthetic split."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import bootstrap, selective  # noqa: E402

K = 4
CHUNK_ELEMS = 4_000_000  # (replicates x rows) per chunk of the torch side: ~10 live fp64 / int64 tensors of this size


def case(M, cines, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    key_id = torch.randperm(M, generator=g) % cines
    labels = (key_id * 7919) % K
    logits = torch.rand(M, K, generator=g) * 8 - 4
    logits[torch.arange(M), labels] += 2.0
    probs = torch.softmax(logits, 1)
    u = 1 - probs.max(1).values
    return probs.to(dev), labels.to(torch.int32).to(dev), u.to(dev), selective.build_groups(key_id.tolist())


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
class Order:
    """A sorted order shared by all replicates: the permutation, and per position the first and last position of its tie run."""

    def __init__(self, score):
        s, self.idx = torch.sort(score.double(), stable=True)
        _, inv, cnt = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
        end = cnt.cumsum(0)
        self.first, self.last = (end - cnt)[inv], (end - 1)[inv]


def u2_weighted(order, w, pos):
    """sum over (i positive, j negative) of w_i w_j (2 [s_j < s_i] + [s_j == s_i]) for every replicate row of w (Bc, M), fp64."""
    ws, p = w[:, order.idx], pos[order.idx]
    cn = torch.cumsum(ws * (~p), 1)
    cn0 = torch.cat([torch.zeros_like(cn[:, :1]), cn], 1)  # exclusive prefix at [i], inclusive at [i + 1]
    return (ws * p * (cn0[:, order.first] + cn0[:, order.last + 1])).sum(1)


def torch_replicates(probs, labels, u, groups, B, gen):
    M = probs.shape[0]
    dev = probs.device
    pred = probs.argmax(1)
    lab = labels.long()
    right = pred == lab
    if groups is None:
        G, gid = M, torch.arange(M, device=dev)
    else:
        G = len(groups[0]) - 1
        gid = torch.empty(M, dtype=torch.int64, device=dev)
        gid[torch.from_numpy(groups[1]).to(dev).long()] = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(np.diff(groups[0])).to(dev))
    cell = torch.nn.functional.one_hot(lab * K + pred, K * K).double()
    orders = [Order(probs[:, k]) for k in range(K)]
    ou = Order(u)
    out = []
    step = max(1, CHUNK_ELEMS // M)
    for b0 in range(0, B + 1, step):
        n = min(step, B + 1 - b0)
        draws = torch.randint(0, G, (n, G), device=dev, generator=gen)
        counts = torch.bincount((draws + torch.arange(n, device=dev)[:, None] * G).flatten(), minlength=n * G).view(n, G)
        if b0 + n == B + 1:
            counts[-1] = 1  # the point row
        w = counts[:, gid].double()
        cm = (w @ cell).view(n, K, K)
        tp, sup, prd = cm.diagonal(dim1=1, dim2=2), cm.sum(2), cm.sum(1)
        W = sup.sum(1)
        acc = tp.sum(1) / W
        bal = torch.where(sup > 0, tp / sup.clamp(min=1), torch.zeros_like(tp)).sum(1) / (sup > 0).sum(1)
        f1 = torch.where(sup + prd > 0, 2 * tp / (sup + prd).clamp(min=1), torch.zeros_like(tp)).mean(1)
        auc_k = torch.stack([u2_weighted(orders[k], w, lab == k) for k in range(K)], 1) / (2 * sup * (W[:, None] - sup))
        auc = (sup * auc_k).sum(1) / W  # NaN where a class is lost (0 / 0)
        ws, r = w[:, ou.idx], right[ou.idx]
        T = torch.cumsum(ws, 1) - ws
        C = torch.cumsum(ws * r, 1) - ws * r
        h = torch.special.digamma(T + ws + 1) - torch.special.digamma(T + 1)  # sum over a row's copies of 1 / (T + t)
        aurc = torch.where(r, (T - C) * h, ws - C * h).sum(1) / W
        wrong_w = W - tp.sum(1)
        ea = u2_weighted(ou, w, ~right) / (2 * wrong_w * tp.sum(1))
        out.append(torch.stack([acc, bal, f1, auc, aurc, ea], 1))
    return torch.cat(out)


# ---- timing ------------------------------------------------------------------------------------------------------------------------------
def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def summary(t):
    dev, wall = [x[0] for x in t], [x[1] for x in t]
    n = max(len(dev) // 4, 1)
    blocks = [statistics.median(dev[i: i + n]) for i in range(0, len(dev) - n + 1, n)]
    return {"device_ms": round(statistics.median(dev), 3), "wall_ms": round(statistics.median(wall), 3),
            "block_spread_ms": round(max(blocks) - min(blocks), 3), "fastest_ms": round(min(dev), 3)}


def alternating(fa, fb, reps, warm=3):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(one(fa))
        tb.append(one(fb))
    return summary(ta), summary(tb)


def trainer_lines(reps):
    """``evaluate_selective`` on the synthetic split of the tests with and without ``bootstrap=1000``."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from protoasnet_amd.trainer import DPTrainer
    from test_cpu_trainer import TRAIN_CFG
    from test_gpu_selective import _cine_loader
    from util import CFG_VIDEO_X3D, synth_model

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to("cuda")
    loader = _cine_loader(4, 3, 70)
    t = DPTrainer(m, {"abstain_class": True, "save_dir": "", "train": TRAIN_CFG}, {"train": loader, "val": loader, "test": loader}, log=lambda *_: None)
    out = []
    for level in ("clip", "cine"):
        sa, sb = alternating(lambda: t.evaluate_selective("test", level=level, bootstrap=1000), lambda: t.evaluate_selective("test", level=level), reps)
        out.append({"bench": "DPTrainer.evaluate_selective", "level": level, "clip_rows": 12, "cines": 3, "reps": reps, "bootstrap_1000": sa, "bootstrap_0": sb,
                    "added_device_ms": round(sa["device_ms"] - sb["device_ms"], 3), "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=0, help="repeats of the pairs whose torch side takes seconds (0: --reps)")
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--replicates", default="1000,2000")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for M in (int(x) for x in a.sizes.split(",")):
        probs, labels, u, groups = case(M, M // 10, dev)
        for unit in ("clip", "cine"):
            gr = None if unit == "clip" else groups[:2]
            for B in (int(x) for x in a.replicates.split(",")):
                lib = lambda: bootstrap.intervals(bootstrap.replicates(probs, labels, u, gr, B, seed=1))  # noqa: E731
                ref = lambda: bootstrap.intervals_of(torch_replicates(probs, labels, u, gr, B, gen).cpu().numpy())  # noqa: E731
                ca, cb = lib(), ref()
                point = max(abs(ca[n]["point"] - cb[n]["point"]) for n in ca)
                width = max(abs((ca[n]["hi"] - ca[n]["lo"]) / (cb[n]["hi"] - cb[n]["lo"]) - 1) for n in ca)
                reps = a.torch_reps if a.torch_reps and M * B >= 100_000_000 else a.reps
                sa, sb = alternating(lib, ref, reps, warm=3 if reps >= 10 else 1)
                lines.append({"bench": "bootstrap.replicates+intervals", "unit": unit, "clip_rows": M, "groups": M if gr is None else len(gr[0]) - 1,
                              "K_real": K, "B": B, "counts_in": "LDS" if (M if gr is None else len(gr[0]) - 1) <= bootstrap.lds_max_groups() else "global",
                              "reps": reps, "library": sa, "eager_torch": sb, "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                              "max_abs_difference_of_the_point_rows": point, "max_relative_difference_of_the_interval_widths": round(width, 4),
                              "device": torch.cuda.get_device_name()})
                print(json.dumps(lines[-1]), flush=True)
    if a.trainer:
        lines += trainer_lines(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
