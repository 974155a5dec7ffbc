#!/usr/bin/env python3
"""``ordinal.screen`` and ``ordinal.agreement`` (csrc/ordinal.hip) against the same product in eager torch, on one GPU.

    python tools/ordinal_bench.py [--reps 20] [--out profiles/ordinal_bench.jsonl]

Cells: K_real = 4 (three cuts); M = 10 000 and 100 000 clip rows; B = 0 and B = 1000 replicates; the unit is the clip (G = M) or the cine
(10 clips per cine, interleaved).  Side A is the library: up to four memsets and six launches whatever B is, one read.  Side B sorts each
cut's scores once per call, then per chunk of replicates (sized to a fixed number of (replicate, row) elements so that it fits in
memory) draws the counts with ``randint`` + ``bincount`` and reads P, N, U2, average precision and the three kinds of operating point
off weighted ``cumsum``s gathered at the tie-run starts.  Its draws are torch's, not Philox's: the two sides are compared on the point
row, which is exact on both.  The agreement statistics are timed on their own: from the rows (``agreement``) and from B + 1 confusion
matrices (``agreement_of``), against ``bincount`` and elementwise torch.

Timing: 3 warm-up calls of each side, then ``--reps`` alternating A/B repeats, each call between two events and ended by its own
synchronising read; ``device_ms`` is the median event time, ``block_spread_ms`` the range of the medians of four consecutive blocks of
repeats.  No ratio is fixed in advance."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import ordinal, selective  # noqa: E402

K = 4
SPEC, SENS = (0.9,), (0.9,)
CHUNK_ELEMS = 4_000_000  # (replicates x rows) per chunk of the torch side: ~12 live fp64 / int64 tensors of this size


def case(M, cines, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    key_id = torch.randperm(M, generator=g) % cines
    labels = (key_id * 7919) % K
    logits = torch.rand(M, K, generator=g) * 8 - 4
    logits[torch.arange(M), labels] += 2.0
    probs = torch.softmax(logits, 1)
    return probs.to(dev), labels.to(torch.int32).to(dev), selective.build_groups(key_id.tolist())


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
class Order:
    """An ascending order shared by all replicates: the permutation, the sorted scores, and per position the first and last position of
    its tie run."""

    def __init__(self, score):
        self.s, self.idx = torch.sort(score, stable=True)
        _, inv, cnt = torch.unique_consecutive(self.s, return_inverse=True, return_counts=True)
        end = cnt.cumsum(0)
        self.first, self.last = (end - cnt)[inv], (end - 1)[inv]
        self.is_first = self.first == torch.arange(score.numel(), device=score.device)


def torch_cut(o, w, pos):
    """(P, N, U2, auc, ap, theta (n, 3), TP (n, 3), FP (n, 3)) of every replicate row of w (n, M) for one cut."""
    ws, p = w[:, o.idx], pos[o.idx]
    zero = torch.zeros_like(ws[:, :1])
    cp0, cn0 = torch.cat([zero, torch.cumsum(ws * p, 1)], 1), torch.cat([zero, torch.cumsum(ws * (~p), 1)], 1)
    P, N = cp0[:, -1:], cn0[:, -1:]
    plt, nlt = cp0[:, o.first], cn0[:, o.first]
    u2 = (ws * p * (nlt + cn0[:, o.last + 1])).sum(1)
    TP, FP = P - plt, N - nlt
    tpv = (cp0[:, o.last + 1] - plt) * o.is_first
    ap = torch.nan_to_num(tpv / P * (TP / (TP + FP))).sum(1)
    live = ws > 0
    n, M = ws.shape
    inf_col = torch.full((n, 1), float("inf"), dtype=o.s.dtype, device=ws.device)
    s_ext = torch.cat([o.s.expand(n, M), inf_col], 1)
    TPx, FPx = torch.cat([TP, zero], 1), torch.cat([FP, zero], 1)
    picks = []
    for tau in SPEC:  # the first position that qualifies; none: +inf (column M)
        ok = live & (nlt / N >= tau)
        picks.append(torch.where(ok.any(1), ok.int().argmax(1), torch.full((n,), M, device=ws.device)))
    for tau in SENS:  # the last position that qualifies
        ok = live & (TP / P >= tau)
        picks.append(M - 1 - ok.flip(1).int().argmax(1))
    J = torch.where(live, TP * N - FP * P, torch.full_like(TP, -1.0))
    jmax, jrev = J.flip(1).max(1)
    picks.append(torch.where(jmax > 0, M - 1 - jrev, torch.full((n,), M, device=ws.device)))
    pk = torch.stack(picks, 1)
    return P[:, 0], N[:, 0], u2, u2 / (2 * P[:, 0] * N[:, 0]), ap, s_ext.gather(1, pk), TPx.gather(1, pk), FPx.gather(1, pk)


def unit_ids(M, groups, dev):
    if groups is None:
        return M, torch.arange(M, device=dev)
    G = len(groups[0]) - 1
    gid = torch.empty(M, dtype=torch.int64, device=dev)
    gid[torch.from_numpy(groups[1]).to(dev).long()] = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(np.diff(groups[0])).to(dev))
    return G, gid


def torch_screen(probs, labels, groups, B, gen):
    """One fp64 vector per call: per replicate and cut P, N, U2, auc, ap and (theta, TP, FP) of the three operating points."""
    M = probs.shape[0]
    dev = probs.device
    G, gid = unit_ids(M, groups, dev)
    orders = []
    for c in range(1, K):  # p[c] + p[c + 1] + ... in that order, as the library adds them
        s = probs[:, c]
        for k in range(c + 1, K):
            s = s + probs[:, k]
        orders.append(Order(s))
    out = []
    step = max(1, CHUNK_ELEMS // M)
    for b0 in range(0, B + 1, step):
        n = min(step, B + 1 - b0)
        draws = torch.randint(0, G, (n, G), device=dev, generator=gen)
        counts = torch.bincount((draws + torch.arange(n, device=dev)[:, None] * G).flatten(), minlength=n * G).view(n, G)
        if b0 + n == B + 1:
            counts[-1] = 1  # the point row
        w = counts[:, gid].double()
        per = []
        for c in range(1, K):
            r = torch_cut(orders[c - 1], w, labels >= c)
            per.append(torch.cat([torch.stack(r[:5], 1), r[5].double(), r[6], r[7]], 1))
        out.append(torch.stack(per, 1))
    return torch.cat(out)


def torch_agreement_of(cm):
    """(R, 6) fp64 from (R, K, K) matrices, elementwise torch."""
    cm = cm.double()
    i = torch.arange(K, device=cm.device)
    d = (i[:, None] - i[None, :]).abs().double()
    n = cm.sum((1, 2))
    rc = cm.sum(2)[:, :, None] * cm.sum(1)[:, None, :]
    kap = [1 - n * (w * cm).sum((1, 2)) / (w * rc).sum((1, 2)) for w in (d, d * d)]
    return torch.stack([(d * cm).sum((1, 2)) / n, (cm * (d <= 1)).sum((1, 2)) / n, (cm * (i[None, :] < i[:, None])).sum((1, 2)) / n,
                        (cm * (i[None, :] > i[:, None])).sum((1, 2)) / n] + kap, 1)


def torch_agreement(probs, labels):
    cm = torch.bincount(labels.long() * K + probs.argmax(1), minlength=K * K).view(1, K, K)
    return torch_agreement_of(cm)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=0, help="repeats of the pairs whose torch side takes seconds (0: --reps)")
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--replicates", default="0,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for M in (int(x) for x in a.sizes.split(",")):
        probs, labels, groups = case(M, M // 10, dev)
        for unit in ("clip", "cine"):
            gr = None if unit == "clip" else groups[:2]
            G = M if gr is None else len(gr[0]) - 1
            for B in (int(x) for x in a.replicates.split(",")):
                lib = lambda: ordinal.screen(probs, labels, SPEC, SENS, gr, B, seed=1).packed().cpu()  # noqa: E731
                ref = lambda: torch_screen(probs, labels, gr, B, gen).cpu()  # noqa: E731
                ca = ordinal.Screening.split(lib().numpy(), K, B, 3, 0)
                cb = ref()[B].numpy()  # (cuts, 5 + 9)
                point = max(float(np.abs(ca["stats"][B] - cb[:, 3:5]).max()), float(np.abs(ca["op_theta"][B] - cb[:, 5:8]).max()),
                            float(np.abs(ca["op_tally"][B, :, :, 0] - cb[:, 8:11]).max()), float(np.abs(ca["u2"][B] - cb[:, 2]).max()))
                reps = a.torch_reps if a.torch_reps and M * B >= 10_000_000 else a.reps
                sa, sb = alternating(lib, ref, reps, warm=3 if reps >= 10 else 1)
                lines.append({"bench": "ordinal.screen", "unit": unit, "clip_rows": M, "groups": G, "K_real": K, "B": B,
                              "counts_in": "LDS" if G <= ordinal._lib.lib().pasn_bootstrap_lds_max_groups() else "global", "reps": reps,
                              "library": sa, "eager_torch": sb, "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                              "max_abs_difference_of_the_point_rows": point, "device": torch.cuda.get_device_name()})
                print(json.dumps(lines[-1]), flush=True)
        sa, sb = alternating(lambda: ordinal.agreement(probs, labels).stats.cpu(), lambda: torch_agreement(probs, labels).cpu(), a.reps)
        diff = float((ordinal.agreement(probs, labels).stats.cpu() - torch_agreement(probs, labels).cpu()).abs().max())
        lines.append({"bench": "ordinal.agreement", "clip_rows": M, "K_real": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                      "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4), "max_abs_difference": diff,
                      "device": torch.cuda.get_device_name()})
        print(json.dumps(lines[-1]), flush=True)
    cms = torch.randint(0, 5000, (1001, K, K), device=dev, generator=gen)
    sa, sb = alternating(lambda: ordinal.agreement_of(cms).stats.cpu(), lambda: torch_agreement_of(cms).cpu(), a.reps)
    lines.append({"bench": "ordinal.agreement_of", "matrices": 1001, "K_real": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                  "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                  "max_abs_difference": float((ordinal.agreement_of(cms).stats.cpu() - torch_agreement_of(cms).cpu()).abs().max()),
                  "device": torch.cuda.get_device_name()})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
