#!/usr/bin/env python3
"""``prune.importance`` / ``prune.eliminate`` (csrc/prune.hip) against the same products in eager torch, on one GPU.

    python tools/prune_bench.py [--reps 20] [--out profiles/prune_bench.jsonl]

Sizes: M = 10 000 and 100 000 rows, P = 40 prototypes, K = K_real = 5.  Side A is the library: ``importance`` is one memset and two
launches (the pass that builds z and tallies; the one-block sum of the chunk partials), ``eliminate(keep_per_class=2)`` one memset and
1 + 2 x 30 launches, each ended by ONE read.  Side B writes the same products in eager torch on the device: a float64 matmul for z, the
(M, P, K) ablated logits by broadcasting, ``argmax`` / comparisons / ``sum`` for the tallies, a masked ``max`` for the margins; its
elimination loop reads the (P,) keys on the host every round to pick (an eager loop has to decide somewhere) and updates z by the same
subtraction.  Its sums are torch's reductions, not the fixed chunk order, and its z a matmul, so the margin sums agree to rounding only;
the integer tallies and the removal order are compared and the differences reported.

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by its
own synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of
repeats.  No ratio is fixed in advance."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating  # noqa: E402
from protoasnet_amd import prune  # noqa: E402

P, K, KEEP = 40, 5, 2
ROUNDS = P - K * KEEP
LIBRARY_LAUNCHES = {"importance": {"kernels": 2, "memsets": 1}, "eliminate": {"kernels": 1 + 2 * ROUNDS, "memsets": 1}}


def case(M, dev, seed=0):
    """A model that is mostly right with redundant prototypes: the last layer favours a prototype's class, the similarities of the
    label's prototypes are raised."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.arange(P) // (P // K)
    labels = torch.randint(0, K, (M,), generator=g)
    w = torch.where(cls[None, :] == torch.arange(K)[:, None], torch.tensor(1.0), -0.5 * torch.rand(K, P, generator=g))
    sim = (0.6 * torch.rand(M, P, generator=g) + 0.3 * (cls[None, :] == labels[:, None]) * torch.rand(M, P, generator=g)).clamp(0, 1)
    return sim.to(dev), w.to(dev), labels.to(torch.int32).to(dev), cls.to(torch.int32).to(dev)


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
def torch_table(z, sim, w, labels):
    """(wrong (P + 1,), flips (P,), wrong per class (P + 1, K), margin sums (P + 1,)) of every ablation and of the model itself."""
    y = labels.long()
    za = z[:, None, :] - sim.double()[:, :, None] * w.double().t()[None]  # (M, P, K)
    za = torch.cat([za, z[:, None, :]], dim=1)
    pred = za.argmax(2)
    wrong = pred != y[:, None]
    per = torch.nn.functional.one_hot(y, K).double().t() @ wrong.double()  # (K, P + 1)
    flips = (pred[:, :P] != pred[:, P:]).sum(0)
    own = za.gather(2, y[:, None, None].expand(-1, P + 1, 1))[..., 0]
    other = za.masked_fill(torch.nn.functional.one_hot(y, K).bool()[:, None, :], float("-inf")).amax(2)
    return wrong.sum(0), flips, per.t(), (own - other).sum(0)


def torch_importance(sim, w, labels):
    z = sim.double() @ w.double().t()
    return torch_table(z, sim, w, labels)


def torch_eliminate(sim, w, labels, cls):
    z = sim.double() @ w.double().t()
    kept = torch.ones(P, dtype=torch.bool)
    counts = torch.bincount(cls.cpu().long(), minlength=K)
    cls_h = cls.cpu().tolist()
    order, trace = [], []
    for _ in range(ROUNDS):
        wrong, _, _, ms = torch_table(z, sim, w, labels)
        wh, mh = wrong.cpu().tolist(), ms.cpu().tolist()  # the round's host read
        best = min((p for p in range(P) if kept[p] and counts[cls_h[p]] > KEEP), key=lambda p: (wh[p], -mh[p], p))
        order.append(best)
        trace.append((wh[best], mh[best]))
        kept[best] = False
        counts[cls_h[best]] -= 1
        z = z - sim[:, best:best + 1].double() * w[:, best].double()[None, :]
    return order, trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--library-only", action="store_true", help="the library side alone, a few calls: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    lines = []
    for M in (int(x) for x in a.sizes.split(",")):
        sim, w, labels, cls = case(M, dev)
        lib_imp = lambda: prune.importance(sim, w, labels, K, cls).read()  # noqa: E731
        lib_eli = lambda: prune.eliminate(sim, w, labels, K, cls, keep_per_class=KEEP).read()  # noqa: E731
        if a.library_only:
            for _ in range(3):
                lib_imp()
                lib_eli()
            continue
        ref_imp = lambda: [t.cpu() for t in torch_importance(sim, w, labels)]  # noqa: E731
        ref_eli = lambda: torch_eliminate(sim, w, labels, cls)  # noqa: E731
        got, want = lib_imp(), ref_imp()
        counts_differ = int((torch.from_numpy(got["wrong"]) != want[0][:P]).sum() + (torch.from_numpy(got["flips"]) != want[1]).sum())
        margin_diff = float((torch.from_numpy(got["margin_sum"]) - want[3][:P]).abs().max())
        sa, sb = alternating(lib_imp, ref_imp, a.reps)
        lines.append({"bench": "prune.importance", "rows": M, "P": P, "K": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                      "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4), "library_launches": LIBRARY_LAUNCHES["importance"],
                      "tally_counts_that_differ": counts_differ, "max_abs_difference_of_margin_sums": margin_diff,
                      "device": torch.cuda.get_device_name()})
        print(json.dumps(lines[-1]), flush=True)
        got, (order, trace) = lib_eli(), ref_eli()
        sa, sb = alternating(lib_eli, ref_eli, max(4, a.reps // 2))
        lines.append({"bench": "prune.eliminate", "rows": M, "P": P, "K": K, "rounds": ROUNDS, "keep_per_class": KEEP, "reps": max(4, a.reps // 2),
                      "library": sa, "eager_torch": sb, "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                      "library_launches": LIBRARY_LAUNCHES["eliminate"], "same_removal_order": got["order"] == order,
                      "wrong_after_last_round": [got["trace"][-1]["wrong"], trace[-1][0]], "device": torch.cuda.get_device_name()})
        print(json.dumps(lines[-1]), flush=True)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
