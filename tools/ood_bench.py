#!/usr/bin/env python3
"""``ood.knn``, ``ood.moments`` + ``ood.mahalanobis`` and ``ood.evaluate`` (csrc/ood.hip) against the same products in eager torch, on one GPU.

    python tools/ood_bench.py [--reps 20] [--out profiles/ood_bench.jsonl]

Sizes: banks of 10 000 and 100 000 rows, 32 and 10 000 queries, E = 40 and 256, k = 10, 4 classes.  Side A is the library: ``knn`` is one
memset and two launches whatever the sizes (exact fp32 distances in coordinate order, no query x bank matrix), ``moments`` one memset
and two launches, ``mahalanobis`` one launch, ``evaluate`` a tally (memset + launch) and the pairwise AUROC count, each ended by ONE
read.  Side B writes the same product in eager torch on the device: ``cdist`` + ``topk`` (which materialises the query x bank matrix and
computes it in GEMM form -- NOT bit for bit the library's distances: ``max_abs_difference_of_kth_distance`` says how far apart, and
``indices_that_differ`` how many neighbours change), ``einsum`` / ``index_add_`` moments in fp64, a batched matrix product for the
Mahalanobis scores, comparisons and a ``sort``-based Mann-Whitney count for the evaluation.

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by its
own synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of
repeats.  No ratio is fixed in advance: the exact kNN exists for its exactness, and where it is slower the line says so."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating  # noqa: E402
from protoasnet_amd import ood  # noqa: E402

K, KNN_K, TPRS = 4, 10, (0.9, 0.95, 0.99)


def rows(M, E, dev, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, K, (M,), generator=g)
    centres = torch.randn(K, E, generator=torch.Generator().manual_seed(E)) * 2.0
    return (centres[labels] + torch.randn(M, E, generator=g)).to(dev), labels.to(torch.int32).to(dev)


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
def torch_knn(q, bank):
    d, i = torch.cdist(q, bank).pow(2).topk(KNN_K, dim=1, largest=False)
    return d, i


def torch_moments(x, labels):
    xd = x.double()
    s = torch.zeros(K, x.shape[1], dtype=torch.float64, device=x.device).index_add_(0, labels.long(), xd)
    return torch.bincount(labels.long(), minlength=K), s, torch.einsum("mi,mj->ij", xd, xd)


def torch_mahalanobis(x, mu, W):
    y = (x.double()[:, None, :] - mu[None]) @ W.T
    return (y * y).sum(-1).min(1).values.float()


def torch_evaluate(scores, kind, tau, correct):
    """The eight tallies per level and the AUROC (midranks from a sort: the Mann-Whitney statistic with ties counted 1/2)."""
    idr, shifted = kind == 0, kind == 1
    flags = scores[None, :] > tau[:, None]
    ok = correct != 0
    t = torch.stack([idr.sum().expand(len(tau)), (flags & idr).sum(1), shifted.sum().expand(len(tau)), (flags & shifted).sum(1),
                     torch.zeros(len(tau), dtype=torch.long, device=scores.device), (~flags & idr & ok).sum(1), (~flags & idr).sum(1),
                     (flags & idr & ok).sum(1)], 1)
    s, order = torch.sort(scores)
    uniq, inverse, counts = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
    ends = counts.cumsum(0).double()
    midrank = (ends - (counts.double() - 1) / 2)[inverse]
    npos, nneg = shifted.sum().double(), idr.sum().double()
    auc = (midrank[shifted[order]].sum() - npos * (npos + 1) / 2) / (npos * nneg)
    return torch.cat([t.double().flatten(), auc[None]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--banks", default="10000,100000")
    ap.add_argument("--queries", default="32,10000")
    ap.add_argument("--dims", default="40,256")
    ap.add_argument("--library-only", action="store_true", help="the library side alone, a few calls: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name()
    lines = []

    def emit(line):
        lines.append(dict(line, device=name))
        print(json.dumps(lines[-1]), flush=True)

    for E in (int(x) for x in a.dims.split(",")):
        for Mb in (int(x) for x in a.banks.split(",")):
            bank, labels = rows(Mb, E, dev, seed=1)
            for Mq in (int(x) for x in a.queries.split(",")):
                q, _ = rows(Mq, E, dev, seed=2)
                lib = lambda: ood.knn(q, bank, KNN_K).dist.cpu()  # noqa: E731
                ref = lambda: torch_knn(q, bank)[0].cpu()  # noqa: E731
                if a.library_only:
                    for _ in range(3):
                        lib()
                    continue
                got, want = ood.knn(q, bank, KNN_K), torch_knn(q, bank)
                sa, sb = alternating(lib, ref, a.reps)
                pairs = Mq * Mb
                emit({"bench": "ood.knn", "queries": Mq, "bank": Mb, "E": E, "k": KNN_K, "reps": a.reps, "library": sa, "eager_torch": sb,
                      "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                      "library_launches": {"kernels": 2, "memsets": 1}, "vector_flop": 3 * pairs * E,
                      "library_tflops": round(3 * pairs * E / (sa["device_ms"] * 1e-3) / 1e12, 3),
                      "eager_matrix_bytes": 4 * pairs,
                      "max_abs_difference_of_kth_distance": float((got.dist[:, -1] - want[0][:, -1]).abs().max()),
                      "indices_that_differ": int((got.index != want[1].to(torch.int32)).sum())})
            if a.library_only:
                continue
            # the Gaussian side: moments of the bank (ended by the read of n), then the scores of 10 000 queries
            lib = lambda: ood.moments(bank, labels, K).n.cpu()  # noqa: E731
            ref = lambda: torch_moments(bank, labels)[2][0, :1].cpu()  # noqa: E731
            mo, tm = ood.moments(bank, labels, K), torch_moments(bank, labels)
            sa, sb = alternating(lib, ref, a.reps)
            emit({"bench": "ood.moments", "rows": Mb, "E": E, "K": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                  "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4), "library_launches": {"kernels": 2, "memsets": 1},
                  "max_rel_difference_of_scatter": float(((mo.scatter - tm[2]).abs() / tm[2].abs().clamp(min=1e-300)).max())})
            mu_h, W_h = ood.gaussian_fit(mo.n.cpu().numpy(), mo.sum.cpu().numpy(), mo.scatter.cpu().numpy())
            mu, W = torch.from_numpy(mu_h).to(dev), torch.from_numpy(W_h).to(dev)
            q, _ = rows(10000, E, dev, seed=3)
            lib = lambda: ood.mahalanobis(q, mu, W)[1].cpu()  # noqa: E731
            ref = lambda: torch_mahalanobis(q, mu, W).cpu()  # noqa: E731
            diff = float((ood.mahalanobis(q, mu, W)[1] - torch_mahalanobis(q, mu, W)).abs().max())
            sa, sb = alternating(lib, ref, a.reps)
            emit({"bench": "ood.mahalanobis", "rows": 10000, "fit_rows": Mb, "E": E, "K": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                  "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4), "library_launches": {"kernels": 1, "memsets": 0},
                  "max_abs_difference_of_score": diff})
    if not a.library_only:
        for M in (int(x) for x in a.banks.split(",")):
            g = torch.Generator().manual_seed(4)
            kind = (torch.rand(M, generator=g) < 0.5).to(torch.int32)
            scores = (torch.randn(M, generator=g) + kind.float()).to(dev)
            kind, correct = kind.to(dev), (torch.rand(M, generator=g) < 0.8).to(torch.int32).to(dev)
            th = ood.calibrate({"s": scores[kind == 0].contiguous()}, TPRS)
            lib = lambda: ood.evaluate({"s": scores}, kind, th, correct).packed().cpu()  # noqa: E731
            ref = lambda: torch_evaluate(scores, kind, th.tau["s"], correct).cpu()  # noqa: E731
            got, want = lib(), ref()
            sa, sb = alternating(lib, ref, a.reps)
            emit({"bench": "ood.evaluate", "rows": M, "levels": len(TPRS), "reps": a.reps, "library": sa, "eager_torch": sb,
                  "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                  "tallies_that_differ": int((got[:-1] != want[:-1]).sum()), "abs_difference_of_auroc": float((got[-1] - want[-1]).abs())})
            cal = lambda: ood.calibrate({"s": scores}, TPRS).tau["s"].cpu()  # noqa: E731
            tcal = lambda: torch.stack([torch.kthvalue(scores, min(M, int(-(-(M + 1) * t // 1)))).values for t in TPRS]).cpu()  # noqa: E731
            sa, sb = alternating(cal, tcal, a.reps)
            emit({"bench": "ood.calibrate", "rows": M, "levels": len(TPRS), "reps": a.reps, "library": sa, "eager_torch": sb,
                  "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4)})
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
