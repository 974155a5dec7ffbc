#!/usr/bin/env python3
"""``conformal.calibrate`` / ``conformal.predict_sets`` (csrc/conformal.hip) against the same product in eager torch, on one GPU.

    python tools/conformal_bench.py [--reps 20] [--out profiles/conformal_bench.jsonl]

Sizes: M = 10 000 and 100 000 rows, K_real = 4, A = 3 levels (0.05, 0.1, 0.2); every kind (``lac``, randomised ``aps``, randomised
``raps``), marginal and Mondrian sets.  Side A is the library: ``calibrate`` is 6 kernel launches and one memset whatever M is (scores,
four counting passes of the radix select, the finish), ``predict_sets`` 2 launches and one memset (scores, sets), each ended by ONE read.
Side B writes the same product in eager torch on the device: ``sort`` / ``cumsum`` / ``scatter`` for the score table, ``gather`` for the
own-label scores, a boolean selection and ``kthvalue`` per stratum and level for the thresholds (a host read per stratum: the rank
depends on the count), comparisons and ``bincount`` for the masks and tallies.  Its uniforms are torch's, not Philox's, and its running
sum is ``cumsum - p``, so the two sides are compared on the deterministic kinds only (``max_abs_difference_of_qhat``, and the tallies
must agree exactly there).

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by its
own synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of
repeats.  No ratio is fixed in advance."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating  # noqa: E402
from protoasnet_amd import conformal  # noqa: E402

K, ALPHAS, LAM, K_REG = 4, (0.05, 0.1, 0.2), 0.01, 2
LIBRARY_LAUNCHES = {"calibrate": {"kernels": 6, "memsets": 1}, "predict_sets": {"kernels": 2, "memsets": 1}}


def case(M, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, K, generator=g)
    labels = torch.multinomial(torch.softmax(z, 1), 1, generator=g)[:, 0]
    return torch.softmax(2.5 * z, 1).to(dev), labels.to(torch.int32).to(dev), torch.rand(M, generator=g).to(dev)


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
def torch_scores(probs, kind, randomized, gen):
    p = probs.double()
    if kind == "lac":
        return (1.0 - p).float()
    ps, order = torch.sort(p, dim=1, descending=True, stable=True)
    U = torch.rand(p.shape[0], 1, dtype=torch.float64, device=p.device, generator=gen) if randomized else 1.0
    s = (ps.cumsum(1) - ps) + U * ps
    if kind == "raps":
        s = s + LAM * (torch.arange(1, p.shape[1] + 1, device=p.device) - K_REG).clamp(min=0).double()
    return torch.empty_like(s).scatter_(1, order, s).float()


def torch_calibrate(probs, labels, kind, randomized, gen):
    """qhat (1 + K, A) fp32: per stratum a selection, its count read on the host, and one kthvalue per level."""
    table = torch_scores(probs, kind, randomized, gen)
    lab = labels.long()
    own = table.gather(1, lab[:, None])[:, 0]
    q = torch.full((K + 1, len(ALPHAS)), float("inf"), device=probs.device)
    for s in range(K + 1):
        vals = own if s == 0 else own[lab == s - 1]
        n = vals.numel()
        for a, alpha in enumerate(ALPHAS):
            r = math.ceil((n + 1) * (1.0 - alpha))
            if r <= n:
                q[s, a] = torch.kthvalue(vals, r).values
    return q


def torch_predict(probs, labels, u, qhat, kind, randomized, mondrian, gen):
    """(masks (A, M) int32, tallies (A, T) fp64 in the library's order; nan_rows 0, every row valid)."""
    table = torch_scores(probs, kind, randomized, gen)
    M = table.shape[0]
    lab, ud = labels.long(), u.double()
    bit = 1 << torch.arange(K, device=table.device)
    masks, tallies = [], []
    for a in range(len(ALPHAS)):
        inset = table <= (qhat[1:, a][None, :] if mondrian else qhat[0, a])
        size = inset.sum(1)
        cov = inset.gather(1, lab[:, None])[:, 0]
        masks.append((inset * bit).sum(1).to(torch.int32))
        tallies.append(torch.cat([
            torch.tensor([M], dtype=torch.float64, device=table.device), cov.sum().double()[None], torch.zeros(1, dtype=torch.float64, device=table.device),
            torch.bincount(size, minlength=K + 1).double(), torch.bincount(size[cov], minlength=K + 1).double(),
            torch.bincount(size, weights=ud, minlength=K + 1), torch.bincount(size, minlength=K + 1).double(),
            torch.bincount(lab, minlength=K).double(), torch.bincount(lab[cov], minlength=K).double()]))
    return torch.stack(masks), torch.stack(tallies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--library-only", action="store_true", help="the library side alone, a few calls: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for M in (int(x) for x in a.sizes.split(",")):
        probs, labels, u = case(M, dev)
        for kind, rnd in (("lac", False), ("aps", True), ("raps", True)):
            kw = dict(kind=kind, randomized=rnd, seed=1, lam=LAM, k_reg=K_REG)
            lib = lambda: conformal.calibrate(probs, labels, ALPHAS, **kw).qhat.cpu()  # noqa: E731
            ref = lambda: torch_calibrate(probs, labels, kind, rnd, gen).cpu()  # noqa: E731
            if a.library_only:
                for _ in range(3):
                    lib()
                    conformal.predict_sets(probs, conformal.calibrate(probs, labels, ALPHAS, **kw), labels, u).tallies.cpu()
                continue
            det = dict(kw, randomized=False)
            diff = float((conformal.calibrate(probs, labels, ALPHAS, **det).qhat.cpu() - torch_calibrate(probs, labels, kind, False, gen).cpu()).abs().max())
            sa, sb = alternating(lib, ref, a.reps)
            lines.append({"bench": "conformal.calibrate", "rows": M, "K_real": K, "A": len(ALPHAS), "kind": kind, "randomized": rnd, "reps": a.reps,
                          "library": sa, "eager_torch": sb, "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                          "library_launches": LIBRARY_LAUNCHES["calibrate"], "max_abs_difference_of_qhat_deterministic": diff,
                          "device": torch.cuda.get_device_name()})
            print(json.dumps(lines[-1]), flush=True)
            fit = conformal.calibrate(probs, labels, ALPHAS, **kw)
            fit_det = conformal.calibrate(probs, labels, ALPHAS, **det)
            for mondrian in (False, True):
                lib = lambda: conformal.predict_sets(probs, fit, labels, u, mondrian=mondrian).tallies.cpu()  # noqa: E731
                ref = lambda: torch_predict(probs, labels, u, fit.qhat, kind, rnd, mondrian, gen)[1].cpu()  # noqa: E731
                got = conformal.predict_sets(probs, fit_det, labels, u, mondrian=mondrian).tallies.cpu().double()
                want = torch_predict(probs, labels, u, fit_det.qhat, kind, False, mondrian, gen)[1].cpu()
                T1 = 3 + 2 * (K + 1)  # every count before u_by_size, and the counts behind it
                counts_differ = int((got[:, :T1] != want[:, :T1]).sum() + (got[:, T1 + K + 1:] != want[:, T1 + K + 1:]).sum())
                sa, sb = alternating(lib, ref, a.reps)
                lines.append({"bench": "conformal.predict_sets", "rows": M, "K_real": K, "A": len(ALPHAS), "kind": kind, "randomized": rnd,
                              "mondrian": mondrian, "reps": a.reps, "library": sa, "eager_torch": sb,
                              "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                              "library_launches": LIBRARY_LAUNCHES["predict_sets"], "tally_counts_that_differ_deterministic": counts_differ,
                              "device": torch.cuda.get_device_name()})
                print(json.dumps(lines[-1]), flush=True)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
