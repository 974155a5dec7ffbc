#!/usr/bin/env python3
"""``calibration.reliability`` / ``calibration.fit_temperature`` (csrc/calibration.hip) against the same product in eager torch, on one GPU.

    python tools/calibration_bench.py [--reps 20] [--out profiles/calibration_bench.jsonl] [--trainer]

Sizes: M = 10 000 and 100 000 clip rows, K_real = 4, 15 bins, B = 0 and 1000 replicates; the unit is the clip (G = M) or the cine (10
clips per cine, interleaved).  Side A is the library: two launches per chunk of counts (plus the draw) whatever B is, one read.  Side B
computes the same arrays per replicate in eager torch: ``bucketize`` once per call, then per chunk of replicates (sized to a fixed number
of (replicate, row, class) elements) ``randint`` + ``bincount`` for the counts and one ``scatter_add`` per histogram, fp64 throughout.  Its
draws are torch's, not Philox's, so the two sides are compared on the point row.  The fit: the library's fixed 52 launches against the
same safeguarded Newton with torch reductions and a host read per step.

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by its own
synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of repeats.  No
ratio is fixed in advance.  ``--trainer``: what ``evaluate_selective(calibration=15)`` adds on the synthetic split of the tests."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating  # noqa: E402
from protoasnet_amd import calibration, selective  # noqa: E402

K, N_BINS = 4, 15
CHUNK_ELEMS = 8_000_000  # (replicates x rows x classes) per chunk of the torch side
FLT_MIN = 1.1754943508222875e-38


def case(M, cines, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    key_id = torch.randperm(M, generator=g) % cines
    labels = (key_id * 7919) % K
    logits = torch.rand(M, K, generator=g) * 8 - 4
    logits[torch.arange(M), labels] += 2.0
    return logits.to(dev), torch.softmax(logits, 1).to(dev), labels.to(torch.int32).to(dev), selective.build_groups(key_id.tolist())


# ---- side B: eager torch -----------------------------------------------------------------------------------------------------------------
def torch_reliability(probs, labels, groups, n_bins, B, gen):
    """stats (B + 1, 6) fp64 in calibration.STAT_NAMES' order, row B the point estimate (every row valid)."""
    import numpy as np

    M, Kc = probs.shape
    dev = probs.device
    p, lab = probs.double(), labels.long()
    conf, pred = p.max(1)
    hit = (pred == lab).double()
    edges = torch.arange(1, n_bins, device=dev, dtype=torch.float64) / n_bins
    bins = torch.bucketize(conf, edges, right=True)  # [lo, hi)
    cbins = (torch.bucketize(p, edges, right=True) + torch.arange(Kc, device=dev) * n_bins).flatten()
    onehot = torch.nn.functional.one_hot(lab, Kc).double()
    brier_i = ((p - onehot) ** 2).sum(1)
    nll_i = -torch.log(p.gather(1, lab[:, None])[:, 0].clamp(min=FLT_MIN))
    if groups is None:
        G, gid = M, torch.arange(M, device=dev)
    else:
        G = len(groups[0]) - 1
        gid = torch.empty(M, dtype=torch.int64, device=dev)
        gid[torch.from_numpy(groups[1]).to(dev).long()] = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(np.diff(groups[0])).to(dev))
    out = []
    step = max(1, CHUNK_ELEMS // (M * Kc))
    for b0 in range(0, B + 1, step):
        n = min(step, B + 1 - b0)
        draws = torch.randint(0, G, (n, G), device=dev, generator=gen)
        counts = torch.bincount((draws + torch.arange(n, device=dev)[:, None] * G).flatten(), minlength=n * G).view(n, G)
        if b0 + n == B + 1:
            counts[-1] = 1  # the point row
        w = counts[:, gid].double()

        def hist(index, values, size):
            return torch.zeros(n, size, dtype=torch.float64, device=dev).scatter_add_(1, index.expand(n, -1), values)

        nj, hj, cj = hist(bins, w, n_bins), hist(bins, w * hit, n_bins), hist(bins, w * conf, n_bins)
        wk = w[:, :, None].expand(n, M, Kc).reshape(n, M * Kc)
        cpos, cconf = hist(cbins, wk * onehot.flatten(), Kc * n_bins), hist(cbins, wk * p.flatten(), Kc * n_bins)
        W = nj.sum(1)
        gap = cj - hj
        mce = torch.where(nj > 0, gap.abs() / nj.clamp(min=1), torch.zeros_like(gap)).amax(1)
        out.append(torch.stack([gap.abs().sum(1) / W, mce, (cpos - cconf).abs().sum(1) / W / Kc, (w * brier_i).sum(1) / W, (w * nll_i).sum(1) / W,
                                gap.sum(1) / W], 1))
    return torch.cat(out)


def torch_fit(logits, labels, steps=48):
    """The header's safeguarded Newton with torch reductions: one host read per evaluation."""
    z = logits.double()
    d = z - z.amax(1, keepdim=True)
    dl = d.gather(1, labels.long()[:, None])[:, 0]

    def moments(beta):
        e = torch.exp(beta * d)
        S = e.sum(1)
        mean = (e * d).sum(1) / S
        var = (e * (d - mean[:, None]) ** 2).sum(1) / S
        return torch.stack([(torch.log(S) - beta * dl).sum(), (mean - dl).sum(), var.sum()]).tolist()  # the host read

    lo, hi, beta = 1 / 64, 64.0, 1.0
    g1 = moments(1.0)[0]
    if moments(lo)[1] >= 0 or moments(hi)[1] <= 0:
        raise RuntimeError("the benchmark's case has an interior root")
    for _ in range(steps):
        _, d1, d2 = moments(beta)
        lo, hi = (lo, beta) if d1 > 0 else (beta, hi) if d1 < 0 else (beta, beta)
        nt = beta - d1 / d2 if d2 > 0 else lo
        beta = nt if lo < nt < hi else 0.5 * (lo + hi)
    return beta, g1 / len(dl), moments(beta)[0] / len(dl)


def trainer_lines(reps):
    """``evaluate_selective`` on the synthetic split of the tests with and without ``calibration=15``."""
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
        sa, sb = alternating(lambda: t.evaluate_selective("test", level=level, calibration=N_BINS), lambda: t.evaluate_selective("test", level=level), reps)
        out.append({"bench": "DPTrainer.evaluate_selective", "level": level, "clip_rows": 12, "cines": 3, "reps": reps, "calibration_15": sa,
                    "calibration_0": sb, "added_device_ms": round(sa["device_ms"] - sb["device_ms"], 3), "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    sa, _ = alternating(lambda: t.fit_temperature("val"), lambda: None, reps)
    out.append({"bench": "DPTrainer.fit_temperature", "clip_rows": 12, "reps": reps, "fit": sa, "device": torch.cuda.get_device_name()})
    print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=0, help="repeats of the pairs whose torch side takes seconds (0: --reps)")
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--replicates", default="0,1000")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--library-only", action="store_true", help="the library side alone, a few calls: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for M in (int(x) for x in a.sizes.split(",")):
        logits, probs, labels, groups = case(M, M // 10, dev)
        for unit in ("clip", "cine"):
            gr = None if unit == "clip" else groups[:2]
            for B in (int(x) for x in a.replicates.split(",")):
                if unit == "cine" and B == 0:
                    continue  # without replicates the unit does not enter
                lib = lambda: calibration.reliability(probs, labels, N_BINS, None, gr, B, seed=1).stats.cpu()  # noqa: E731
                ref = lambda: torch_reliability(probs, labels, gr, N_BINS, B, gen).cpu()  # noqa: E731
                if a.library_only:
                    for _ in range(3):
                        lib()
                    continue
                point = float((lib()[B] - ref()[B]).abs().max())
                reps = a.torch_reps if a.torch_reps and M * B >= 100_000_000 else a.reps
                sa, sb = alternating(lib, ref, reps, warm=3 if reps >= 10 else 1)
                lines.append({"bench": "calibration.reliability", "unit": unit, "clip_rows": M, "groups": M if gr is None else len(gr[0]) - 1,
                              "K_real": K, "n_bins": N_BINS, "B": B, "reps": reps, "library": sa, "eager_torch": sb,
                              "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4),
                              "max_abs_difference_of_the_point_rows": point, "device": torch.cuda.get_device_name()})
                print(json.dumps(lines[-1]), flush=True)
        lib = lambda: calibration.fit_temperature(logits, labels, K).read()  # noqa: E731
        ref = lambda: torch_fit(logits, labels)  # noqa: E731
        if a.library_only:
            for _ in range(3):
                lib()
            continue
        ca, cb = lib(), ref()
        sa, sb = alternating(lib, ref, a.reps)
        lines.append({"bench": "calibration.fit_temperature", "clip_rows": M, "K_real": K, "reps": a.reps, "library": sa, "eager_torch": sb,
                      "library_over_torch_device": round(sa["device_ms"] / sb["device_ms"], 4), "beta": ca["beta"], "status": ca["status"],
                      "relative_difference_of_beta": abs(ca["beta"] - cb[0]) / cb[0], "device": torch.cuda.get_device_name()})
        print(json.dumps(lines[-1]), flush=True)
    if a.trainer and not a.library_only:
        lines += trainer_lines(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
