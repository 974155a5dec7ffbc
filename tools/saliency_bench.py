#!/usr/bin/env python3
"""``saliency.masked_clips``, ``saliency.saliency_maps`` and the whole ``saliency.rise`` (csrc/rise.hip) against the same product in
eager torch, at the video configuration, on one GPU.

    python tools/saliency_bench.py [--reps 10] [--out profiles/saliency_bench.jsonl] [--no-rise]

One clip of 3 x 16 x 224 x 224, bf16, grid (4, 7, 7).  Side A is the library: one launch per chunk of 64 masked clips; the lattices of all
masks in one launch, then one launch per group of four maps and one that quantises.  Side B is eager torch on the same device: a random
0 / 1 lattice -> ``F.interpolate(mode="trilinear")`` -> one shifted crop per mask -> a broadcast multiply for the clips; for the maps the
masks of 128 masks at a time (they do not fit otherwise: 2048 fp32 masks are 6.6 GB), ``einsum`` for the sums, min-max -> uint8.  The two
sides compute the same PRODUCT, not the same numbers: side B's masks come from torch's generator, and its sums run in whatever order
``einsum`` picks.

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by a
synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of repeats.  No
ratio is fixed in advance.  ``share_of_hbm_peak_on_output``: the bytes of the masked clips over the time, over the 8.0 TB/s of the
specification (a float4 copy reaches 6.3 TB/s).  The ``rise`` lines time the whole call on a synth X3D-S head-B model in bf16 next to the
forwards of the same number of 64-clip batches alone."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating, one, summary  # noqa: E402
from protoasnet_amd import saliency  # noqa: E402

C, SHAPE, GRID, P, CHUNK = 3, (16, 224, 224), (4, 7, 7), 0.5, 64
HBM_PEAK = 8.0e12  # bytes / s, the specification


def eager_masks(n, gen):
    """(n, T, H, W) fp32: the eager formulation of n masks."""
    cells = tuple(-(-s // g) for s, g in zip(SHAPE, GRID))
    low = (torch.rand((n, 1) + tuple(g + 2 for g in GRID), device="cuda", generator=gen) < P).float()
    up = F.interpolate(low, size=tuple((g + 2) * c for g, c in zip(GRID, cells)), mode="trilinear", align_corners=False)[:, 0]
    sh = [torch.randint(0, c, (n,), generator=gen, device="cuda").tolist() for c in cells]  # (one read: the crops need host integers)
    return torch.stack([up[i, sh[0][i]:sh[0][i] + SHAPE[0], sh[1][i]:sh[1][i] + SHAPE[1], sh[2][i]:sh[2][i] + SHAPE[2]] for i in range(n)])


def eager_apply(x, gen):
    return x[:, None] * eager_masks(CHUNK, gen)[None, :, None].to(x.dtype)


def eager_maps(scores, gen, step=128):
    M, k = scores.shape[1:]
    V = SHAPE[0] * SHAPE[1] * SHAPE[2]
    S, cov = torch.zeros((k, V), dtype=torch.float64, device="cuda"), torch.zeros(V, dtype=torch.float64, device="cuda")
    for m0 in range(0, M, step):
        mk = eager_masks(min(step, M - m0), gen).reshape(-1, V)
        S += torch.einsum("mk,mv->kv", scores[0, m0:m0 + step], mk).double()
        cov += mk.sum(0).double()
    sal = (S / cov).float()
    lo, hi = sal.amin(1, keepdim=True), sal.amax(1, keepdim=True)
    return (255.0 * ((sal - lo) / ((hi - lo) + 1e-7))).to(torch.uint8)


def kernel_lines(reps):
    out = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    V = SHAPE[0] * SHAPE[1] * SHAPE[2]
    x = torch.randn((1, C) + SHAPE, device="cuda", generator=gen).to(torch.bfloat16)
    sa, sb = alternating(lambda: saliency.masked_clips(x, GRID, P, 0, 0, 0, CHUNK).view(-1)[0].item(), lambda: eager_apply(x, gen).view(-1)[0].item(), reps)
    moved = CHUNK * C * V * x.element_size()
    out.append({"bench": "masked_clips", "clips": 1, "masks_in_chunk": CHUNK, "channels": C, "grid": list(GRID), "clip": list(SHAPE), "dtype": "bfloat16",
                "reps": reps, "library": sa, "eager_torch": sb, "ratio": round(sb["device_ms"] / sa["device_ms"], 2),
                "library_GBps_of_output": round(moved / sa["device_ms"] / 1e6, 1),
                "share_of_hbm_peak_on_output": round(moved / (sa["device_ms"] * 1e-3) / HBM_PEAK, 3), "device": torch.cuda.get_device_name()})
    print(json.dumps(out[-1]), flush=True)
    for M in (512, 2048):
        for k in (1, 3):
            scores = torch.rand((1, M, k), device="cuda", generator=gen)
            few = max(3, reps // 3)  # (the eager side takes seconds)
            sa, sb = alternating(lambda: saliency.saliency_maps(scores, SHAPE, GRID, P, saliency=False)[1].view(-1)[0].item(),
                                 lambda: eager_maps(scores, gen).view(-1)[0].item(), few, warm=2)
            out.append({"bench": "saliency_maps", "clips": 1, "masks": M, "maps_per_clip": k, "grid": list(GRID), "clip": list(SHAPE), "reps": few,
                        "library": sa, "eager_torch": sb, "ratio": round(sb["device_ms"] / sa["device_ms"], 2),
                        "library_voxel_masks_per_us": round(M * V / (sa["device_ms"] * 1e3), 1), "device": torch.cuda.get_device_name()})
            print(json.dumps(out[-1]), flush=True)
    return out


def rise_lines(reps):
    """The whole call beside the model's forwards alone: what RISE costs on top of running the model M times."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from protoasnet_amd import synth
    from util import CFG_VIDEO_X3D, synth_model

    m = synth_model(CFG_VIDEO_X3D).to("cuda").eval()
    m.set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips((1, C) + SHAPE).to("cuda")
    batch = saliency.masked_clips(x, GRID, P, 0, 0, 0, CHUNK)[0]
    out = []
    for M in (512, 2048):
        def whole():
            return float(m.rise(x, select=1, masks=M, max_batch=CHUNK).saliency.view(-1)[0])

        def forwards():
            with torch.no_grad():
                for _ in range(M // CHUNK):
                    r = m(batch)
            return float(r[0][0, 0])

        few = max(3, reps // 3)
        sa, sb = alternating(whole, forwards, few, warm=1)
        out.append({"bench": "rise", "model": "x3d_s head B, bf16", "clips": 1, "masks": M, "max_batch": CHUNK, "reps": few, "rise": sa,
                    "forwards_alone": sb, "share_not_forward": round(1.0 - sb["device_ms"] / sa["device_ms"], 3),
                    "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-rise", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    lines = kernel_lines(a.reps)
    if not a.no_rise:
        lines += rise_lines(a.reps)
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
