#!/usr/bin/env python3
"""Throughput of the local-explanation map kernels (pasn_explain_maps: stats + write launch) against torch on the device.

    python tools/explain_bench.py [--reps 20] [--out profiles/explain_bench.jsonl]

Per shape: device events around each call, every shape warmed first, the median of --reps calls.  Written bytes per second are the
output bytes over that time, against the 8 TB/s HBM peak.  The torch column computes the same product with F.interpolate + amin / amax
+ division (+ uint8 cast; + the overlay gather) -- a baseline only, not a code path of the package.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import explain  # noqa: E402

PEAK = 8.0e12


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


def torch_maps(occ, sel, out, kind, lut=None, src=None, alpha=0.3, mean=0.099, std=0.171):
    N, P = occ.shape[:2]
    if sel is not None:
        occ = torch.gather(occ, 1, sel.long().view(N, -1, 1, 1, 1).expand(-1, -1, *occ.shape[2:]))
    k = occ.shape[1]
    u = F.interpolate(occ.reshape(N * k, 1, *occ.shape[2:]), size=out, mode="trilinear")
    r = u - u.amin(dim=(2, 3, 4), keepdim=True)
    v = r / (r.amax(dim=(2, 3, 4), keepdim=True) + 1e-7)
    if kind == "uint8" or lut is not None:
        q = (v * 255).to(torch.uint8)
        if lut is not None:
            img = (src * std + mean).repeat_interleave(k, 0).movedim(1, -1)
            if img.shape[-1] == 1:
                img = img.expand(*img.shape[:-1], 3)
            return img + alpha * lut[q[:, 0].long()]
        return q
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = "cuda"
    rng = np.random.default_rng(0)
    lut = torch.from_numpy(rng.random((256, 3)).astype(np.float32)).to(dev)
    rows = []
    shapes = [  # name, N, P, grid, out, maps, k (None = all P), overlay
        ("r2p1d_video_fp32", 8, 40, (8, 14, 14), (32, 112, 112), "float", None, False),
        ("r2p1d_video_uint8", 8, 40, (8, 14, 14), (32, 112, 112), "uint8", None, False),
        ("r2p1d_video_overlay_k3", 8, 40, (8, 14, 14), (32, 112, 112), None, 3, True),
        ("x3d_s_cfg2_uint8", 32, 30, (16, 7, 7), (16, 224, 224), "uint8", None, False),
    ]
    for name, N, P, grid, out, maps, k, ovl in shapes:
        occ = torch.from_numpy(np.abs(rng.standard_normal((N, P) + grid)).astype(np.float32)).to(dev)
        sel = torch.from_numpy(np.stack([rng.permutation(P)[:k] for _ in range(N)]).astype(np.int32)).to(dev) if k else None
        src = torch.from_numpy(rng.standard_normal((N, 1) + out).astype(np.float32)).to(dev) if ovl else None
        kk = k or P
        vox = N * kk * int(np.prod(out))
        nbytes = vox * ((4 if maps == "float" else 1 if maps == "uint8" else 0) + (12 if ovl else 0))
        hip = timed(lambda: explain._maps_launch(occ, sel, kk, out, maps, lut if ovl else None, src, 0.3, 0.099, 0.171), a.reps)
        ref = timed(lambda: torch_maps(occ, sel, out, maps, lut if ovl else None, src), a.reps)
        row = {"shape": name, "N": N, "P": P, "k": kk, "grid": list(grid), "out": list(out), "maps": maps, "overlay": ovl,
               "bytes_written": nbytes, "hip_ms": round(hip * 1e3, 4), "hip_TBps": round(nbytes / hip / 1e12, 3),
               "hip_frac_of_peak": round(nbytes / hip / PEAK, 3), "torch_ms": round(ref * 1e3, 4), "speedup_vs_torch": round(ref / hip, 2),
               "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del occ, sel, src
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
