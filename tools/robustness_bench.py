#!/usr/bin/env python3
"""``robustness.corrupt`` and ``pasn_stability_stats`` (csrc/corrupt.hip) against the same products written in eager torch, and the cost of
one ``evaluate_robustness`` cell next to the two forwards it contains, on one GPU.

    python tools/robustness_bench.py [--reps 12] [--out profiles/robustness_bench.jsonl] [--no-cell]

Side A is the library: one launch per corrupted batch, at most three for the statistics.  Side B is eager torch on the same device, the
baseline a user would write without the library: the photometric stages as broadcast arithmetic, the blur as two ``conv2d`` over a
replicate-padded batch, the noise from ``randn`` (a different variate: the two sides are NOT compared value by value, only timed), the frame
hold as a ``gather``; the statistics as ``softmax`` / ``argmax`` / ``topk`` and a centred dot product per map.  Never the code under test.

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by a
synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of repeats.  No ratio
is fixed in advance.  ``hbm_fraction``: the corruption launch is bound by one read and one write per element; the bytes it must move over
its time, over the HBM peak below."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating, one, summary  # noqa: E402
from protoasnet_amd import _lib, robustness  # noqa: E402
from protoasnet_amd.data import ECHO_MEAN, ECHO_STD  # noqa: E402

CLIP = (32, 3, 16, 224, 224)   # the video clip batch
HEAD = dict(N=32, K=3, K_real=2, P=30, grid=(16, 7, 7), k=1)  # BASELINE config 4's head: X3D-S video, abstain class
HBM_PEAK = 8.0e12              # bytes / s, MI355X HBM3E
SEVERITY = 3


def eager_corrupt(x, d, seed):
    """The descriptor's stages in eager torch, fp32 arithmetic, the clip's dtype out."""
    N, C, T, H, W = x.shape
    dev = x.device
    if d.src_t is not None:
        idx = torch.as_tensor(d.src_t, device=dev).long().clamp(0, T - 1)
        x = x.gather(2, idx[:, None, :, None, None].expand(N, C, T, H, W))
        if d.taps is None and d.row_a is None and d.row_b is None and not d.sigma_add and not d.sigma_mul:
            return x
    v = x.float() * ECHO_STD + ECHO_MEAN
    if d.taps is not None:
        t = torch.as_tensor(d.taps, device=dev)
        R = (t.numel() - 1) // 2
        v = F.pad(v.reshape(N * C * T, 1, H, W), (R, R, R, R), mode="replicate")
        v = F.conv2d(F.conv2d(v, t.reshape(1, 1, 1, -1)), t.reshape(1, 1, -1, 1)).reshape(N, C, T, H, W)
    if d.row_a is not None:
        v = v * torch.as_tensor(d.row_a, device=dev)[:, None]
    if d.row_b is not None:
        v = v + torch.as_tensor(d.row_b, device=dev)[:, None]
    if d.sigma_add or d.sigma_mul:
        g = torch.Generator(device=dev).manual_seed(seed)
        z = torch.randn((N, 1, T, H, W), device=dev, generator=g)
        if d.sigma_add:
            v = v + d.sigma_add * z
        if d.sigma_mul:
            v = v + (d.sigma_mul * z) * v
    return ((v.clamp(0, 1) - ECHO_MEAN) / ECHO_STD).to(x.dtype)


def corrupt_lines(reps, dtype):
    out = []
    g = torch.Generator(device="cuda").manual_seed(1)
    x = ((torch.rand(CLIP, device="cuda", generator=g) ** 2 - ECHO_MEAN) / ECHO_STD).to(dtype)
    moved = 2 * x.numel() * x.element_size()
    for name in robustness.CORRUPTIONS:
        d = robustness.describe(name, SEVERITY, CLIP, seed=3)
        dd = robustness.Corruption(**{f: (None if getattr(d, f) is None else torch.as_tensor(getattr(d, f)).to("cuda"))
                                      for f in ("src_t", "taps", "row_a", "row_b")}, sigma_add=d.sigma_add, sigma_mul=d.sigma_mul)
        a, b = robustness.corrupt(x, dd, seed=3).float(), eager_corrupt(x, dd, 3).float()
        if name not in ("noise", "speckle"):  # the same product: within the rounding of a contracted / reordered fp32 expression
            assert float((a - b).abs().max()) <= (4e-2 if dtype == torch.bfloat16 else 1e-4), name
        del a, b
        sa, sb = alternating(lambda: robustness.corrupt(x, dd, seed=3).view(-1)[0].item(), lambda: eager_corrupt(x, dd, 3).view(-1)[0].item(), reps)
        out.append({"bench": "corrupt", "kind": name, "severity": SEVERITY, "shape": list(CLIP), "dtype": str(dtype)[6:], "reps": reps,
                    "library": sa, "eager_torch": sb, "ratio": round(sb["device_ms"] / sa["device_ms"], 2),
                    "library_GBps": round(moved / sa["device_ms"] / 1e6, 1), "hbm_fraction": round(moved / (sa["device_ms"] * 1e-3) / HBM_PEAK, 3),
                    "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    return out


def eager_stability(la, lb, sa, sb, oa, ob, K_real, G, k, m, grid):
    """The statistics of pasn_stability_stats in eager torch, fp64 where the library is: (clip (N, 4), pair (N, k, 4))."""
    N, P, S = oa.shape
    pa, pb = la[:, :K_real].double().softmax(1), lb[:, :K_real].double().softmax(1)
    pred = la[:, :K_real].argmax(1)
    block = pred[:, None] * G + torch.arange(G, device=la.device)
    sel_a = block.gather(1, sa.gather(1, block).topk(k, dim=1).indices)
    sel_b = block.gather(1, sb.gather(1, block).topk(k, dim=1).indices)
    overlap = (sel_a[:, :, None] == sel_b[:, None, :]).any(2).double().mean(1)
    clip = torch.stack([(lb[:, :K_real].argmax(1) != pred).double(), 0.5 * (pa - pb).abs().sum(1),
                        (pa - pb).gather(1, pred[:, None])[:, 0], overlap], 1)
    ma = oa.gather(1, sel_a[:, :, None].expand(N, k, S)).double()
    mb = ob.gather(1, sel_a[:, :, None].expand(N, k, S)).double()
    ca, cb = ma - ma.mean(2, keepdim=True), mb - mb.mean(2, keepdim=True)
    corr = (ca * cb).sum(2) / ((ca * ca).sum(2) * (cb * cb).sum(2)).sqrt()
    ta = torch.zeros_like(ma, dtype=torch.bool).scatter_(2, ma.topk(m, dim=2).indices, True)
    tb = torch.zeros_like(mb, dtype=torch.bool).scatter_(2, mb.topk(m, dim=2).indices, True)
    inter = (ta & tb).sum(2).double()
    ia, ib = ma.argmax(2), mb.argmax(2)
    HW = grid[1] * grid[2]
    d2 = (ia // HW - ib // HW) ** 2 + (ia % HW // grid[2] - ib % HW // grid[2]) ** 2 + (ia % grid[2] - ib % grid[2]) ** 2
    shift = d2.double().sqrt() / float(sum((v - 1) ** 2 for v in grid)) ** 0.5
    dsim = sb.gather(1, sel_a).double() - sa.gather(1, sel_a).double()
    return clip, torch.stack([dsim, corr, inter / (2 * m - inter), shift], 2)


def stability_line(reps):
    N, K, K_real, P, grid, k = (HEAD[f] for f in ("N", "K", "K_real", "P", "grid", "k"))
    S = grid[0] * grid[1] * grid[2]
    m = robustness.top_count(0.1, S)
    g = torch.Generator(device="cuda").manual_seed(2)
    la = torch.randn((N, K), device="cuda", generator=g)
    lb = la + 0.5 * torch.randn((N, K), device="cuda", generator=g)
    sa = torch.rand((N, P), device="cuda", generator=g)
    sb = (sa + 0.05 * torch.randn((N, P), device="cuda", generator=g)).contiguous()
    oa = torch.rand((N, P, S), device="cuda", generator=g)
    ob = (oa + 0.1 * torch.randn((N, P, S), device="cuda", generator=g)).contiguous()
    clip = torch.empty((N, 4), dtype=torch.float64, device="cuda")
    sel = torch.empty((N, k), dtype=torch.int32, device="cuda")
    pair = torch.empty((N, k, 4), dtype=torch.float64, device="cuda")
    lib = _lib.lib()

    def library():
        _lib.check(lib.pasn_stability_stats(la.data_ptr(), lb.data_ptr(), sa.data_ptr(), sb.data_ptr(), oa.data_ptr(), ob.data_ptr(), 0, N, K,
                                            K_real, P, grid[0], grid[1], grid[2], k, m, clip.data_ptr(), 0, sel.data_ptr(), pair.data_ptr(), 0,
                                            _lib.current_stream()))
        return pair[0, 0, 0].item()

    library()
    e_clip, e_pair = eager_stability(la, lb, sa, sb, oa, ob, K_real, P // K, k, m, grid)
    assert float((clip - e_clip).abs().max()) <= 1e-9 and float((pair - e_pair).abs().max()) <= 1e-9  # (continuous random maps: no ties)
    ta, tb = alternating(library, lambda: eager_stability(la, lb, sa, sb, oa, ob, K_real, P // K, k, m, grid)[1][0, 0, 0].item(), reps)
    line = {"bench": "stability_stats", "clips": N, "K": K, "P": P, "grid": list(grid), "select": k, "top_voxels": m, "reps": reps, "library": ta,
            "eager_torch": tb, "ratio": round(tb["device_ms"] / ta["device_ms"], 2), "device": torch.cuda.get_device_name()}
    print(json.dumps(line), flush=True)
    return [line]


def cell_line(reps):
    """One (corruption, severity) cell of a sweep -- corrupt, the corrupted push_forward, the statistics; the clean push_forward is shared
    by the cells of a batch and is counted here too -- beside two plain push_forwards of the same batch, bf16 compute."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from protoasnet_amd import synth
    from util import CFG_VIDEO_X3D, synth_model

    m = synth_model(CFG_VIDEO_X3D).to("cuda").eval()
    m.set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips(CLIP).to("cuda")
    out = []
    for name in ("noise", "blur"):
        def cell():
            return float(m.robustness(x, name, SEVERITY, seed=1).corr[0, 0])

        def forwards():
            with torch.no_grad():
                m.push_forward(x)
                return float(m.push_forward(x)[3][0, 0])

        for _ in range(2):
            cell(), forwards()
        tc, tf = [], []
        for _ in range(reps):
            tc.append(one(cell))
            tf.append(one(forwards))
        sc, sf = summary(tc), summary(tf)
        out.append({"bench": "evaluate_robustness cell", "kind": name, "severity": SEVERITY, "shape": list(CLIP), "compute": "bfloat16", "reps": reps,
                    "cell": sc, "two_push_forwards": sf, "bookkeeping_ms": round(sc["device_ms"] - sf["device_ms"], 3),
                    "bookkeeping_share": round((sc["device_ms"] - sf["device_ms"]) / sf["device_ms"], 3), "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-cell", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robustness_bench needs the GPU: a timing taken elsewhere says nothing")
    lines = corrupt_lines(a.reps, torch.bfloat16) + corrupt_lines(a.reps, torch.float32) + stability_line(a.reps)
    if not a.no_cell:
        lines += cell_line(a.reps)
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
