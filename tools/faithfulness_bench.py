#!/usr/bin/env python3
"""``faithfulness.removal_steps`` + ``faithfulness.perturb`` (csrc/perturb.hip) against the eager ``argsort`` / ``where`` formulation, and the
whole deletion + insertion curve, on one GPU.

    python tools/faithfulness_bench.py [--reps 12] [--out profiles/faithfulness_bench.jsonl] [--no-curves] [--trace]

Side A is the library: three launches for the step volume of N k maps, one launch per chunk of perturbed clips.  Side B is eager torch on
the same device: per map one stable ``argsort`` of the int64 key ``(255 - level) V + index`` (the (level descending, index ascending) order),
a scatter of ``arange`` for the positions, ``searchsorted`` for the steps, then per step one ``torch.where`` over the broadcast clip.  Both
sides produce the same tensors (checked once, bit for bit, before timing).

Timing as in tools/bootstrap_bench.py: 3 warm-up calls of each side, alternating A/B repeats, each between two events and ended by a
synchronising read; ``device_ms`` is the median, ``block_spread_ms`` the range of the medians of four consecutive blocks of repeats.  No ratio
is fixed in advance.  The curve lines time ``perturbation_curves(mode="both")`` of synth models at the X3D-S and R(2+1)D clip shapes, next to
one clean forward of the same clips.  ``--trace``: the library side alone at the X3D-S clip shape, three calls of ``removal_steps`` and of
``perturb`` in fp32 and bf16, for a kernel trace taken in a run of its own."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bootstrap_bench import alternating, one, summary  # noqa: E402
from protoasnet_amd import faithfulness  # noqa: E402

# (name, clips, channels, grid, maps per clip, steps per chunk): the perturbed chunk is N k Sc clips
SHAPES = (("x3d_s", 4, 3, (16, 224, 224), 1, 11), ("r2p1d", 4, 3, (32, 112, 112), 1, 11), ("image", 8, 3, (1, 224, 224), 2, 11))


def eager_steps(maps, counts):
    N, k = maps.shape[:2]
    V = maps[0, 0].numel()
    flat = maps.reshape(N * k, V)
    key = (255 - flat.long()) * V + torch.arange(V, device=maps.device)
    order = torch.argsort(key, dim=1)
    pos = torch.empty_like(order)
    pos.scatter_(1, order, torch.arange(V, device=maps.device).expand(N * k, V))
    return torch.searchsorted(counts.long(), pos, right=True).to(torch.uint8).reshape(maps.shape)


def eager_perturb(x, steps, ids, mode, fill):
    base = torch.full_like(x, fill)[:, None, None]
    touched = steps[:, :, None, None] <= ids.to(torch.uint8).reshape(1, 1, -1, *([1] * (steps.dim() - 1)))
    return torch.where(touched if mode == 1 else ~touched, x[:, None, None], base)


def kernel_lines(reps, dtype):
    out = []
    for name, N, C, grid, k, Sc in SHAPES:
        V = grid[0] * grid[1] * grid[2]
        g = torch.Generator(device="cuda").manual_seed(1)
        low = torch.rand((N, k, max(1, grid[0] // 4), 7, 7), device="cuda", generator=g)  # a smooth map, as the occurrence maps are
        maps = (torch.nn.functional.interpolate(low, size=grid, mode="trilinear") * 255).to(torch.uint8)
        x = torch.randn((N, C) + grid, device="cuda", generator=g).to(dtype)
        counts = torch.tensor(faithfulness.step_counts(V, 10), dtype=torch.int32, device="cuda")
        ids = torch.arange(Sc, dtype=torch.int32, device="cuda")
        a_steps, b_steps = faithfulness.removal_steps(maps, counts), eager_steps(maps, counts)
        assert torch.equal(a_steps, b_steps), name
        assert torch.equal(faithfulness.perturb(x, a_steps, ids, 0).view(torch.uint8), eager_perturb(x, b_steps, ids, 0, 0.0).view(torch.uint8)), name
        pairs = {
            "removal_steps": (lambda: faithfulness.removal_steps(maps, counts)[0, 0, 0, 0, 0].item(), lambda: eager_steps(maps, counts)[0, 0, 0, 0, 0].item()),
            "perturb": (lambda: faithfulness.perturb(x, a_steps, ids, 0).view(-1)[0].item(), lambda: eager_perturb(x, b_steps, ids, 0, 0.0).view(-1)[0].item()),
        }
        for what, (fa, fb) in pairs.items():
            sa, sb = alternating(fa, fb, reps)
            moved = N * k * V * 2 if what == "removal_steps" else N * k * Sc * C * V * x.element_size()
            out.append({"bench": what, "shape": name, "clips": N, "maps_per_clip": k, "grid": list(grid), "steps_in_chunk": Sc, "dtype": str(dtype)[6:],
                        "reps": reps, "library": sa, "eager_torch": sb, "ratio": round(sb["device_ms"] / sa["device_ms"], 2),
                        "library_GBps_of_output": round(moved / sa["device_ms"] / 1e6, 1), "device": torch.cuda.get_device_name()})
            print(json.dumps(out[-1]), flush=True)
    return out


def curve_lines(reps):
    """The whole curve (one explain, one removal_steps, the forwards of 2 x 11 perturbed copies per clip, two curve launches) beside one
    clean forward of the same clips, bf16 compute."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from protoasnet_amd import synth
    from util import CFG_VIDEO_R2P1D, CFG_VIDEO_X3D, synth_model

    out = []
    for name, cfg, shape in (("x3d_s", CFG_VIDEO_X3D, (4, 3, 16, 224, 224)), ("r2p1d", CFG_VIDEO_R2P1D, (4, 3, 32, 112, 112))):
        m = synth_model(cfg).to("cuda").eval()
        m.set_compute_dtype(torch.bfloat16)
        x = synth.echo_clips(shape).to("cuda")

        def curve():
            return float(m.faithfulness(x, select=1, steps=10, mode="both", max_batch=44).deletion.auc_prob[0, 0])

        def forward():
            with torch.no_grad():
                return float(m(x)[0][0, 0])

        for _ in range(2):
            curve(), forward()
        tc, tf = [one(curve) for _ in range(reps)], [one(forward) for _ in range(reps)]
        out.append({"bench": "perturbation_curves both", "shape": name, "clips": shape[0], "steps": 10, "select": 1, "max_batch": 44,
                    "perturbed_clips_forwarded": shape[0] * 11 * 2, "reps": reps, "curves": summary(tc), "clean_forward": summary(tf),
                    "device": torch.cuda.get_device_name()})
        print(json.dumps(out[-1]), flush=True)
    return out


def trace_calls():
    name, N, C, grid, k, Sc = SHAPES[0]
    V = grid[0] * grid[1] * grid[2]
    g = torch.Generator(device="cuda").manual_seed(1)
    low = torch.rand((N, k, 4, 7, 7), device="cuda", generator=g)
    maps = (torch.nn.functional.interpolate(low, size=grid, mode="trilinear") * 255).to(torch.uint8)
    counts = torch.tensor(faithfulness.step_counts(V, 10), dtype=torch.int32, device="cuda")
    ids = torch.arange(Sc, dtype=torch.int32, device="cuda")
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn((N, C) + grid, device="cuda", generator=g).to(dtype)
        for _ in range(3):
            steps = faithfulness.removal_steps(maps, counts)
            faithfulness.perturb(x, steps, ids, 0)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-curves", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        return trace_calls()
    lines = kernel_lines(a.reps, torch.float32) + kernel_lines(a.reps, torch.bfloat16)[1::2]  # (the step volume does not depend on the dtype)
    if not a.no_curves:
        lines += curve_lines(a.reps)
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
