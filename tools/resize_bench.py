#!/usr/bin/env python3
"""Raw cine windows -> model clips (pasn_cine_resize) against the host resize it replaces.  One JSON line per measurement:

    python tools/resize_bench.py [--n 32] [--steps 20] [--warmup 3] [--procs 16] [--out FILE] [--kernel-only]

For the reference video config (40 x 600 x 800 uint8 -> 32 x 112 x 112) and the X3D headline shape (24 x 600 x 800 -> 16 x 224 x 224),
N clips per batch, each its own source:

* ``host``: the scipy restatement of skimage's resize (tests/resize_cases.py) over a pool of ``--procs`` processes, clips/s;
* ``kernel``: one launch on a device batch (HIP events over back-to-back launches), clips/s and (raw bytes read + clip bytes written)
  / time as a fraction of the measured device-to-device copy rate;
* ``pipeline``: pinned host batch -> H2D copy -> launch, clips/s, as a fraction of a plain pinned H2D copy of the same bytes: the next
  batch's copy on a side stream overlapping the launch (``DPTrainer.staged``), and serialized on one stream (``us_serialized``).

``--kernel-only``: the kernel loop only (for ``rocprofv3 --kernel-trace --stats`` and counter runs)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from protoasnet_amd import data, resample  # noqa: E402

SHAPES = {"video": ((40, 600, 800), (32, 112, 112)), "x3d_headline": ((24, 600, 800), (16, 224, 224))}


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _windows(n, shape, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(n)]


def _batch(wins):
    return data.collate_raw_cines([dict(cine=w, window_start=0, window_end=w.shape[0], filename=f"c{i}") for i, w in enumerate(wins)])["cine"]


def _host_one(args):
    from resize_cases import skimage_resize

    w, so = args
    return skimage_resize(w, so).shape


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e-3  # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    d2d = float("nan")
    if not args.kernel_only:  # (counter runs profile the resize alone)
        big = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        big2 = torch.empty_like(big)
        d2d = 2 * big.numel() / _timed(lambda: big2.copy_(big), 10, 2)  # bytes read + written per second
        del big, big2
    for name, (si, so) in SHAPES.items():
        wins = _windows(args.n, si)
        host = _batch(wins).pin_memory()
        dev_batch = host.to(dev)
        raw_bytes = args.n * int(np.prod(si))
        out_bytes = args.n * int(np.prod(so)) * 4
        t_k = _timed(lambda: resample.resize_raw(dev_batch, so, torch.float32), args.steps, args.warmup)
        rec = {"bench": "kernel", "shape": name, "in": [args.n, *si], "out": [args.n, *so], "us": round(t_k * 1e6, 1),
               "clips_per_s": round(args.n / t_k, 1), "GB/s": round((raw_bytes + out_bytes) / t_k / 1e9, 1),
               "d2d_copy_GB/s": round(d2d / 1e9, 1), "frac_of_copy": round((raw_bytes + out_bytes) / t_k / d2d, 3)}
        _emit(rec, args.out)
        if args.kernel_only:
            continue
        staging = torch.empty(host.buffer.numel(), dtype=torch.uint8, device=dev)
        t_copy = _timed(lambda: staging.copy_(host.buffer, non_blocking=True), args.steps, args.warmup)
        t_serial = _timed(lambda: resample.resize_raw(host.to(dev, non_blocking=True), so, torch.float32), args.steps, args.warmup)
        # as DPTrainer.staged runs it: batch i + 1 uploads on a side stream while batch i is resized
        side, state = torch.cuda.Stream(), {}

        def upload():
            main = torch.cuda.current_stream()
            with torch.cuda.stream(side):
                d = host.to(dev, non_blocking=True)
                d.ready = torch.cuda.Event()
                d.ready.record(side)
            d.buffer.record_stream(main)
            return d

        def step():
            nxt = upload()
            resample.resize_raw(state.get("cur") or upload(), so, torch.float32)
            state["cur"] = nxt

        t_pipe = _timed(step, args.steps, args.warmup)
        rec = {"bench": "pipeline", "shape": name, "us": round(t_pipe * 1e6, 1), "clips_per_s": round(args.n / t_pipe, 1),
               "us_serialized": round(t_serial * 1e6, 1), "h2d_copy_us": round(t_copy * 1e6, 1),
               "h2d_GB/s": round(host.buffer.numel() / t_copy / 1e9, 1), "frac_of_copy": round(t_copy / t_pipe, 3)}
        _emit(rec, args.out)
        try:
            import scipy  # noqa: F401
        except ImportError:
            _emit({"bench": "host", "shape": name, "skipped": "scipy not importable"}, args.out)
            continue
        with ProcessPoolExecutor(args.procs) as ex:
            list(ex.map(_host_one, [(wins[0][:2], so)] * args.procs))  # start the workers
            t0 = time.perf_counter()
            list(ex.map(_host_one, [(w, so) for w in wins]))
            t_h = time.perf_counter() - t0
        _emit({"bench": "host", "shape": name, "procs": args.procs, "s_per_batch": round(t_h, 3), "clips_per_s": round(args.n / t_h, 1),
               "pipeline_over_host": round((args.n / t_pipe) / (args.n / t_h), 1)}, args.out)


if __name__ == "__main__":
    main()
