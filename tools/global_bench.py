#!/usr/bin/env python3
"""The global-explanation scan (csrc/global_explain.hip, global_explain.nearest_clips) on one GPU.

    python tools/global_bench.py [--reps 200] [--blocks 3] [--clips 10000] [--k 10] [--out profiles/global_explain_bench.jsonl]

At the sweep shape of BASELINE config 4 (batches of 32 clips, X3D-S video head: P = 30 prototypes, K = 3 logits, occurrence maps
16 x 7 x 7):

1. one batch's bookkeeping alone -- pasn_topk_xproto_update + the three pasn_topk_gather calls (occurrence maps, logits, labels) +
   pasn_proto_class_stats -- against the eager torch formulation of the same step on the same device (concatenate the batch onto the
   running rows, stable sort, gather the payloads, one-hot matmul for the class sums): device time (events around the call, median),
   host wall time per call and launches per call (torch profiler);
2. the whole sweep over --clips synthetic clips, nearest_clips(k) against push_prototypes over the same loader on the same build,
   alternating blocks (A B A B ...) in one process: the spread of the push blocks is the yardstick for the difference.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from protoasnet_amd import _lib, global_explain, model_builder, push, synth  # noqa: E402

B, P, K, MAP = 32, 30, 3, (1, 16, 7, 7)


def batches(n, dev):
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(n):
        out.append((torch.rand(B, P, generator=g).to(dev), torch.randint(0, K, (B,), generator=g).to(dev),
                    torch.rand((B, P) + MAP, generator=g).to(dev), torch.randn(B, K, generator=g).to(dev)))
    return out


def make_calls(k, dev):
    pool = batches(16, dev)
    proto_class = (torch.arange(P) // (P // K)).to(torch.int32).to(dev)
    mask = push.xproto_class_mask(P, K, True, False).to(dev)
    lib = _lib.lib()
    st = global_explain.TopKState(P, k, dev)
    csum = torch.zeros((P, K), dtype=torch.float64, device=dev)
    ccnt = torch.zeros((K,), dtype=torch.int64, device=dev)
    step = [0]

    def run_hip():
        d, lab, occ, lg = pool[step[0] % len(pool)]
        base = step[0] * B
        step[0] += 1
        st.update(d, lab, proto_class, mask, base)
        st.gather("occ", occ, True, base)
        st.gather("logits", lg, False, base)
        st.gather("labels", lab, False, base, fill=-1)
        _lib.check(lib.pasn_proto_class_stats(d.data_ptr(), lab.data_ptr(), B, P, K, csum.data_ptr(), ccnt.data_ptr(), _lib.current_stream()))

    S = int(torch.tensor(MAP).prod())
    e = {"d": torch.full((P, k), float("inf"), device=dev), "i": torch.full((P, k), -1, dtype=torch.int64, device=dev),
         "occ": torch.zeros((P, k, S), device=dev), "lg": torch.zeros((P, k, K), device=dev),
         "lab": torch.full((P, k), -1, dtype=torch.int64, device=dev), "sum": torch.zeros((K, P), dtype=torch.float64, device=dev),
         "cnt": torch.zeros((K,), dtype=torch.int64, device=dev)}
    estep = [0]
    pc64, inf = proto_class.long(), torch.tensor(float("inf"), device=dev)

    def run_eager():
        d, lab, occ, lg = pool[estep[0] % len(pool)]
        base = estep[0] * B
        estep[0] += 1
        out = mask.bool()[:, None] & (lab[None, :] != pc64[:, None])                       # (P, B) not eligible
        all_d = torch.cat([e["d"], torch.where(out, inf, d.t())], dim=1)
        all_i = torch.cat([e["i"], torch.where(out, -1, (base + torch.arange(B, device=dev))[None, :].expand(P, B))], dim=1)
        v, o = torch.sort(all_d, dim=1, stable=True)  # the running row comes first and holds the lower indices: (distance, index) order
        o = o[:, :k]
        e["d"], e["i"] = v[:, :k], all_i.gather(1, o)
        e["occ"] = torch.cat([e["occ"], occ.reshape(B, P, S).transpose(0, 1)], dim=1).gather(1, o[:, :, None].expand(P, k, S))
        e["lg"] = torch.cat([e["lg"], lg[None].expand(P, B, K)], dim=1).gather(1, o[:, :, None].expand(P, k, K))
        e["lab"] = torch.cat([e["lab"], lab[None].expand(P, B)], dim=1).gather(1, o)
        hot = torch.nn.functional.one_hot(lab, K).to(torch.float64)
        e["sum"] += hot.t() @ (1 - d).to(torch.float64)
        e["cnt"] += hot.sum(0).long()

    return run_hip, run_eager


def device_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def host_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def launches(fn):
    """(all kernel launches, library launches, {library kernel: device us}) of one call, from the torch profiler's device events."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [x for x in prof.events() if x.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in x.name and "Memset" not in x.name]
    per = {}
    for x in ev:
        if "pasn" in x.name:
            short = x.name.split("pasn::")[-1].split("(")[0]
            per[short] = round(per.get(short, 0.0) + float(getattr(x, "device_time", 0.0) or getattr(x, "cuda_time", 0.0)), 1)
    return len(ev), sum("pasn" in x.name for x in ev), per


def sweep_ab(blocks, clips, k, dev):
    cfg = dict(checkpoint_path="", name="Video_XProtoNet", base_architecture="x3d_s", backbone_last_layer_num=-3, pretrained=False,
               prototype_shape="(30, 256, 1, 1, 1)", num_classes=3, img_size=224)
    m = model_builder.build(cfg)
    synth.load_synth(m)
    m = m.to(dev).eval().set_compute_dtype(torch.bfloat16)
    xs = synth.echo_clips((B, 3, 16, 224, 224)).to(dev).to(torch.bfloat16)
    full, rest = divmod(clips, B)

    class Loader:  # the resident clips re-labelled per batch (tests/configs_bench.py push)
        batch_size = B

        def __len__(self):
            return full + (rest > 0)

        def __iter__(self):
            for b in range(len(self)):
                n = B if b < full else rest
                yield {"cine": xs[:n], "target_AS": (torch.arange(n) + b) % 3, "filename": None}

    def run_push():
        push.push_prototypes(Loader(), m, class_specific=True, abstain_class=False, replace_prototypes=False, log=lambda *_: None)

    def run_global():
        global_explain.nearest_clips(Loader(), m, k=k, class_specific=True, abstain_class=False, log=lambda *_: None)

    rate = {"push": [], "global": []}
    for fn in (run_push, run_global):
        fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for tag, fn in (("push", run_push), ("global", run_global)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rate[tag].append(clips / (time.perf_counter() - t0))
    return rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3, help="sweeps of each kind in the whole-sweep A/B (0: skip it)")
    ap.add_argument("--clips", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda")
    name = torch.cuda.get_device_name()
    rows = []
    run_hip, run_eager = make_calls(a.k, dev)
    row = {"bench": "per-batch bookkeeping: update + 3 gathers + class sums", "B": B, "P": P, "K": K, "map": list(MAP), "k": a.k,
           "reps": a.reps, "device": name}
    for tag, fn in (("eager", run_eager), ("hip", run_hip)):
        n_all, n_lib, per = launches(fn)
        row[tag] = {"device_us": round(device_us(fn, a.reps), 1), "host_us_per_call": round(host_us(fn, a.reps), 1), "launches": n_all,
                    "library_launches": n_lib}
        if per:
            row[tag]["library_kernel_us"] = per
    rows.append(row)
    if a.blocks > 0:
        rate = sweep_ab(a.blocks, a.clips, a.k, dev)
        rows.append({"bench": f"sweep A/B over {a.clips} clips 3x16x224x224 bf16, X3D-S, 30 prototypes, class specific: push_prototypes vs "
                              f"nearest_clips(k={a.k})", "push_clips_per_s_blocks": [round(v, 1) for v in rate["push"]],
                     "global_clips_per_s_blocks": [round(v, 1) for v in rate["global"]],
                     "push_median": round(statistics.median(rate["push"]), 1), "global_median": round(statistics.median(rate["global"]), 1),
                     "push_spread": round(max(rate["push"]) - min(rate["push"]), 1),
                     "global_spread": round(max(rate["global"]) - min(rate["global"]), 1), "device": name})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
