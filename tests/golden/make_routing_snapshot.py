"""Writes the two committed routing snapshots.  Geometry and host-side packing only, runs without a GPU:

    python tests/golden/make_routing_snapshot.py

* routing_x3d_s_cfg2.json: the DEFAULT launch list of the benchmarked configuration (BASELINE config 2: X3D-S, 32 x 3 x 16 x 224 x 224,
  bf16) -- one entry per launch: plan kind, kernel instance, layer shape.
* call_stream_digests.json: for every case of ``CASES`` one short digest per launch of EVERYTHING the launch passes to the library --
  entry point, scalars, descriptors, buffer dataflow, packed operand bytes -- plus its ``meta`` row (``call_stream``).

tests/test_cpu_routing.py compares the plans compiled now against these files, so an environment variable or a refactor cannot silently
change the benchmarked path or an operand layout; regenerate them when a routing change is intended (and say so in the commit)."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def routing(arch="x3d_s", shape=(32, 3, 16, 224, 224)):
    import torch

    from protoasnet_amd import backbones, plan

    trunk = backbones.X3DFeatures(arch)
    pb = plan.PlanBuilder(torch.device("cpu"), torch.bfloat16, torch.bfloat16)
    x = pb.input(shape)
    with torch.no_grad():
        trunk.build_plan(pb, x)
    return [{"kind": m.get("kind", ""), "kernel": m["kernel"], "shape": m.get("shape", "")} for m in pb.meta]


# ---- call-stream digests ----------------------------------------------------------------------------------------------------------
# (name, trunk, input shape, compute dtype, input dtype, switches).  A uint8 input is the grey clip with the device-side normalisation.
_X3D_S = (32, 3, 16, 224, 224)
CASES = [
    ("x3d_s_n32_bf16", "x3d_s", _X3D_S, "bf16", "bf16", {}),
    ("x3d_s_n2_grey_u8_bf16", "x3d_s", (2, 1, 16, 224, 224), "bf16", "u8", {}),
    ("x3d_s_n2_f32", "x3d_s", (2, 3, 16, 224, 224), "f32", "f32", {}),
    ("x3d_m_n1_bf16", "x3d_m", (1, 3, 32, 312, 312), "bf16", "bf16", {}),
    ("r2plus1d_18_n2_bf16", "resnet2p1d_18", (2, 3, 32, 112, 112), "bf16", "bf16", {}),
    ("r2plus1d_18_n2_f32", "resnet2p1d_18", (2, 3, 32, 112, 112), "f32", "f32", {}),
    ("resnet18_n8_bf16", "resnet18", (8, 3, 224, 224), "bf16", "bf16", {}),
    ("resnet18_n8_f32", "resnet18", (8, 3, 224, 224), "f32", "f32", {}),
] + [
    (f"x3d_s_n32_bf16[{k}={v}]", "x3d_s", _X3D_S, "bf16", "bf16", {k: v})
    for k, v in (("PASN_EXPDW", "0"), ("PASN_NO_SE_PROLOGUE", "1"), ("PASN_NO_XPAIR", "1"), ("PASN_NO_SHORTFUSE", "1"), ("PASN_NO_EDP", "1"),
                 ("PASN_NO_PE", "1"), ("PASN_NO_STEM", "1"), ("PASN_WS", "0"), ("PASN_EXPDW_FOLD", "0"))
]
FIELDS = ("entry", "scalars", "descs", "buffers", "operands", "meta")  # a launch's digest = one 6-hex-digit group per field, in this order


class _LibProxy:
    """Stands in for the loaded library.  While a plan is built (``calls is None``) every call goes to the real library -- only geometry
    queries happen then; while the plan's ops are replayed it records (entry point, arguments) and returns 0 instead of launching."""

    def __init__(self, real):
        self._real, self.calls = real, None

    def __getattr__(self, name):
        real = getattr(self._real, name)

        def call(*args):
            if self.calls is None:
                return real(*args)
            self.calls.append((name, args))
            return 0

        call.__name__ = name  # what the real entry point answers (the training tape names its ops by it)
        return call


def _hex(obj) -> str:
    return hashlib.sha256(repr(obj).encode()).hexdigest()[:6]


def call_stream(case):
    """Build one case's plan on the CPU and replay it against the recording proxy.  Returns (digests, len(ops), arena_bytes, naive_bytes)."""
    import torch

    from protoasnet_amd import _lib, backbones, plan, synth

    name, arch, shape, dtype, in_dtype, env = case
    dt = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}
    trunk = {"x3d_s": lambda: backbones.X3DFeatures("x3d_s"), "x3d_m": lambda: backbones.X3DFeatures("x3d_m"),
             "resnet2p1d_18": lambda: backbones.resnet2p1d_18(pretrained=False), "resnet18": backbones.ResNet18Features}[arch]()
    synth.load_synth(trunk)
    if in_dtype == "u8":
        trunk.set_input_normalization(mean=0.099, std=0.171, scale=1.0 / 255.0)
    proxy, real_lib = _LibProxy(_lib.lib()), _lib.lib
    _lib.lib = lambda: proxy
    try:
        with _lib.tuning_env(**env):
            pb = plan.PlanBuilder(torch.device("cpu"), dt[dtype], dt[in_dtype], trunk.input_affine)
            x_in = pb.input(shape)
            with torch.no_grad():
                y_out = trunk.build_plan(pb, x_in)
            ptrs = [(i + 1) << 40 for i in range(len(pb.bufs))]  # synthetic addresses: no tensor lives there
            proxy.calls = []
            for op in pb.ops:
                op(ptrs, 0)
            calls, proxy.calls = proxy.calls, None
            built = pb.finish(x_in, y_out)
    finally:
        _lib.lib = real_lib
    assert len(calls) == len(pb.ops) == len(pb.meta), "one library call and one meta row per launch"
    buf_of = {p: i for i, p in enumerate(ptrs)}
    kept = {}
    for t in pb.keep:
        if isinstance(t, torch.Tensor) and t.numel():
            kept.setdefault(t.data_ptr(), t)
    order, digests = {}, []  # buffer id -> its rank in order of first use
    for (entry, args), meta in zip(calls, pb.meta):
        scalars, descs, buffers, operands = [], [], [], []
        argtypes = _lib.SIGNATURES[entry][1]
        assert len(args) == len(argtypes), entry
        for a, ty in zip(args, argtypes):
            if ty is ctypes.POINTER(_lib.ConvDesc):
                descs.append(None if a is None else tuple(getattr(a._obj, f) for f, _ in _lib.ConvDesc._fields_))
            elif ty is not ctypes.c_void_p:
                scalars.append(a)
            elif a in buf_of:
                buffers.append(order.setdefault(buf_of[a], len(order)))
            elif a == 0:
                buffers.append(None)
                operands.append(0)
            else:
                t = kept[a]  # KeyError: a pointer that is neither a plan buffer nor a tensor the plan keeps alive
                operands.append(hashlib.sha256(t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16])
        row = {"entry": entry, "scalars": scalars, "descs": descs, "buffers": buffers, "operands": operands,
               "meta": [meta[k] for k in ("kind", "kernel", "shape", "bytes", "flops")]}
        digests.append("".join(_hex(row[f]) for f in FIELDS))
    return digests, len(pb.ops), built.arena_bytes, built.naive_bytes


if __name__ == "__main__":
    for k in [k for k in os.environ if k.startswith("PASN_")]:
        del os.environ[k]
    rows = routing()
    out = os.path.join(HERE, "routing_x3d_s_cfg2.json")
    with open(out, "w") as fh:
        json.dump({"workload": "x3d_s 32x3x16x224x224 bf16", "launches": len(rows), "rows": rows}, fh, indent=1)
    print(f"{out}: {len(rows)} launches")
    streams = {}
    for case in CASES:
        streams[case[0]], n_ops, arena, naive = call_stream(case)
        print(f"{case[0]}: len(ops)={n_ops} arena_bytes={arena} naive_bytes={naive}")
    out = os.path.join(HERE, "call_stream_digests.json")
    with open(out, "w") as fh:
        json.dump({"fields": list(FIELDS), "cases": streams}, fh, indent=0)
    print(f"{out}: {len(streams)} cases")
