"""Writes train_call_stream_digests.json: what the compiled TRAINING pass (protoasnet_amd/train.py: forward + backward launch list of
trunk + head for one input shape) hands to the library.  Host side only, runs without a GPU:

    python tests/golden/make_train_stream_snapshot.py

For every case of ``TRAIN_CASES`` a ``TrainRunner`` is compiled on the CPU and its ops are replayed against the recording stand-in of
make_routing_snapshot.py (``_LibProxy``).  Per op, one row with the fields of ``TRAIN_FIELDS``:

* op       -- (op_names[i], op_kind[i], op_join.get(i), op_bytes[i])
* entry    -- the entry point (None for a join: it calls nothing)
* scalars  -- every non-pointer argument
* descs    -- every field of each ConvDesc / XProtoDesc argument
* buffers  -- per pointer into the plan's buffers (rank of the buffer in order of first use, byte offset: a gradient slot is an offset
              into the flat gradient buffer), None for NULL
* operands -- per other pointer: the NAME of the live parameter / buffer of the model it is, or the hash of the bytes of the tensor the
              plan keeps (after ``plan.refresh`` ran once on the synthetic weights), or -- a destination of the native packer, which
              nothing fills on the CPU -- its rank among the kept tensors

and once per case the ``plan`` row: n_fwd, arena_bytes, naive_bytes, gsize, len(nbt), groups, the arena offsets (in blocks of 16
buffers), ``pslots`` (parameter name, offset, numel) and ``pack_jobs`` (parameter name, rank of the destination among the kept tensors,
mode and the eight integers).  The native packer does not run on the CPU: its job rows are what is pinned, and the bytes the torch
refresh closures write are pinned by the PASN_NO_PACK=1 case.

What is committed per case: ``sha``, the SHA-256 of all of the above written out in full -- the comparison is exact through it -- and,
to say WHERE a stream moved, one character (6 bits of ``_hex``) per field of every op in ``ops`` and per block / row of ``offsets``,
``pslots`` and ``pack_jobs``: the shape of call_stream_digests.json with narrow groups, because the 14 000 ops of the 27 cases would
otherwise make a file of 600 KB.

tests/test_cpu_train_stream.py compares the runners compiled now against this file: buffer order decides arena offsets, side-launch and
join order decide live ranges, and neither shows on a CPU otherwise."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_routing_snapshot import _hex, _LibProxy  # noqa: E402

_VIDEO = dict(checkpoint_path="", name="Video_XProtoNet", backbone_last_layer_num=-3, pretrained=False, num_classes=3)
MODELS = {
    "ppnet_r18": dict(checkpoint_path="", name="ProtoPNet", base_architecture="resnet18", pretrained=False, prototype_shape="(30, 512, 1, 1)",
                      num_classes=3, img_size=224, add_on_layers_type="regular", prototype_activation_function="log"),
    "xproto_r18": dict(checkpoint_path="", name="XProtoNet", base_architecture="resnet18", pretrained=False, prototype_shape="(40, 512, 1, 1)",
                       num_classes=4, img_size=224, add_on_layers_type="regular"),
    "video_r2p1d": dict(_VIDEO, base_architecture="resnet2p1d_18", prototype_shape="(40, 256, 1, 1, 1)", num_classes=4, img_size=112),
    "video_x3d_s": dict(_VIDEO, base_architecture="x3d_s", prototype_shape="(30, 256, 1, 1, 1)", img_size=224),
    "video_x3d_m": dict(_VIDEO, base_architecture="x3d_m", prototype_shape="(60, 256, 1, 1, 1)", img_size=312),
}
_IMG, _R2P1D, _X3D, _X3D_M, _CFG3 = (4, 3, 224, 224), (2, 3, 16, 112, 112), (2, 3, 4, 64, 64), (1, 3, 16, 224, 224), (64, 3, 16, 224, 224)
_SWITCHES = (("PASN_NO_PACK", "1"), ("PASN_TRAIN_STREAMS", "1"), ("PASN_TRAIN_SIDE_DEPTH", "1"), ("PASN_NO_SE_ANALYTIC", "1"),
             ("PASN_NO_DW_STATS", "1"), ("PASN_DW_DGRAD_REDUCE", "1"))
# (PASN_NO_STEM_MFMA has no case: it routes the fused X3D stem of the inference plan only; the training tape emits the stem's two convs as
# units and its stream is the default one under that switch)
_X3D_BF16 = (2, 3, 16, 224, 224)  # the switch cases: a shape on which every fused / matrix-core training arm of X3D-S is taken


def _case(name, model, shape, dtype, mode=0, env=None, phase=None):
    """(name, model of MODELS, input shape, compute dtype, TrainRunner mode, switches, frozen phase).  The input clip has the compute
    dtype; mode 2 = the paired pass (two statistics groups), its shape is that of [clips, warped clips]."""
    return (name, model, shape, dtype, mode, env or {}, phase)


TRAIN_CASES = [_case(f"{m}_{dt}", m, s, dt) for m, s in (("ppnet_r18", _IMG), ("xproto_r18", _IMG), ("video_r2p1d", _R2P1D),
                                                         ("video_x3d_s", _X3D), ("video_x3d_m", _X3D_M)) for dt in ("f32", "bf16")] + [
    _case("video_x3d_s_f32_mode1", "video_x3d_s", _X3D, "f32", mode=1),
    _case("video_x3d_s_f32_mode2", "video_x3d_s", (4,) + _X3D[1:], "f32", mode=2),
    _case("xproto_r18_bf16_mode1", "xproto_r18", _IMG, "bf16", mode=1),
    _case("xproto_r18_f32_grey", "xproto_r18", (4, 1, 224, 224), "f32"),
    _case("xproto_r18_bf16_grey", "xproto_r18", (4, 1, 224, 224), "bf16"),
    _case("video_x3d_s_bf16_grey", "video_x3d_s", (2, 1, 16, 224, 224), "bf16"),
    _case("video_x3d_s_cfg3_bf16_mode2", "video_x3d_s", _CFG3, "bf16", mode=2),  # BASELINE config 3: 2 x 32 clips in one pass; compile only
    _case("video_x3d_s_f32_warm", "video_x3d_s", _X3D, "f32", phase="warm"),
    _case("video_x3d_s_f32_last_layer", "video_x3d_s", _X3D, "f32", phase="last_layer"),
    _case("video_x3d_s_n2_bf16", "video_x3d_s", _X3D_BF16, "bf16"),
] + [_case(f"video_x3d_s_n2_bf16[{k}={v}]", "video_x3d_s", _X3D_BF16, "bf16", env={k: v}) for k, v in _SWITCHES] + [
    _case("ppnet_r18_bf16[PASN_NO_FC_MFMA=1]", "ppnet_r18", _IMG, "bf16", env={"PASN_NO_FC_MFMA": "1"}),
]
# every switch case must differ from the case it is a variation of (checked when the file is written: no vacuous case)
SWITCH_BASE = {c[0]: ("ppnet_r18_bf16" if c[1] == "ppnet_r18" else "video_x3d_s_n2_bf16") for c in TRAIN_CASES if c[5]}
TRAIN_FIELDS = ("op", "entry", "scalars", "descs", "buffers", "operands")


_ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-"


def _mark(obj) -> str:
    """One character of ``_hex(obj)``: enough to locate a difference; ``sha`` decides whether there is one."""
    return _ALPHABET[int(_hex(obj)[:2], 16) & 63]


def _bytes_hash(t) -> str:
    import torch

    return hashlib.sha256(t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def train_call_stream(case):
    """Compile one case's TrainRunner on the CPU and replay its ops against the recording proxy.  Returns the case's entry of the
    committed file: {"sha", "n_ops", "ops", "plan"} (module docstring)."""
    import torch

    from protoasnet_amd import _lib, model_builder, synth, train

    name, model_key, shape, dtype, mode, env, phase = case
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[dtype]
    model = model_builder.build(MODELS[model_key])
    synth.load_synth(model)
    model.train().set_compute_dtype(dt)
    if phase is not None:  # the two frozen phases of the reference's agents (tests/test_gpu_train.py::test_frozen_parameter_phases)
        trainable = (lambda n: not n.startswith("cnn_backbone.")) if phase == "warm" else (lambda n: n == "last_layer.weight")
        for n, p in model.named_parameters():
            p.requires_grad_(trainable(n) and n != "ones")
    x = torch.empty(1, dtype=dt).expand(shape)  # shape, dtype and device are all the compiler reads: no clip is allocated
    proxy, real_lib = _LibProxy(_lib.lib()), _lib.lib
    _lib.lib = lambda: proxy
    try:
        with _lib.tuning_env(**env):
            runner = train.TrainRunner(model, x, mode, head="A" if model_key.startswith("ppnet") else "B")
            plan = runner.plan
            with torch.no_grad():
                for r in plan.refresh:
                    r()
            ptrs = [(i + 1) << 40 for i in range(len(plan.offsets))]  # synthetic addresses: no tensor lives there
            proxy.calls, per_op = [], []
            for op in plan.ops:
                before = len(proxy.calls)
                op(ptrs, 0)
                assert len(proxy.calls) - before <= 1, "an op is at most one library call"
                per_op.append(proxy.calls[before] if len(proxy.calls) > before else None)
            proxy.calls = None
    finally:
        _lib.lib = real_lib
    named = {t.data_ptr(): n for n, t in list(model.named_parameters()) + list(model.named_buffers()) if t.numel()}
    kept, kept_rank = {}, {}
    for t in plan.keep:
        if isinstance(t, torch.Tensor) and t.numel() and t.data_ptr() not in kept:
            kept_rank[t.data_ptr()] = len(kept)
            kept[t.data_ptr()] = t
    packed = {j[1].data_ptr() for j in plan.pack_jobs}  # written by the native packer only: named by rank, their bytes are not set here
    desc_types = {ctypes.POINTER(_lib.ConvDesc): _lib.ConvDesc, ctypes.POINTER(_lib.XProtoDesc): _lib.XProtoDesc}
    order, rows = {}, []  # buffer id -> its rank in order of first use
    for i, call in enumerate(per_op):
        row = {"op": (plan.op_names[i], plan.op_kind[i], plan.op_join.get(i), plan.op_bytes[i]), "entry": None, "scalars": [], "descs": [],
               "buffers": [], "operands": []}
        if call is not None:
            row["entry"], args = call
            argtypes = _lib.SIGNATURES[row["entry"]][1]
            assert len(args) == len(argtypes), row["entry"]
            for a, ty in zip(args, argtypes):
                if ty in desc_types:
                    row["descs"].append(None if a is None else tuple(getattr(a._obj, f) for f, _ in desc_types[ty]._fields_))
                elif ty is not ctypes.c_void_p:
                    row["scalars"].append(a)
                elif a == 0:
                    row["buffers"].append(None)
                elif a in named:
                    row["operands"].append(named[a])
                elif a in kept:
                    row["operands"].append(("packed", kept_rank[a]) if a in packed else _bytes_hash(kept[a]))
                else:
                    b, off = (a >> 40) - 1, a & ((1 << 40) - 1)
                    # neither a plan buffer (+ an offset inside the gradient buffer) nor a tensor the plan keeps alive nor a parameter
                    assert 0 <= b < len(ptrs) and off < (max(4 * plan.gsize, 1) if b == plan.gbuf else 1), (i, row["entry"], hex(a))
                    row["buffers"].append((order.setdefault(b, len(order)), off))
        rows.append([row[f] for f in TRAIN_FIELDS])
    pname = {id(p): n for n, p in model.named_parameters()}
    offsets = [plan.offsets[j: j + 16] for j in range(0, len(plan.offsets), 16)]
    pslots = [(pname[id(p)], off, numel) for p, off, numel in plan.pslots]
    jobs = [(pname[id(j[0])], kept_rank[j[1].data_ptr()]) + tuple(int(v) for v in j[2:]) for j in plan.pack_jobs]
    head = {"n_fwd": plan.n_fwd, "arena_bytes": plan.arena_bytes, "naive_bytes": plan.naive_bytes, "gsize": plan.gsize,
            "nbt": len(plan.nbt), "groups": plan.groups, "refresh": len(plan.refresh)}
    return {"sha": hashlib.sha256(repr((rows, head, offsets, pslots, jobs)).encode()).hexdigest(), "n_ops": len(rows),
            "ops": "".join(_mark(f) for r in rows for f in r),
            "plan": dict(head, offsets="".join(_mark(o) for o in offsets), pslots="".join(_mark(r) for r in pslots),
                         pack_jobs="".join(_mark(r) for r in jobs))}


if __name__ == "__main__":
    import time

    for k in [k for k in os.environ if k.startswith("PASN_")]:
        del os.environ[k]
    streams = {}
    for case in TRAIN_CASES:
        t0 = time.time()
        s = streams[case[0]] = train_call_stream(case)
        print(f"{case[0]}: {s['n_ops']} ops, {s['plan']['n_fwd']} forward, arena {s['plan']['arena_bytes']} B, "
              f"{len(s['plan']['pack_jobs'])} pack jobs, {s['plan']['refresh']} refresh closures, {time.time() - t0:.1f} s")
    for sw, base in SWITCH_BASE.items():
        assert streams[sw]["sha"] != streams[base]["sha"], f"{sw} moves nothing in the training stream: drop the case"
    out = os.path.join(HERE, "train_call_stream_digests.json")
    with open(out, "w") as fh:
        json.dump({"fields": list(TRAIN_FIELDS), "cases": streams}, fh, indent=1)
    print(f"{out}: {len(streams)} cases, {os.path.getsize(out)} bytes")
