"""Writes probe_sweep.json: what the library's geometry probes answer, over every descriptor the plan builder and the training tape hand
to the library and over a synthetic grid that crosses the rungs of the routing ladders.  Geometry queries only, runs without a GPU:

    python tests/golden/make_probe_sweep.py

The probes (``SINGLE`` take one descriptor, ``PAIR`` two) are the sizing and routing questions of csrc/conv.hip and csrc/wgrad.hip.  The
descriptors come in groups:

* ``plan:<case>`` / ``train:<case>`` -- every ConvDesc, and every adjacent pair of ConvDesc arguments of one call, that a case of
  make_routing_snapshot.CASES / make_train_stream_snapshot.TRAIN_CASES passes to the library while it is compiled and replayed (taken
  by a recording subclass of those scripts' ``_LibProxy``).  The file stores these descriptors (``descs``, ``groups``) so that the
  comparison does not compile 35 plans again.
* ``grid:<window>`` -- ``grid_descs()``: channel counts around the tile sizes and the X3D widths, six windows, strides 1 and 2, five
  plane sizes, N = 1 and 32.  Generated, not stored.

Every group is asked under the default environment and once under each switch of ``ENVS``; per (group, probe, environment) the file
keeps one digest of the list of answers (``digest``; an environment's cell is stored only where it differs from the default one).
tests/test_cpu_probe_sweep.py recomputes them; on a mismatch it prints the descriptors of the blocks that moved (``moved_blocks``)."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "probe_sweep.json")
OUT_WGRAD = os.path.join(HERE, "probe_sweep_wgrad.json")
_BIG = {"PASN_DWWG_BLOCKS": "2048"}
ENVS = [("default", {})] + [(f"{k}={v}", {k: v}) for k, v in (
    ("PASN_XTILE_GATED", "1"), ("PASN_NO_SE_PROLOGUE", "1"), ("PASN_NO_SE_FUSE", "1"), ("PASN_SE_FUSE_MAXC", "256"), ("PASN_WS", "0"),
    ("PASN_DWMFMA", "0"), ("PASN_NO_DWWG_STRIP", "1"), ("PASN_NO_DWWG_MARCH", "1"), ("PASN_DWWG_MARCH2", "0"), ("PASN_DWWG_CH", "2"),
    ("PASN_DWWG_WT", "3"), ("PASN_DWWG_BLOCKS", "256"), ("PASN_DWWG_BLOCKS", "2048"))] + [
    (f"PASN_DWWG_BLOCKS=2048,{k}={v}", dict(_BIG, **{k: v})) for k, v in (("PASN_DWWG_MARCH2", "0"), ("PASN_DWWG_CH", "2"), ("PASN_DWWG_WT", "3"))]
# The dense weight-gradient switches and probes came later.  They live in a file of their own (OUT_WGRAD: their environments' cells for
# every probe, and the two probes' cells for every environment), so that probe_sweep.json, which they leave byte for byte as it was, stays
# untouched; load_golden() reads the two as one.
N_BASE_ENVS = len(ENVS)
ENVS += [(f"{k}={v}", {k: v}) for k, v in (
    ("PASN_NO_WGRAD_HALO", "1"), ("PASN_NO_WGRAD_GATHER", "1"), ("PASN_WGRAD_DET", "1"), ("PASN_NO_WGRAD_TILE", "1"), ("PASN_NO_WGRAD_LDS", "1"),
    ("PASN_WGT_WIDE", "0"), ("PASN_WGT_XCD", "0"))]
# The depthwise weight-gradient workspace is sized for the first marching kernel's block count (at most 1024) whenever a marching kernel
# covers the layer, and the second marching kernel's count stays below it up to its default cap of 512: alone, these four environments
# move no answer (they are recorded all the same -- a change that made them matter would show).  With the cap raised above 1024 each
# of them does: an environment of ENV_BASE must differ from the one it names, every other one from the default.
SIZING_BLIND = ("PASN_DWWG_MARCH2=0", "PASN_DWWG_CH=2", "PASN_DWWG_WT=3", "PASN_DWWG_BLOCKS=256")
ENV_BASE = {e: "PASN_DWWG_BLOCKS=2048" for e, _ in ENVS if e.startswith("PASN_DWWG_BLOCKS=2048,")}
DTYPES = (0, 1)  # _lib.F32, _lib.BF16
CSE = (8, 16, 32, 36)  # squeeze-excite widths: the X3D ones (multiples of 4 up to 32) and one past the prologue's limit

# name -> fn(lib, descriptor ref) -> answers.  The depthwise probes are only asked of depthwise layers (what their launches require).
SINGLE = {
    "conv3d_variant": lambda L, d: [L.pasn_conv3d_variant(d, t, f) for t in DTYPES for f in range(4)],
    "conv3d_se_supported": lambda L, d: [L.pasn_conv3d_se_supported(d, t, c, r) for t in DTYPES for c in CSE for r in (0, 1)],
    "conv3d_wgrad_workspace_bytes": lambda L, d: [L.pasn_conv3d_wgrad_workspace_bytes(d, t) for t in DTYPES],
}
WGRAD = {  # asked of every descriptor, like SINGLE; recorded in OUT_WGRAD
    "conv3d_wgrad_variant": lambda L, d: [L.pasn_conv3d_wgrad_variant(d, t, w) for t in DTYPES for w in (0, 1)],
    "conv3d_wgrad_row_parts": lambda L, d: [L.pasn_conv3d_wgrad_row_parts(d, t, w) for t in DTYPES for w in (0, 1)],
}
DEPTHWISE = {
    "dwconv3d_variant": lambda L, d: [L.pasn_dwconv3d_variant(d, t) for t in DTYPES],
    "dwconv3d_pool_blocks": lambda L, d: [L.pasn_dwconv3d_pool_blocks(d, t) for t in DTYPES],
    "dwconv3d_se_pool_blocks": lambda L, d: [L.pasn_dwconv3d_se_pool_blocks(d, t) for t in DTYPES],
    "dwconv3d_se_supported": lambda L, d: [L.pasn_dwconv3d_se_supported(d, t, c) for t in DTYPES for c in CSE],
    "dwconv3d_wgrad_workspace_floats": lambda L, d: [L.pasn_dwconv3d_wgrad_workspace_floats(d)],
}
PAIR = {
    "conv3d_pair_variant": lambda L, a, b: [L.pasn_conv3d_pair_variant(a, b, t, f) for t in DTYPES for f in (0, 1)],
    "conv3d_pair_supported": lambda L, a, b: [L.pasn_conv3d_pair_supported(a, b, t) for t in DTYPES],
    "conv3d_pair_se_supported": lambda L, a, b: [L.pasn_conv3d_pair_se_supported(a, b, t, c) for t in DTYPES for c in CSE],
    "conv3d_short_supported": lambda L, a, b: [L.pasn_conv3d_short_supported(a, b, t) for t in DTYPES],
    "x3d_expdw_supported": lambda L, a, b: [L.pasn_x3d_expdw_supported(a, b, t) for t in DTYPES],
    "x3d_expdw_variant": lambda L, a, b: [L.pasn_x3d_expdw_variant(a, b, t) for t in DTYPES],
    "x3d_expdw_pool_blocks": lambda L, a, b: [L.pasn_x3d_expdw_pool_blocks(a, b, t) for t in DTYPES],
}
PROBES = tuple(SINGLE) + tuple(DEPTHWISE) + tuple(PAIR) + tuple(WGRAD)


def _fields():
    from protoasnet_amd import _lib

    return [f for f, _ in _lib.ConvDesc._fields_]


def _is_depthwise(t) -> bool:
    f = dict(zip(_fields(), t))
    return f["Cin"] == f["Cout"] and f["Cin_p"] == f["Cout_p"] and f["Cout_p"] > 0 and f["Cout_p"] % 8 == 0 and f["kh"] * f["kw"] <= 9


def answers(probe, singles, pairs):
    """[(descriptor or pair of descriptors as field tuples, the probe's answers)] under the environment now in force."""
    from protoasnet_amd import _lib

    L, mk = _lib.lib(), lambda t: ctypes.byref(_lib.ConvDesc(*t))
    if probe in PAIR:
        return [((a, b), PAIR[probe](L, mk(a), mk(b))) for a, b in pairs]
    if probe in DEPTHWISE:
        return [(t, DEPTHWISE[probe](L, mk(t))) for t in singles if _is_depthwise(t)]
    return [(t, dict(SINGLE, **WGRAD)[probe](L, mk(t))) for t in singles]


BLOCK = 16
_ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-"


def digest(rows) -> str:
    """"<10 hex digits of all answers>:<one character per block of BLOCK rows>": the first part is the comparison, the second says where."""
    sha = lambda obj: hashlib.sha256(repr(obj).encode()).hexdigest()
    ans = [a for _, a in rows]
    return sha(ans)[:10] + ":" + "".join(_ALPHABET[int(sha(ans[i: i + BLOCK])[:2], 16) & 63] for i in range(0, len(ans), BLOCK))


def moved_blocks(rows, want: str):
    """The rows of the blocks whose mark differs from the recorded cell ``want`` (all rows if only the digest does)."""
    got, wm = digest(rows).split(":")[1], want.split(":")[1]
    bad = [i for i in range(len(got)) if got[i: i + 1] != wm[i: i + 1]] if len(got) == len(wm) else []
    return [r for i in bad for r in rows[i * BLOCK: (i + 1) * BLOCK]] or rows


# ---- (a) the descriptors of the compiled plans and training tapes ------------------------------------------------------------------
def _harvesting(base, singles, pairs):
    """``base`` (a _LibProxy) that also notes the ConvDesc arguments of every call, passed through or recorded."""
    from protoasnet_amd import _lib

    class Harvest(base):
        def __getattr__(self, name):
            call = super().__getattr__(name)

            def noting(*args):
                ds = [tuple(getattr(a._obj, f) for f in _fields()) for a in args if isinstance(getattr(a, "_obj", None), _lib.ConvDesc)]
                for t in ds:
                    singles.setdefault(t)
                for p in zip(ds, ds[1:]):
                    pairs.setdefault(p)
                return call(*args)

            noting.__name__ = name
            return noting

    return Harvest


def harvest():
    """{group: (singles, pairs)} of the plan and training cases, in order of first use."""
    import make_routing_snapshot as plan_snap
    import make_train_stream_snapshot as train_snap

    groups = {}
    for prefix, mod, cases, run in (("plan", plan_snap, plan_snap.CASES, plan_snap.call_stream),
                                    ("train", train_snap, train_snap.TRAIN_CASES, train_snap.train_call_stream)):
        base = mod._LibProxy
        for case in cases:
            singles, pairs = {}, {}
            mod._LibProxy = _harvesting(base, singles, pairs)
            try:
                run(case)
            finally:
                mod._LibProxy = base
            groups[f"{prefix}:{case[0]}"] = (list(singles), list(pairs))
            print(f"{prefix}:{case[0]}: {len(singles)} descriptors, {len(pairs)} pairs")
    return groups


# ---- (b) the synthetic grid ----------------------------------------------------------------------------------------------------------
WINDOWS = ((1, 1, 1), (3, 1, 1), (5, 1, 1), (1, 3, 3), (3, 3, 3), (1, 7, 7))
_WIDTHS = (8, 16, 24, 32, 40, 48, 54, 64, 72, 96, 108, 128, 136, 192, 216, 256, 264, 432, 512, 520, 2048)
# (Cin, Cout): every width onto itself (the depthwise layers among them), neighbours in both directions, and the X3D expand / project
# / head pairs
CHANNELS = ([(c, c) for c in _WIDTHS] + [(a, b) for a, b in zip(_WIDTHS, _WIDTHS[1:])] + [(b, a) for a, b in zip(_WIDTHS, _WIDTHS[1:])]
            + [(24, 54), (54, 24), (48, 108), (108, 48), (96, 216), (216, 96), (192, 432), (432, 192), (432, 2048), (3, 24), (512, 2048)])
PLANES = (7, 14, 28, 56, 13)


def _up(v, m):
    return (v + m - 1) // m * m


def grid_desc(n, t, plane, cin, cout, k, stride, in_swish=0, w_frag=0):
    p = tuple(e // 2 for e in k)
    s = (1, 1, 1) if k[1] == 1 and k[0] > 1 else (1, stride, stride)  # the temporal windows keep the frame
    out = lambda i, j: (i + 2 * p[j] - k[j]) // s[j] + 1
    f = dict(N=n, Ti=t, Hi=plane, Wi=plane, Cin=cin, Cin_p=_up(cin, 8), To=out(t, 0), Ho=out(plane, 1), Wo=out(plane, 2), Cout=cout,
             Cout_p=_up(cout, 8), kt=k[0], kh=k[1], kw=k[2], st=s[0], sh=s[1], sw=s[2], pt=p[0], ph=p[1], pw=p[2], act=1, in_swish=in_swish,
             w_kc=_up(_up(cin, 8), 16), w_rows=_up(_up(cout, 8), 128), w_frag=w_frag)
    return tuple(f[name] for name in _fields())


def grid_descs():
    """{group: (singles, pairs)}, one group per window.  A (1,1,1) layer also comes with a swish on its input and with fragment-major
    weights; the pairs are (1,1,1) project -> expand chains and expand -> depthwise (3,3,3) pairs of one width."""
    groups = {}
    for k in WINDOWS:
        singles, pairs = {}, {}
        for n, t in ((1, 16), (32, 4)):
            for plane in PLANES:
                for stride in (1, 2):
                    if k[1] == 1 and k[0] > 1 and stride == 2:
                        continue
                    for cin, cout in CHANNELS:
                        singles.setdefault(grid_desc(n, t, plane, cin, cout, k, stride))
                        if k == (1, 1, 1):
                            singles.setdefault(grid_desc(n, t, plane, cin, cout, k, stride, in_swish=1))
                            singles.setdefault(grid_desc(n, t, plane, cin, cout, k, stride, w_frag=1))
                    if k == (1, 1, 1) and stride == 1:
                        for a, b in CHANNELS:
                            for frag in (0, 1):
                                pairs.setdefault((grid_desc(n, t, plane, a, b, k, 1, w_frag=frag), grid_desc(n, t, plane, b, a, k, 1, w_frag=frag)))
                    if k == (3, 3, 3):
                        for a, b in CHANNELS:
                            if a != b:
                                pairs.setdefault((grid_desc(n, t, plane, a, b, (1, 1, 1), 1, w_frag=1), grid_desc(n, t, plane, b, b, k, stride)))
                                # the strided shortcut beside a project conv (pasn_conv3d_short_supported)
                                pairs.setdefault((grid_desc(n, t, plane // stride or 1, a, b, (1, 1, 1), 1), grid_desc(n, t, plane, b, b, (1, 1, 1), stride)))
        groups["grid:%dx%dx%d" % k] = (list(singles), list(pairs))
    return groups


def sweep(groups):
    """{group: {probe: {environment: digest}}}"""
    from protoasnet_amd import _lib

    out = {g: {p: {} for p in PROBES} for g in groups}
    for env_name, env in ENVS:
        with _lib.tuning_env(**env):
            for g, (singles, pairs) in groups.items():
                for p in PROBES:
                    out[g][p][env_name] = digest(answers(p, singles, pairs))
    return out


def load_golden():
    """probe_sweep.json and probe_sweep_wgrad.json as one record."""
    g, w = json.load(open(OUT)), json.load(open(OUT_WGRAD))
    g["envs"] += w["envs"]
    g["probes"] += w["probes"]
    for grp, per in w["digests"].items():
        for p, cell in per.items():
            g["digests"][grp].setdefault(p, {}).update(cell)
    return g


def stored_groups(golden):
    descs = [tuple(t) for t in golden["descs"]]
    return {g: ([descs[i] for i in v["singles"]], [(descs[i], descs[j]) for i, j in v["pairs"]]) for g, v in golden["groups"].items()}


if __name__ == "__main__":
    for k in [k for k in os.environ if k.startswith("PASN_")]:
        del os.environ[k]
    harvested = harvest()
    index = {}
    for singles, pairs in harvested.values():
        for t in singles + [t for p in pairs for t in p]:
            index.setdefault(t, len(index))
    stored = {g: {"singles": [index[t] for t in s], "pairs": [[index[a], index[b]] for a, b in p]} for g, (s, p) in harvested.items()}
    groups = dict(harvested, **grid_descs())
    for g, (s, p) in groups.items():
        print(f"{g}: {len(s)} descriptors, {len(p)} pairs")
    digests = {g: {p: {e: c for e, c in cell.items() if e == "default" or c != cell["default"]} for p, cell in per.items()}
               for g, per in sweep(groups).items()}
    base_envs, late_envs = [e for e, _ in ENVS[:N_BASE_ENVS]], [e for e, _ in ENVS[N_BASE_ENVS:]]
    base = {g: {p: {e: c for e, c in cell.items() if e in base_envs} for p, cell in per.items() if p not in WGRAD} for g, per in digests.items()}
    late = {g: {p: {e: c for e, c in cell.items() if p in WGRAD or e in late_envs} for p, cell in per.items()} for g, per in digests.items()}
    with open(OUT, "w") as fh:
        json.dump({"fields": _fields(), "envs": base_envs, "probes": [p for p in PROBES if p not in WGRAD], "descs": [list(t) for t in index],
                   "groups": stored, "digests": base}, fh, separators=(",", ":"))
    with open(OUT_WGRAD, "w") as fh:
        json.dump({"envs": late_envs, "probes": list(WGRAD), "digests": {g: {p: c for p, c in per.items() if c} for g, per in late.items()}},
                  fh, separators=(",", ":"))
    print(f"{OUT}: {len(groups)} groups, {len(index)} stored descriptors, {os.path.getsize(OUT)} + {os.path.getsize(OUT_WGRAD)} bytes")
