"""The numpy restatement of the RISE kernels (protoasnet_amd/saliency.py, csrc/rise.hip, include/protoasnet_amd.h, "Black-box saliency").
The reference has no code for any of this: the restatement IS the specification the kernels are held to.  float32 arrays throughout the
mask (numpy rounds every float32 operation on its own: nothing is contracted), float64 sums in a Python loop over the masks."""
import math

import numpy as np

from bootstrap_cases import philox4x32_10

F32 = np.float32
QNAN = {np.dtype(np.float32): np.uint32(0x7FC00000), np.dtype(np.uint16): np.uint16(0x7FC0)}


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def thw(shape):
    shape = tuple(int(v) for v in shape)
    return shape if len(shape) == 3 else (1,) + shape


def cells(shape, grid):
    """ceil(T / gt), ceil(H / gh), ceil(W / gw)."""
    return tuple(-(-s // g) for s, g in zip(thw(shape), grid))


def keep_of(p):
    """min(2^32 - 1, floor(p 2^32)); the product is exact (a power-of-two scale)."""
    return min(2 ** 32 - 1, int(math.floor(float(p) * 4294967296.0)))


def _key(seed):
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)


def lattice(grid, keep, seed, clip, m):
    """(gt + 2, gh + 2, gw + 2) float32 of 0 / 1: point c is word c & 3 of philox(counter (c >> 2, m, clip, 0)) < keep."""
    gt, gh, gw = grid
    L = (gt + 2) * (gh + 2) * (gw + 2)
    q = np.arange((L + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, m), np.full_like(q, clip & 0xFFFFFFFF), np.zeros_like(q)], -1)
    words = philox4x32_10(ctr, _key(seed)).reshape(-1)[:L]
    return (words.astype(np.uint64) < np.uint64(keep)).astype(F32).reshape(gt + 2, gh + 2, gw + 2)


def shifts(shape, grid, seed, clip, m):
    """(st, sh, sw): word i of philox((0, m, clip, 1)) times the cell, shifted right by 32."""
    w = philox4x32_10(np.array([0, m, clip & 0xFFFFFFFF, 1], dtype=np.uint64), _key(seed))
    return tuple(int((int(w[i]) * c) >> 32) for i, c in enumerate(cells(shape, grid)))


def axis(n, c, s):
    """Lattice index and fraction of the positions 0 .. n - 1 of an axis with cell c under shift s: i = (pos + s) // c,
    f = float32(pos + s - i c) / float32(c), an IEEE float32 division."""
    pos = np.arange(n, dtype=np.int64) + s
    i = pos // c
    return i, (pos - i * c).astype(F32) / F32(c)


def lerp(a, b, f):
    return a + (b - a) * f  # float32 arrays: three roundings


def mask(shape, grid, keep, seed, clip, m):
    """The mask (T, H, W) float32 of mask m of clip `clip`: first along W (four times), then along H (twice), then along T."""
    T, H, W = thw(shape)
    lat = lattice(grid, keep, seed, clip, m)
    st, sh, sw = shifts(shape, grid, seed, clip, m)
    ct, ch, cw = cells(shape, grid)
    (it, ft), (iy, fy), (ix, fx) = axis(T, ct, st), axis(H, ch, sh), axis(W, cw, sw)
    assert it.max() + 1 <= grid[0] + 1 and iy.max() + 1 <= grid[1] + 1 and ix.max() + 1 <= grid[2] + 1
    it, iy, ix = it[:, None, None], iy[None, :, None], ix[None, None, :]
    ft, fy, fx = ft[:, None, None], fy[None, :, None], fx[None, None, :]
    w = [[lerp(lat[it + dt, iy + dy, ix], lat[it + dt, iy + dy, ix + 1], fx) for dy in (0, 1)] for dt in (0, 1)]
    return lerp(lerp(w[0][0], w[0][1], fy), lerp(w[1][0], w[1][1], fy), ft)


# ---- pasn_rise_apply -----------------------------------------------------------------------------------------------------------------------
def widen(raw):
    """Raw elements (float32, or the uint16 bit patterns of bf16) -> float32."""
    raw = np.asarray(raw)
    return raw if raw.dtype == np.float32 else (raw.astype(np.uint32) << np.uint32(16)).view(F32)


def narrow(f, like):
    """float32 -> raw elements of `like`'s dtype: once, to nearest even; a NaN is the canonical quiet NaN."""
    f = np.ascontiguousarray(f, dtype=F32)
    u = f.view(np.uint32)
    nan = np.isnan(f)
    if like.dtype == np.float32:
        return np.where(nan, QNAN[like.dtype], u).astype(np.uint32).view(F32)
    r = ((u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(nan, QNAN[like.dtype], r).astype(np.uint16)


def masked_ref(x, shape, grid, keep, seed, clip0, m0, Mc, baseline=None, fill=0):
    """x (N, C, V) raw elements, baseline like x or None (then the scalar `fill`, already a raw element) -> (N, Mc, C, V) raw:
    b + (x - b) mask in float32, three roundings, then one to the dtype."""
    x = np.asarray(x)
    N, C, V = x.shape
    xf = widen(x)
    bf = widen(np.full_like(x, fill) if baseline is None else np.asarray(baseline))
    out = np.empty((N, Mc, C, V), x.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            for mc in range(Mc):
                mk = mask(shape, grid, keep, seed, clip0 + n, m0 + mc).reshape(1, V)
                out[n, mc] = narrow(bf[n] + (xf[n] - bf[n]) * mk, x)
    return out


# ---- pasn_rise_scores ----------------------------------------------------------------------------------------------------------------------
def scores_ref(sim, logits, sel, cls, target, K_real):
    """sim (N, M, P), logits (N, M, K), sel (N, k), cls (N,) -> (N, M, k): the prototype kind a copy (float32), the class kind the
    float64 softmax over the first K_real logits read at cls[n]; NaN where the index is out of range."""
    if target == "prototype":
        sim, sel = np.asarray(sim), np.asarray(sel, np.int64)
        N, M, P = sim.shape
        ok = (sel >= 0) & (sel < P)
        got = np.take_along_axis(sim, np.clip(sel, 0, P - 1)[:, None, :].repeat(M, 1), axis=2)
        return np.where(ok[:, None, :], got, F32(np.nan))
    z = np.asarray(logits, np.float64)[..., :K_real]
    cls = np.asarray(cls, np.int64)
    e = np.exp(z - z.max(-1, keepdims=True))
    pr = e / e.sum(-1, keepdims=True)
    ok = (cls >= 0) & (cls < K_real)
    got = np.take_along_axis(pr, np.clip(cls, 0, K_real - 1)[:, None, None].repeat(z.shape[1], 1), axis=2)
    return np.where(ok[:, None, None], got, np.nan)


# ---- pasn_rise_maps ------------------------------------------------------------------------------------------------------------------------
def quantise(sal):
    """pasn_explain_maps' uint8 rule on one map's float32 values."""
    sal = np.asarray(sal, F32)
    lo, hi = sal.min(), sal.max()
    v = (sal - lo) / ((hi - lo) + F32(1e-7))
    return (F32(255.0) * v).astype(np.uint8)


def saliency_ref(scores, shape, grid, keep, seed, clip, norm):
    """scores (M, k) float32 of ONE clip -> (saliency (k, V) float32, maps (k, V) uint8, cov (V,) float64): S and Cov summed with m
    ascending in float64; "coverage": S / Cov, 0 where Cov == 0; "expected": S / (M (keep / 2^32)); rounded to float32 once."""
    scores = np.asarray(scores, F32)
    M, k = scores.shape
    V = int(np.prod(thw(shape)))
    S, cov = np.zeros((k, V), np.float64), np.zeros(V, np.float64)
    for m in range(M):
        mk = mask(shape, grid, keep, seed, clip, m).reshape(V).astype(np.float64)
        cov = cov + mk
        for j in range(k):
            S[j] = S[j] + np.float64(scores[m, j]) * mk
    with np.errstate(invalid="ignore", divide="ignore"):
        if norm == "coverage":
            val = np.where(cov == 0.0, 0.0, S / np.where(cov == 0.0, 1.0, cov))
        else:
            val = S / (np.float64(M) * (np.float64(keep) / 4294967296.0))
    sal = val.astype(F32)
    return sal, np.stack([quantise(sal[j]) for j in range(k)]), cov


# ---- the planted box -----------------------------------------------------------------------------------------------------------------------
BOX_CASE = dict(shape=(4, 24, 24), grid=(2, 4, 4), M=256, p=0.5, seed=11, clip=5, box=(slice(2, None), slice(6, 12), slice(12, 18)))


def box_scores(case=BOX_CASE):
    """(M, 1) float32: the mean of each mask over the box -- a "model" that looks at the box and nowhere else."""
    keep = keep_of(case["p"])
    return np.array([[mask(case["shape"], case["grid"], keep, case["seed"], case["clip"], m)[case["box"]].astype(np.float64).mean()]
                     for m in range(case["M"])]).astype(F32)


def box_summary(sal, case=BOX_CASE):
    """(mean inside, mean outside, argmax inside?) of a saliency volume."""
    sal = np.asarray(sal, np.float64).reshape(case["shape"])
    inside = np.zeros(case["shape"], bool)
    inside[case["box"]] = True
    return float(sal[inside].mean()), float(sal[~inside].mean()), bool(inside.reshape(-1)[int(sal.argmax())])


# ---- the limits of the C ABI ---------------------------------------------------------------------------------------------------------------
def abi_refusals(lib, F32=0, U8=2):
    """{description: return code} of calls that break ONE limit of include/protoasnet_amd.h each (1 = PASN_ERR_ARG is expected of every
    one), plus "good geometry" size queries that must be positive.  The pointers are never dereferenced: every call fails its checks
    before any launch."""
    fake = 256
    geom = dict(T=4, H=24, W=24, gt=2, gh=4, gw=4)

    def apply(N=2, C=3, keep=1 << 31, m0=0, Mc=3, dtype=F32, x=fake, baseline=0, out=fake, **g):
        g = {**geom, **g}
        return lib.pasn_rise_apply(x, baseline, 0.0, N, C, g["T"], g["H"], g["W"], g["gt"], g["gh"], g["gw"], keep, 7, 0, m0, Mc, dtype, out, 0)

    def scores(N=2, M=5, k=2, P=12, K=4, K_real=3, target=0, sim=fake, logits=fake, sel=fake, cls=fake, out=fake):
        return lib.pasn_rise_scores(sim, logits, sel, cls, N, M, k, P, K, K_real, target, out, 0)

    def maps(N=2, k=2, M=5, keep=1 << 31, norm=0, scores=fake, saliency=fake, u8=fake, cov=0, ws=fake, **g):
        g = {**geom, **g}
        return lib.pasn_rise_maps(scores, N, k, M, g["T"], g["H"], g["W"], g["gt"], g["gh"], g["gw"], keep, 7, 0, norm, saliency, u8, cov, ws, 0)

    def size(N=2, k=2, M=5, **g):  # 1: the query refuses (0 bytes)
        g = {**geom, **g}
        return 0 if lib.pasn_rise_maps_workspace_bytes(N, k, M, g["T"], g["H"], g["W"], g["gt"], g["gh"], g["gw"]) else 1

    bad_geometry = (dict(gt=0), dict(gt=17), dict(gh=0), dict(gh=33), dict(gw=0), dict(gw=33), dict(gt=16, gh=21, gw=21),  # 18 * 23 * 23 = 9522 points
                    dict(T=0), dict(H=0), dict(W=0), dict(T=1 << 11, H=1 << 10, W=1 << 10))                              # V = 2^31
    out = {}
    for g in bad_geometry:
        out[f"apply {g}"], out[f"maps {g}"], out[f"size {g}"] = apply(**g), maps(**g), size(**g)
    for bad in (dict(keep=0), dict(C=0), dict(C=65), dict(N=0), dict(N=65536), dict(m0=-1), dict(Mc=0), dict(m0=65535, Mc=1), dict(m0=1, Mc=65535),
                dict(dtype=U8), dict(x=0), dict(out=0), dict(x=258), dict(baseline=258)):
        out[f"apply {bad}"] = apply(**bad)
    for bad in (dict(M=0), dict(M=65536), dict(N=0), dict(k=0), dict(N=256, k=256), dict(target=2), dict(P=0), dict(sim=0), dict(sel=0), dict(out=0),
                dict(target=1, k=2), dict(target=1, k=1, K_real=0), dict(target=1, k=1, K_real=17, K=17), dict(target=1, k=1, K=2),
                dict(target=1, k=1, K=18), dict(target=1, k=1, logits=0), dict(target=1, k=1, cls=0)):
        out[f"scores {bad}"] = scores(**bad)
    for bad in (dict(keep=0), dict(M=0), dict(M=65536), dict(N=0), dict(k=0), dict(N=256, k=256), dict(norm=2), dict(scores=0), dict(ws=0), dict(ws=264),
                dict(saliency=0, u8=0, cov=0)):
        out[f"maps {bad}"] = maps(**bad)
    for bad in (dict(M=0), dict(M=65536), dict(N=0), dict(N=256, k=256)):
        out[f"size {bad}"] = size(**bad)
    out["stage of a bad grid"] = 1 if lib.pasn_rise_stage_masks(0, 4, 4) == 0 and lib.pasn_rise_stage_masks(16, 21, 21) == 0 else 0
    # what is inside the limits passes the checks of the queries (the launching calls are for the GPU tests)
    out["size of a good call"] = 1 - size()
    out["size at the limits"] = 1 - size(gt=16, gh=20, gw=18, M=65535, N=1, k=1)  # 18 * 22 * 20 = 7920 <= 8192 points
    return out
