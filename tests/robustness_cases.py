"""The numpy restatement of the robustness kernels (protoasnet_amd/robustness.py, csrc/corrupt.hip, include/protoasnet_amd.h) and the case
generators of their tests.  The reference has no code for any of this: the restatement IS the specification the kernels are held to.
The corruption is restated step by step in np.float32 (every operation one rounding; bf16 by explicit rounding of the bit pattern), the
statistics in float64.  Philox is the one of tests/bootstrap_cases.py."""
import numpy as np

from bootstrap_cases import philox4x32_10

ZC = np.float32(np.sqrt(3.0) / 2.0 ** 24)  # the fp32 nearest sqrt(3) 2^-24
F0, F1 = np.float32(0.0), np.float32(1.0)


# ---- pasn_clip_corrupt ---------------------------------------------------------------------------------------------------------------------
def widen(raw):
    """Raw elements -> float32: float32 as it is, uint16 as the bit pattern of a bf16."""
    raw = np.asarray(raw)
    if raw.dtype == np.float32:
        return raw
    assert raw.dtype == np.uint16
    return (raw.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow(v, like):
    """float32 -> the raw dtype of `like`: bf16 by rounding the bit pattern to nearest even (no NaN arrives: the clamp removed it)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if like.dtype == np.float32:
        return v
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def z_of(seed, n, q):
    """The Irwin-Hall(4) variate of voxel(s) q of clip(s) n (broadcast together): integers, one conversion, one fp32 product."""
    q, n = np.broadcast_arrays(np.asarray(q, np.uint64), np.asarray(n, np.uint64))
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), n, np.zeros_like(q)], -1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    r = philox4x32_10(ctr, key).astype(np.int64)
    s = (r >> 8).sum(-1) - 33554430
    return s.astype(np.int32).astype(np.float32) * ZC


def z_ref(seed, N, T, H, W):
    """(N, T, H, W) float32: z of every output voxel, q = (t H + h) W + w."""
    return z_of(seed, np.arange(N)[:, None], np.arange(T * H * W)[None, :]).reshape(N, T, H, W)


def _blur_axis(v, taps, axis):
    R, L = (len(taps) - 1) // 2, v.shape[axis]
    acc = np.zeros_like(v)
    for i in range(-R, R + 1):  # from 0.0f, i ascending: acc = acc + (tap * v)
        idx = np.clip(np.arange(L) + i, 0, L - 1)
        acc = acc + np.float32(taps[i + R]) * np.take(v, idx, axis=axis)
    return acc


def corrupt_ref(x, src_t=None, taps=None, row_a=None, row_b=None, sigma_add=0.0, sigma_mul=0.0, seed=0, mean=0.099, std=0.171):
    """x (N, C, T, H, W) raw elements (float32, or the uint16 bit patterns of bf16) -> the corrupted clip in the same raw dtype."""
    x = np.asarray(x)
    N, C, T, H, W = x.shape
    mean, std, sa, sm = np.float32(mean), np.float32(std), np.float32(sigma_add), np.float32(sigma_mul)
    if src_t is not None:
        ts = np.clip(np.asarray(src_t, np.int64), 0, T - 1)
        x = np.stack([x[n][:, ts[n]] for n in range(N)])
    R = 0 if taps is None else (len(taps) - 1) // 2
    photo, noise = row_a is not None or row_b is not None, sa != 0 or sm != 0
    if R == 0 and not photo and not noise:
        return x.copy()
    v = widen(x) * std + mean
    assert v.dtype == np.float32
    if R > 0:
        v = _blur_axis(_blur_axis(v, np.asarray(taps, np.float32), 4), np.asarray(taps, np.float32), 3)
    if photo:
        a = np.ones(H, np.float32) if row_a is None else np.asarray(row_a, np.float32)
        b = np.zeros(H, np.float32) if row_b is None else np.asarray(row_b, np.float32)
        v = a[:, None] * v + b[:, None]
    if noise:
        z = z_ref(seed, N, T, H, W)[:, None]  # shared by the channels
        if sa != 0:
            v = v + sa * z
        if sm != 0:
            v = v + (sm * z) * v
    v = np.fmin(np.fmax(v, F0), F1)  # NaN -> 0
    y = (v - mean) / std
    assert y.dtype == np.float32
    return narrow(y, x)


def descriptor_kwargs(d):
    """A robustness.Corruption as corrupt_ref's keywords."""
    arr = lambda v: None if v is None else np.asarray(v)  # noqa: E731
    return dict(src_t=arr(d.src_t), taps=arr(d.taps), row_a=arr(d.row_a), row_b=arr(d.row_b), sigma_add=d.sigma_add, sigma_mul=d.sigma_mul)


def echo_raw(shape, seed, bf16=False):
    """A seeded normalised clip with speckle-like texture, pixel values inside and a little outside [0, 1]: float32, or bf16 bits."""
    rng = np.random.default_rng(seed)
    pix = rng.random(shape) ** 2 * 1.1 - 0.02
    x = ((pix - 0.099) / 0.171).astype(np.float32)
    return narrow(x, np.zeros(1, np.uint16)) if bf16 else x


# ---- pasn_stability_stats ------------------------------------------------------------------------------------------------------------------
def pred_ref(l, K_real):
    """pasn_explain_rank's prediction: the first maximum of l[:K_real], NaN counts as the largest value."""
    best, bv = 0, l[0]
    for c in range(1, K_real):
        v = l[c]
        if not (bv != bv) and (v > bv or v != v):
            best, bv = c, v
    return best


def select_ref(sim, base, G, k):
    """The first k of the class block by (similarity descending, the HIGHER index first on ties)."""
    return sorted(range(base, base + G), key=lambda p: (-float(sim[p]), -p))[:k]


AGREE_K, AGREE_K_REAL, AGREE_G, AGREE_SELECT, AGREE_GRID = 4, 3, 5, 3, (1, 2, 2)


def agreement_case():
    """Six hand-made clips on which pasn_stability_stats and pasn_explain_rank must report the same class and the same k = 3 prototypes
    (K = 4, K_real = 3, G = 5, P = 20; no NaN similarities).  Returns (logits (6, 4), sim (6, 20), occ (6, 20, 4), fc_w (4, 20),
    pred by hand (6,), sel by hand for the first three clips (3, 3))."""
    nan = np.nan
    logits = np.array([[0.5, 2.0, 1.0, 9.0],   # distinct; the abstain logit is the largest and is not looked at: class 1
                       [0.0, 1.0, 3.0, 0.0],   # class 2
                       [4.0, 1.0, 0.0, 0.0],   # class 0
                       [2.0, nan, 3.0, 0.0],   # NaN at class 1 counts as the largest: class 1
                       [nan, 5.0, 1.0, 0.0],   # NaN at class 0, a larger finite logit after it: class 0
                       [1.0, 1.0, 1.0, 1.0]],  # all equal: class 0
                      np.float32)
    rng = np.random.default_rng(5)
    sim = (np.stack([rng.permutation(20) for _ in range(6)]) / 8.0).astype(np.float32)  # distinct within every clip
    sim[0, 5:10] = [.125, .875, .5, 1.0, .25]  # clip 0, block 1, distinct: 8, 6, 7
    sim[1, 10:15] = [.5, .25, .75, .5, 1.0]    # clip 1, block 2: 14, 12, then 13 and 10 tie across rank k - 1 / k: the HIGHER index is in
    sim[2, 0:5] = .375                         # clip 2, block 0: all equal: 4, 3, 2
    occ = (rng.integers(0, 17, (6, 20, 4)) / 16.0).astype(np.float32)
    fc_w = (rng.integers(-8, 9, (4, 20)) / 8.0).astype(np.float32)
    return logits, sim, occ, fc_w, np.array([1, 2, 0, 1, 0, 0]), np.array([[8, 6, 7], [14, 12, 13], [4, 3, 2]])


def softmax64(l):
    z = np.asarray(l, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def top_set(v, m):
    """The m voxels first in (value descending, index ascending)."""
    return set(np.lexsort((np.arange(len(v)), -np.asarray(v, np.float64)))[:m].tolist())


def pair_ref(a, b, m, grid, degenerate_ok=False):
    """(corr, iou, shift) of two maps (S,) on the grid (Ti, Hi, Wi), float64 in index order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    S = a.size
    mu_a = mu_b = 0.0
    for i in range(S):
        mu_a += a[i]
        mu_b += b[i]
    mu_a, mu_b = mu_a / S, mu_b / S
    saa = sbb = sab = 0.0
    for i in range(S):
        saa += (a[i] - mu_a) * (a[i] - mu_a)
        sbb += (b[i] - mu_b) * (b[i] - mu_b)
        sab += (a[i] - mu_a) * (b[i] - mu_b)
    for s in (saa, sbb):  # a map that is not constant must be well away from it: the correlation is well-conditioned
        assert s == 0.0 or s / S >= 1e-4, s / S
    if saa == 0.0 and sbb == 0.0:
        corr = 1.0
    elif saa == 0.0 or sbb == 0.0:
        corr = 0.0
    else:
        corr = sab / np.sqrt(saa * sbb)
    inter = len(top_set(a, m) & top_set(b, m))
    iou = inter / (2 * m - inter)
    pa, pb = np.unravel_index(int(np.argmax(a)), grid), np.unravel_index(int(np.argmax(b)), grid)  # the first maximum
    diag = sum((g - 1) ** 2 for g in grid)
    shift = float(np.sqrt(float(sum((int(u) - int(w)) ** 2 for u, w in zip(pa, pb)))) / np.sqrt(float(diag))) if diag else 0.0
    return float(corr), float(iou), shift


def stats_ref(la, lb, sa, sb, oa, ob, labels, K_real, k, m, grid):
    """dict(clip (N, 4) f64, correct (N, 2) i32 or None, sel (N, k) i32, pair (N, k, 4) f64) of logits (N, K), sim (N, P), occ (N, P, S)."""
    N, K = la.shape
    P = sa.shape[1]
    G = P // K
    clip, sel, pair = np.zeros((N, 4)), np.zeros((N, k), np.int32), np.zeros((N, k, 4))
    correct = None if labels is None else np.zeros((N, 2), np.int32)
    for n in range(N):
        pa, pb = pred_ref(la[n], K_real), pred_ref(lb[n], K_real)
        qa, qb = softmax64(la[n, :K_real]), softmax64(lb[n, :K_real])
        s_a, s_b = select_ref(sa[n], pa * G, G, k), select_ref(sb[n], pa * G, G, k)
        clip[n] = [float(pa != pb), 0.5 * np.abs(qa - qb).sum(), qa[pa] - qb[pa], len(set(s_a) & set(s_b)) / k]
        sel[n] = s_a
        if labels is not None:
            correct[n] = [pa == labels[n], pb == labels[n]]
        for j, p in enumerate(s_a):
            pair[n, j] = (float(np.float64(sb[n, p]) - np.float64(sa[n, p])),) + pair_ref(oa[n, p], ob[n, p], m, grid)
    return {"clip": clip, "correct": correct, "sel": sel, "pair": pair}


def acc_ref(acc, res, k):
    """acc + the sums over the clips, n ascending."""
    acc = np.array(acc, np.float64)
    N = res["clip"].shape[0]
    for n in range(N):
        acc[:4] += res["clip"][n]
        if res["correct"] is not None:
            acc[4:6] += res["correct"][n]
        acc[6:6 + 4 * k] += res["pair"][n].reshape(-1)
    acc[-1] += N
    return acc


def stats_case(N, K, G, grid, seed):
    """Seeded inputs full of ties: logits and similarities in eighths (clip 0's two best logits tie), maps in sixteenths; clip 1 has
    constant clean maps, clip 2 constant maps on both sides, clip 3 identical maps; the rest differ by noise.  N >= 4."""
    rng = np.random.default_rng(seed)
    P, S = K * G, int(np.prod(grid))
    la = (rng.integers(-16, 17, (N, K)) / 8.0).astype(np.float32)
    lb = (la + rng.integers(-16, 17, (N, K)) / 8.0).astype(np.float32)  # (large enough to flip some predictions)
    la[0, :2] = la[0].max() + 1.0  # a tie for the prediction: the lowest index wins
    sa = (rng.integers(0, 9, (N, P)) / 8.0).astype(np.float32)
    sb = (sa + rng.integers(-1, 2, (N, P)) / 8.0).astype(np.float32)
    oa = (rng.integers(0, 17, (N, P, S)) / 16.0).astype(np.float32)
    ob = np.clip(oa + rng.integers(-4, 5, (N, P, S)) / 16.0, 0.0, 1.0).astype(np.float32)
    oa[1] = 0.25
    oa[2], ob[2] = 0.5, 0.75
    ob[3] = oa[3]
    labels = rng.integers(0, K - 1, N).astype(np.int32)
    return la, lb, sa, sb, oa, ob, labels
