"""The numpy restatement of the faithfulness kernels (protoasnet_amd/faithfulness.py, csrc/perturb.hip, include/protoasnet_amd.h) and the
map / count generators of their tests.  The reference has no code for any of this: the restatement IS the specification the kernels are
held to.  Integers and bit patterns throughout, float64 for the curves."""
import numpy as np


# ---- pasn_perturb_steps --------------------------------------------------------------------------------------------------------------------
def positions(maps):
    """maps (M, V) uint8 -> pos (M, V) int64: a voxel's place in its map's (level descending, flat index ascending) order."""
    maps = np.asarray(maps)
    M, V = maps.shape
    index = np.arange(V)
    pos = np.empty((M, V), np.int64)
    for m in range(M):
        order = np.lexsort((index, -maps[m].astype(np.int64)))  # the last key is the primary one
        pos[m, order] = index
    return pos


def steps_of_positions(pos, counts):
    """steps[v] = the number of s with counts[s] <= pos[v].  Small volumes count, entry by entry; large ones use that counts is
    non-decreasing: the s with counts[s] <= p are a prefix, and searchsorted gives its length (test_cpu_faithfulness holds the two equal)."""
    counts = np.asarray(counts, np.int64)
    assert counts.ndim == 1 and 1 <= counts.size <= 64 and np.all(np.diff(counts) >= 0)
    if pos.size * counts.size <= 1 << 22:
        return (counts[None, None, :] <= pos[:, :, None]).sum(-1).astype(np.uint8)
    return np.searchsorted(counts, pos, side="right").astype(np.uint8)


def steps_ref(maps, counts):
    return steps_of_positions(positions(maps), counts)


def _steps_sorted_equal(maps, counts):
    """Both arms of steps_of_positions on one input."""
    pos, c = positions(maps), np.asarray(counts, np.int64)
    return np.array_equal((c[None, None, :] <= pos[:, :, None]).sum(-1), np.searchsorted(c, pos, side="right"))


def steps_brute(level, counts):
    """O(V^2), straight from the definition: pos(v) = the voxels that come before v."""
    V = len(level)
    out = []
    for v in range(V):
        pos = sum(1 for u in range(V) if level[u] > level[v] or (level[u] == level[v] and u < v))
        out.append(sum(1 for c in counts if c <= pos))
    return np.array(out, np.uint8)


# ---- pasn_perturb_apply --------------------------------------------------------------------------------------------------------------------
def apply_ref(x, steps, step_ids, mode, baseline=None, fill=0):
    """x (N, C, V) raw elements (float32, or the uint16 bit patterns of bf16), steps (N, k, V) uint8, step_ids (Sc,), mode 0 deletion /
    1 insertion, baseline like x or None (then the scalar `fill`, already in x's raw dtype) -> (N, k, Sc, C, V): element by element a copy."""
    x, steps, ids = np.asarray(x), np.asarray(steps), np.asarray(step_ids, np.int64)
    touched = steps[:, :, None, None, :].astype(np.int64) <= ids[None, None, :, None, None]  # (N, k, Sc, 1, V)
    base = np.full_like(x, fill) if baseline is None else np.asarray(baseline)
    assert base.dtype == x.dtype and base.shape == x.shape
    from_x = touched if mode == 1 else ~touched
    return np.where(from_x, x[:, None, None], base[:, None, None])


# ---- pasn_perturb_curves -------------------------------------------------------------------------------------------------------------------
def trapezoid(y, counts, V):
    """sum_{s >= 1} (x_s - x_{s-1}) (y_s + y_{s-1}) / 2 over the last axis, x_s = counts[s] / V, float64, s ascending."""
    y = np.asarray(y, np.float64)
    xs = np.asarray(counts, np.float64) / np.float64(V)
    area = np.zeros(y.shape[:-1], np.float64)
    for s in range(1, y.shape[-1]):
        area = area + (xs[s] - xs[s - 1]) * (y[..., s] + y[..., s - 1]) / 2.0
    return area


def curves_ref(sim, logits, sel, cls, counts, V, K_real):
    """sim (N, k, S1, P), logits (N, k, S1, K), sel (N, k), cls (N,) -> curve_sim (a copy), curve_prob (float64 softmax over the first
    K_real logits, read at cls[n]), auc (N, k, 2) of those float64 curves."""
    sim, logits = np.asarray(sim), np.asarray(logits, np.float64)
    N, k, S1, _ = sim.shape
    cs = np.take_along_axis(sim, np.asarray(sel, np.int64)[:, :, None, None].repeat(S1, 2), axis=3)[..., 0]
    z = logits[..., :K_real]
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    cp = np.take_along_axis(p, np.asarray(cls, np.int64)[:, None, None, None].repeat(k, 1).repeat(S1, 2), axis=3)[..., 0]
    auc = np.stack([trapezoid(cs, counts, V), trapezoid(cp, counts, V)], -1)
    return cs, cp, auc


# ---- maps and counts of the tests ----------------------------------------------------------------------------------------------------------
def staircase(V, counts, rng):
    """A map whose level boundaries coincide with `counts` (strictly increasing, 0 first, V last): the counts[s] - counts[s-1] voxels of
    stair s, scattered over the volume, share level 250 - 40 s -- no level straddles a count."""
    m = np.empty(V, np.uint8)
    perm = rng.permutation(V)
    for s in range(1, len(counts)):
        m[perm[counts[s - 1]:counts[s]]] = 250 - 40 * s
    return m


def synthetic_maps(M, V, seed):
    """{name: (M, V) uint8}: constant (the order is the index), two levels, uniform random, a staircase on step_counts(V, 4)."""
    from protoasnet_amd.faithfulness import step_counts

    rng = np.random.default_rng(seed)
    return {
        "constant": np.full((M, V), 77, np.uint8),
        "two_levels": np.where(rng.random((M, V)) < 0.3, 200, 10).astype(np.uint8),
        "uniform": rng.integers(0, 256, (M, V), dtype=np.uint8),
        "staircase": np.stack([staircase(V, step_counts(V, 4), rng) for _ in range(M)]),
    }


def count_sets(V):
    """{name: counts}: the default ten steps; repeats with a last entry below V (the value S1 appears); one voxel; all but one; the
    staircase's own counts; 64 entries."""
    from protoasnet_amd.faithfulness import step_counts

    return {
        "ten": step_counts(V, 10),
        "repeats_short": [0, 0, V // 3, V // 3, V // 2],
        "one": [1],
        "all_but_one": [V - 1],
        "stairs": step_counts(V, 4),
        "sixty_four": step_counts(V, fractions=[i / 63 for i in range(64)]),
    }
