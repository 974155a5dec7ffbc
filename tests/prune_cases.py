"""The float64 / int64 restatement of the prototype-pruning definitions (include/protoasnet_amd.h, "Prototype pruning"), chunk order
included, a brute-force variant that recomputes every masked logit in order, and the inputs the CPU and GPU tests share.  numpy only."""
import numpy as np

CHUNK = 128  # pasn_prune_chunk(); the GPU tests assert that the library agrees


# ---- the definitions ----------------------------------------------------------------------------------------------------------------------
def base_logits(sim, w, kept, K_real):
    """z[n, k] = the fp64 sum of (double)w[k, j] * (double)sim[n, j], sequential, j ascending over the kept prototypes, from 0.0."""
    s, wd = sim.astype(np.float64), w.astype(np.float64)
    z = np.zeros((sim.shape[0], K_real), np.float64)
    for j in range(sim.shape[1]):
        if kept[j]:
            z = z + s[:, j:j + 1] * wd[None, :K_real, j]  # exact products (24 + 24 bits), one rounding per add
    return z


def predictions(z):
    return np.argmax(z, axis=1)  # the first largest: the lowest k on ties


def margins(z, y):
    """z[..., y] - max_{k != y} z[..., k] for rows n with labels y[n]; z is (M, K) or (M, C, K)."""
    yy = y.reshape((-1,) + (1,) * (z.ndim - 1))
    own = np.take_along_axis(z, np.broadcast_to(yy, z.shape[:-1] + (1,)), axis=-1)[..., 0]
    ks = np.arange(z.shape[-1]).reshape((1,) * (z.ndim - 1) + (-1,))
    other = np.where(ks == yy, -np.inf, z).max(axis=-1)
    return own - other


def chunked_sum(m, rows, chunk):
    """Sum over the rows ``rows`` (ascending global indices) of m[rows]: per chunk of ``chunk`` consecutive GLOBAL rows from 0.0 in row
    order, the chunk sums from 0.0 in ascending chunk order.  m is (M, ...): the trailing axes are summed independently."""
    total = np.zeros(m.shape[1:], np.float64)
    M = m.shape[0]
    rows = set(int(r) for r in rows)
    for c0 in range(0, M, chunk):
        part = np.zeros(m.shape[1:], np.float64)
        for n in range(c0, min(M, c0 + chunk)):
            if n in rows:
                part = part + m[n]
        total = total + part
    return total


def tallies_of(zc, z, labels, K_real, chunk):
    """The tallies of the candidate logits zc (M, C, K_real) against the current model's z (M, K_real): wrong (C,), flips (C,), wrong per
    true class (C, K_real), margin_sum (C,)."""
    valid = np.flatnonzero((labels >= 0) & (labels < K_real))
    y = labels[valid].astype(np.int64)
    pc = np.argmax(zc[valid], axis=2)  # (V, C)
    p0 = predictions(z[valid])
    wrong_rows = pc != y[:, None]
    cls = np.zeros((zc.shape[1], K_real), np.int64)
    for k in range(K_real):
        cls[:, k] = wrong_rows[y == k].sum(axis=0)
    flips = (pc != p0[:, None]).sum(axis=0).astype(np.int64)
    mg = np.zeros(zc.shape[:2], np.float64)
    mg[valid] = margins(zc[valid], y)
    return wrong_rows.sum(axis=0).astype(np.int64), flips, cls, chunked_sum(mg, valid, chunk)


def round_table(z, sim, w, labels, kept, K_real, chunk=CHUNK, brute=False):
    """(wrong, flips, wrong per class, margin_sum) with P + 1 rows: row p the model without prototype p (zeros where p is not kept), row P
    the model as it stands.  ``brute``: every ablated logit recomputed in order over the kept set without p, not by the one subtraction."""
    M, P = sim.shape
    s, wd = sim.astype(np.float64), w.astype(np.float64)
    zc = np.empty((M, P + 1, K_real), np.float64)
    for p in range(P):
        if brute and kept[p]:
            k2 = np.array(kept).copy()
            k2[p] = 0
            zc[:, p] = base_logits(sim, w, k2, K_real)
        else:
            zc[:, p] = z - s[:, p:p + 1] * wd[None, :K_real, p]
    zc[:, P] = base_logits(sim, w, kept, K_real) if brute else z
    wrong, flips, cls, ms = tallies_of(zc, zc[:, P], labels, K_real, chunk)
    dead = np.flatnonzero(np.asarray(kept) == 0)
    wrong[dead], flips[dead], cls[dead], ms[dead] = 0, 0, 0, 0.0
    return wrong, flips, cls, ms


def eliminate(sim, w, labels, K_real, proto_class, rounds, floors, accept, max_extra=0, margin_fraction=None, chunk=CHUNK, brute=False):
    """The elimination loop.  Returns a dict: table (the round-0 ``round_table``), removed (rounds,), trace_wrong (rounds, 1 + K_real),
    trace_margin (rounds,), kept (P,), z (M, K_real)."""
    M, P = sim.shape
    s, wd = sim.astype(np.float64), w.astype(np.float64)
    kept = np.ones(P, np.int64)
    z = base_logits(sim, w, kept, K_real)
    tab = round_table(z, sim, w, labels, kept, K_real, chunk, brute)
    table0 = tab
    wrong0, margin0 = int(tab[0][P]), float(tab[3][P])
    removed, tw, tm = np.full(rounds, -1, np.int64), np.zeros((rounds, 1 + K_real), np.int64), np.zeros(rounds, np.float64)
    stop = False
    for r in range(rounds):
        if stop:
            tw[r], tm[r] = tw[r - 1], tm[r - 1]
            continue
        wrong, _, cls, ms = tab
        counts = np.bincount(np.asarray([proto_class[p] for p in range(P) if kept[p] and 0 <= proto_class[p] < K_real], np.int64), minlength=K_real)
        best = -1
        for p in range(P):
            c = int(proto_class[p])
            if not kept[p] or c < 0 or c >= K_real or counts[c] <= floors[c]:
                continue
            if best < 0 or wrong[p] < wrong[best] or (wrong[p] == wrong[best] and ms[p] > ms[best]):
                best = p
        ok = best >= 0
        if ok and accept:
            ok = wrong[best] <= wrong0 + max_extra
            if ok and margin_fraction is not None:
                ok = ms[best] >= np.float64(margin_fraction) * np.float64(margin0)
        src = best if ok else P
        tw[r, 0], tw[r, 1:], tm[r] = wrong[src], cls[src], ms[src]
        if not ok:
            stop = True
            continue
        removed[r] = best
        kept[best] = 0
        z = base_logits(sim, w, kept, K_real) if brute else z - s[:, best:best + 1] * wd[None, :K_real, best]
        if r + 1 < rounds:
            tab = round_table(z, sim, w, labels, kept, K_real, chunk, brute)
    return {"table": table0, "removed": removed, "trace_wrong": tw, "trace_margin": tm, "kept": kept, "z": z}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def class_major(P, K):
    """Class of each prototype, class-major, the remainder to the first classes."""
    per, extra = divmod(P, K)
    return np.repeat(np.arange(K), [per + (k < extra) for k in range(K)]).astype(np.int32)


def make_case(M, P, K, K_real, seed, dyadic=False, unlabeled=0.0, informative=0.0, wide=False):
    """sim (M, P) fp32 in [0, 1], w (K, P) fp32 with |w| <= 2, labels (M,) int32 (a fraction ``unlabeled`` of them -1), proto_class (P,).
    ``dyadic``: multiples of 1/8, so that every fp64 sum is exact.  ``informative`` > 0: the last layer favours a prototype's own class
    and the similarities of the label's prototypes are raised by it, so that the model is mostly right and prototypes are redundant.
    ``wide``: magnitudes spread over many binades, so that the fp64 sums ROUND and their order shows (uniform fp32 numbers are multiples of
    2^-24: a few hundred products of them add exactly in fp64, in any order)."""
    rng = np.random.default_rng(seed)
    pc = class_major(P, K)
    labels = rng.integers(0, K_real, M).astype(np.int32)
    if dyadic:
        sim = rng.integers(0, 9, (M, P)).astype(np.float32) / 8
        w = rng.integers(-16, 17, (K, P)).astype(np.float32) / 8
    else:
        sim = rng.random((M, P), dtype=np.float32)
        w = (rng.random((K, P), dtype=np.float32) * 4 - 2).astype(np.float32)
    if wide:
        sim = np.maximum(sim.astype(np.float64) ** 8, 2.0 ** -100).astype(np.float32)  # (no fp32 denormals)
        w = (np.sign(w) * 2 * (np.abs(w.astype(np.float64)) / 2) ** 5).astype(np.float32)
    if informative > 0:
        own = (pc[None, :] == np.arange(K)[:, None])
        w = np.where(own, np.float32(1.0), np.float32(-0.5) * w.astype(np.float32) * np.float32(0.25)).astype(np.float32)
        boost = (pc[None, :] == labels[:, None]) * np.float32(informative)
        sim = np.minimum(sim * np.float32(0.5) + boost.astype(np.float32), np.float32(1.0)).astype(np.float32)
        if dyadic:
            sim, w = np.round(sim * 8).astype(np.float32) / 8, np.round(w * 8).astype(np.float32) / 8
    if unlabeled > 0:
        labels[rng.random(M) < unlabeled] = -1
    return sim, w, labels, pc


def floors_for(K_real, g):
    return [int(g)] * K_real


def rounds_for(pc, K_real, floors):
    counts = np.bincount(pc[pc < K_real], minlength=K_real)
    return int(np.maximum(counts - np.asarray(floors), 0).sum())
