"""Torch CPU restatement of the local-explanation arithmetic (explainability_utils.py:158-200, local_explainability.py:88-125) and the
seeded inputs of the G8 fixture (tests/golden/make_golden_explain.py::case_inputs), shared by test_cpu_explain.py and test_gpu_explain.py."""
import numpy as np
import torch

CASES = [("video_int", (2, 4, 4), (8, 28, 28), 81), ("video_frac", (3, 5, 6), (7, 17, 23), 82), ("image", (5, 6), (37, 45), 83)]
P_MAPS = 2


def case_inputs(grid, out, seed):
    rng = np.random.default_rng(seed)
    occ = np.abs(rng.standard_normal((P_MAPS, 1) + tuple(grid))).astype(np.float32) * np.float32(3.0)
    grey = rng.random((P_MAPS, 1) + tuple(out), dtype=np.float32)
    src = np.repeat((grey - np.float32(0.099)) / np.float32(0.171), 3, axis=1)
    return occ, src


def lut_rgb(lut_bgr):
    """The colour table the kernel takes for cv2's BGR uint8 table: get_heatmap divides by 255 and flips to RGB."""
    return np.ascontiguousarray(np.float32(lut_bgr)[:, ::-1] / 255)


def norm_maps(occ, out):
    """occ (M, 1, *grid) -> normalised maps (M, *out) fp32: torch.nn.Upsample (align_corners=False) + the reference's min-max."""
    occ = torch.as_tensor(occ, dtype=torch.float32)
    mode = "trilinear" if len(out) == 3 else "bilinear"
    u = torch.nn.Upsample(size=tuple(out), mode=mode)(occ)[:, 0]
    dims = tuple(range(1, u.dim()))
    r = u - u.amin(dim=dims, keepdim=True)
    return r / (r.amax(dim=dims, keepdim=True) + 1e-7)


def overlays(maps, src, lut, alpha=0.3, mean=0.099, std=0.171):
    """maps (M, *out) fp32, src (M, C, *out) -> (M, *out, 3): (src * std + mean) + alpha * lut[uint8(255 * maps)]."""
    maps = torch.as_tensor(maps)
    src = torch.as_tensor(src, dtype=torch.float32)
    if src.shape[1] == 1:
        src = src.expand(-1, 3, *src.shape[2:])
    img = torch.movedim(src, 1, -1) * np.float32(std) + np.float32(mean)
    q = (maps * 255).to(torch.uint8).long()
    return img + np.float32(alpha) * torch.as_tensor(lut)[q]


def rank_ref(sim, fc_w, logits, K_real, k_sel=None):
    """(contrib, totals fp64, order, rank, pred, sel) of pasn_explain_rank on the CPU; ties: the higher index first."""
    sim, fc_w, logits = (torch.as_tensor(t, dtype=torch.float32) for t in (sim, fc_w, logits))
    N, P = sim.shape
    K = fc_w.shape[0]
    G = P // K
    contrib = fc_w[None] * sim[:, None, :]
    totals = sim.double() @ fc_w.double().T
    order = torch.empty((N, P), dtype=torch.int64)
    rank = torch.empty((N, P), dtype=torch.int64)
    for c in range(K):
        blk = sim[:, c * G:(c + 1) * G].numpy()
        o = np.argsort(blk, axis=1, kind="stable")[:, ::-1] + c * G  # local_explainability.py:114-117 with a stable sort
        order[:, c * G:(c + 1) * G] = torch.from_numpy(o.copy())
    for n in range(N):
        for c in range(K):
            rank[n, order[n, c * G:(c + 1) * G]] = torch.arange(G)
    pred = logits[:, :K_real].argmax(dim=1)
    sel = None
    if k_sel is not None:
        sel = torch.stack([order[n, int(pred[n]) * G:int(pred[n]) * G + k_sel] for n in range(N)])
    return contrib, totals, order, rank, pred, sel


def u8_mismatch_ok(got_u8, maps_ref, window=1e-5, share=1e-4):
    """uint8 maps against np.uint8(255 * reference): equal except where 255 * v lies within `window` of an integer on the reference side,
    where they may differ by one; such voxels are at most `share` of all voxels.  Returns an error string or None."""
    ref = torch.as_tensor(maps_ref, dtype=torch.float32)
    x = ref * 255
    want = x.to(torch.uint8).long()
    got = torch.as_tensor(got_u8).long().cpu()
    diff = got - want
    near = (x - x.round()).abs() <= window
    bad = (diff != 0) & ~(near & (diff.abs() <= 1))
    if bad.any():
        return f"{int(bad.sum())} uint8 voxels differ outside the near-integer rule (first at {bad.nonzero()[0].tolist()})"
    if int((diff != 0).sum()) > share * diff.numel():
        return f"{int((diff != 0).sum())} of {diff.numel()} uint8 voxels differ"
    return None
