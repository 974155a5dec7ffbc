"""Inputs and fp64 references of the kernel-level training tests (tests/test_gpu_train.py), pure torch on the CPU.

Shared by the GPU tests, which run the HIP kernels on these inputs, and tests/test_cpu_train_kernel_cases.py, which checks without a
GPU that the references are right (against autograd / an independent restatement) and that the inputs have the properties the
comparisons rely on: nothing at a ReLU kink, unambiguous arg-mins, enough tied pooling windows, bounds that discriminate.

Every activation tensor is rounded to the compute dtype BEFORE the reference is taken, so a bf16 case compares the kernel with the
exact result on the operands it actually reads; what is left is the kernel's own accumulation and the rounding of its stores."""
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS_BN, MOMENTUM = 1e-5, 0.1
KINK = 1e-5            # |u| < KINK * max|u|: a pre-activation two correct implementations may put on either side of a ReLU
BF16_STORE = 2.0 ** -8  # allowance per bf16 store: round-to-nearest is within 2^-9 relative, the factor 2 is the margin


def rnd(x, dtype):
    """fp32 tensor -> what a kernel of compute dtype `dtype` reads, as fp64."""
    return x.float().to(dtype).to(F64)


def tol_stores(fp32_tol, k, dtype):
    """Bound (as a fraction of the tensor's scale) of an elementwise output behind k stores in the compute dtype."""
    return fp32_tol + (k * BF16_STORE if dtype == torch.bfloat16 else 0.0)


# ------------------------------------------------------------------------------------------------- grid geometry
def row_geom(n, s, cp, contig=False, blocks=1024):
    """CPU replica of row_geom() in csrc/train.hip: how the passes over [N][S][Cp] rows cut a clip into chunks."""
    cg = cp // 8
    lpr = 1
    while lpr < cg:
        lpr <<= 1
    if contig:
        lpr = cg
    rl = 256 // lpr
    want = max(1, blocks // max(1, n))
    maxc = max(1, s // (rl * 16))
    chunks = min(want, maxc)
    rpc = -(-s // chunks)
    chunks = -(-s // rpc)
    return dict(CG=cg, LPR=lpr, RL=rl, chunks=chunks, rows_per_chunk=rpc, live_threads=rl * lpr)


# (c, (n, t, h, w), offset): the first three are the single-chunk cases the suite has always had; the fourth has fewer rows in a clip
# (S = 25) than a block has row lanes (64, or 85 with PASN_TRAIN_ROWS_CONTIG): most threads never load a row and still join the block reduce
UNIT_CASES = [(54, (3, 4, 9, 7), 0.0), (24, (2, 3, 16, 16), 300.0), (432, (2, 2, 3, 3), -5.0), (24, (2, 1, 5, 5), 0.0),
              (432, (2, 3, 7, 7), 0.0), (54, (3, 3, 21, 19), 0.0), (24, (2, 3, 31, 31), 0.0)]
UNIT_MULTI_CHUNK = UNIT_CASES[4:]
# (c, (n, t, h, w), groups)
GROUP_CASES = [(54, (4, 3, 9, 7), 2), (24, (6, 2, 8, 8), 3), (216, (2, 2, 5, 4), 2), (54, (4, 3, 21, 19), 2)]
GROUP_MULTI_CHUNK = GROUP_CASES[3:]
# (n, c, cse, (t, h, w))
SE_CASES = [(3, 54, 8, (2, 5, 6)), (3, 432, 32, (3, 7, 7)), (3, 54, 8, (3, 21, 19))]
SE_MULTI_CHUNK = SE_CASES[1:]


# ------------------------------------------------------------------------------------------------- norm unit
def _bn_forward(y, gamma, beta, groups):
    """Train-mode batch norm of `groups` runs of consecutive clips, each with its own statistics.  y: (N, C, S) fp64."""
    n, c, s = y.shape
    yg = y.view(groups, n // groups, c, s)
    mean = yg.mean(dim=(1, 3))                                          # (G, C)
    var = ((yg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    invstd = 1.0 / torch.sqrt(var + EPS_BN)
    yhat = ((yg - mean[:, None, :, None]) * invstd[:, None, :, None]).reshape(n, c, s)
    u = yhat * gamma[None, :, None] + beta[None, :, None]
    return mean, var, invstd, yhat, u


def _bn_backward(dpre, yhat, gamma, invstd, groups):
    """Gradient of the norm given dL/d(norm output): (dy, dgamma, dbeta, coef (G, 2, C) = (mean d, mean d yhat) per group)."""
    n, c, s = dpre.shape
    dg, yg = dpre.view(groups, n // groups, c, s), yhat.view(groups, n // groups, c, s)
    m1, m2 = dg.mean(dim=(1, 3)), (dg * yg).mean(dim=(1, 3))
    dy = (gamma * invstd)[:, None, :, None] * (dg - m1[:, None, :, None] - yg * m2[:, None, :, None])
    return dy.reshape(n, c, s), (dpre * yhat).sum(dim=(0, 2)), dpre.sum(dim=(0, 2)), torch.stack([m1, m2], dim=1)


def _running(mean, var, rows, c):
    rm, rv = torch.zeros(c, dtype=F64), torch.ones(c, dtype=F64)
    for k in range(mean.shape[0]):  # group by group, in order
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean[k]
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var[k] * rows / (rows - 1)
    return rm, rv


def _kink_band(u):
    return u.abs() < KINK * float(u.abs().max())


def unit_case(c, shape, offset=0.0, dtype=torch.float32, groups=1):
    """relu(batch_norm(y) + res) and, for one group without offset, relu(batch_norm(y)) (the unit without residual: mode 3 + lazy apply).

    Inputs as the suite has always drawn them (same seeds), then moved clear of the ReLU kink: an element whose reference pre-activation
    lies within 10 * KINK of zero gets 1/8 added (to y where it decides the unit without residual, to res otherwise) -- a flipped mask
    moves a whole channel's sums by d / R, so no bound on them could hold across two correct implementations otherwise."""
    n, t, h, w = shape
    s, gd = t * h * w, shape[0] // groups
    g = torch.Generator().manual_seed(c + groups if groups > 1 else c)
    y = torch.randn(n, c, t, h, w, generator=g) * 2 + offset
    if groups > 1:
        y = y + torch.arange(n).view(n, 1, 1, 1, 1) // gd * 1.5  # groups with different means
    res = torch.randn(n, c, t, h, w, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    da = torch.randn(n, c, t, h, w, generator=g)
    plain = offset == 0.0 and groups == 1
    gm, bt = gamma.to(F64), beta.to(F64)
    for _ in range(8):
        yr, rr = rnd(y, dtype).view(n, c, s), rnd(res, dtype).view(n, c, s)
        _, _, _, _, u0 = _bn_forward(yr, gm, bt, groups)
        near0 = (u0.abs() < 10 * KINK * float(u0.abs().max())).view_as(y) if plain else torch.zeros_like(y, dtype=torch.bool)
        near1 = ((u0 + rr).abs() < 10 * KINK * float((u0 + rr).abs().max())).view_as(y)
        if not bool(near0.any() | near1.any()):
            break
        y = torch.where(near0, y + 0.125, y)
        res = torch.where(near1 & ~near0, res + 0.125, res)
    y, res, da = (x.to(dtype).float() for x in (y, res, da))
    yr, rr, dr = (x.to(F64).view(n, c, s) for x in (y, res, da))
    mean, var, invstd, yhat, u0 = _bn_forward(yr, gm, bt, groups)
    u = u0 + rr
    dpre = dr * (u > 0)
    dy, dgamma, dbeta, coef = _bn_backward(dpre, yhat, gm, invstd, groups)
    rm, rv = _running(mean, var, gd * s, c)
    v5 = lambda x: x.view(n, c, t, h, w)
    case = dict(n=n, c=c, cp=(c + 7) // 8 * 8, S=s, thw=(t, h, w), groups=groups, dtype=dtype, offset=offset,
                y=y, res=res, gamma=gamma, beta=beta, da=da,
                u=v5(u), out=v5(torch.relu(u)), mean=mean, invstd=invstd, running_mean=rm, running_var=rv,
                dres=v5(dpre), dy=v5(dy), dgamma=dgamma, dbeta=dbeta, coef=coef, yhat=v5(yhat))
    if plain:
        dpre0 = dr * (u0 > 0)
        dy0, dgamma0, dbeta0, coef0 = _bn_backward(dpre0, yhat, gm, invstd, 1)
        case.update(u_plain=v5(u0), out_plain=v5(torch.relu(u0)), dy_plain=v5(dy0), dgamma_plain=dgamma0, dbeta_plain=dbeta0, coef_plain=coef0)
    return case


# ------------------------------------------------------------------------------------------------- squeeze-excite unit
def _swish_grad(v):
    sg = torch.sigmoid(v)
    return sg * (1 + v * (1 - sg))


def se_case(n, c, cse, thw, dtype=torch.float32):
    """out = swish(u * gate),  u = batch_norm(y),  gate = sigmoid(w2 relu(w1 mean_s(u) + b1) + b2)  (an X3D block with squeeze-excite).

    Two references of the backward, identical in fp32:
      * `two_pass`: what modes 1 + 2 + the plain apply compute -- mode 2 reads the d' = d swish'(.) that mode 1 STORED, so its sums (coef,
        dgamma, dbeta) and everything behind them see d' rounded to the compute dtype, and the apply pass reads a stored d'' in turn;
      * `analytic`: mode 4 takes every sum from the unrounded d'; only the apply pass reads the stored d'."""
    t, h, w = thw
    s = t * h * w
    g = torch.Generator().manual_seed(7)
    y = torch.randn(n, c, t, h, w, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    w1, b1 = torch.randn(cse, c, generator=g) * 0.3, torch.randn(cse, generator=g)
    w2, b2 = torch.randn(c, cse, generator=g) * 0.3, torch.randn(c, generator=g)
    da = torch.randn(n, c, t, h, w, generator=g)
    y, da = y.to(dtype).float(), da.to(dtype).float()
    P = [x.to(F64) for x in (gamma, beta, w1, b1, w2, b2)]
    yr, dr = y.to(F64).view(n, c, s), da.to(F64).view(n, c, s)
    mean, var, invstd, yhat, u = _bn_forward(yr, P[0], P[1], 1)
    pool = u.mean(dim=2)                                                  # (N, C)
    pre1 = pool @ P[2].t() + P[3]
    hid = torch.relu(pre1)
    gate = torch.sigmoid(hid @ P[4].t() + P[5])                           # (N, C)
    v = u * gate[:, :, None]
    out = v * torch.sigmoid(v)
    dv = dr * _swish_grad(v)                                              # d' (what modes 1 and 4 store)
    dgate = (dv * u).sum(dim=2)
    dpre2 = dgate * gate * (1 - gate)
    dh = (dpre2 @ P[4]) * (pre1 > 0)
    grads = dict(dw2=dpre2.t() @ hid, db2=dpre2.sum(0), dw1=dh.t() @ pool, db1=dh.sum(0))
    add = (dh @ P[2]) / s                                                 # (N, C): dL/dpool / S

    def norm_bwd(dv_read, round_d2):
        d2 = dv_read * gate[:, :, None] + add[:, :, None]                 # d''
        _, dgamma, dbeta, coef = _bn_backward(d2, yhat, P[0], invstd, 1)
        d2r = rnd(d2, dtype) if round_d2 else d2
        dy = (P[0] * invstd[0])[None, :, None] * (d2r - coef[0, 0][None, :, None] - yhat * coef[0, 1][None, :, None])
        return dict(dy=dy.view(n, c, t, h, w), dgamma=dgamma, dbeta=dbeta, coef=coef[0], **grads)

    dv_stored = rnd(dv, dtype)
    two_pass = norm_bwd(dv_stored, True)
    analytic = norm_bwd(dv, False)
    analytic["dy"] = ((P[0] * invstd[0])[None, :, None] * (dv_stored * gate[:, :, None] + add[:, :, None] - analytic["coef"][0][None, :, None]
                                                            - yhat * analytic["coef"][1][None, :, None])).view(n, c, t, h, w)
    exact = norm_bwd(dv, False)  # no store rounded: autograd's gradient
    return dict(n=n, c=c, cp=(c + 7) // 8 * 8, cse=cse, S=s, thw=thw, dtype=dtype, y=y, da=da, params=(gamma, beta, w1, b1, w2, b2),
                out=out.view(n, c, t, h, w), u=u.view(n, c, t, h, w), pool=pool, gate=gate, pre1=pre1, mean=mean[0], invstd=invstd[0], dv=dv.view(n, c, t, h, w),
                add=add, two_pass=two_pass, analytic=analytic, exact=exact)


# ------------------------------------------------------------------------------------------------- max pooling
# (n, c, (t, h, w), kernel, stride, padding)
MAXPOOL_CASES = [
    (2, 64, (1, 15, 14), (1, 3, 3), (1, 2, 2), (0, 1, 1)),   # the ResNet stem geometry, an odd and an even plane extent
    (2, 20, (1, 9, 11), (1, 3, 3), (1, 2, 2), (0, 1, 1)),    # Cp = 24: padded channels
    (1, 16, (5, 8, 7), (3, 3, 3), (2, 2, 2), (1, 1, 1)),     # 3-D overlapping windows
    (2, 8, (2, 6, 6), (2, 2, 2), (2, 2, 2), (0, 0, 0)),      # non-overlapping windows
]


def pool_out(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def pool_windows(x, k, s, p):
    """(N, C, To, Ho, Wo, kt*kh*kw) window contents in scan order (t, h, w), out-of-range positions -inf, and the linear input index
    (into T*H*W) of every window slot (-1 out of range)."""
    n, c, t, h, w = x.shape
    xp = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]), value=float("-inf"))
    idx = torch.arange(t * h * w, dtype=F64).view(1, 1, t, h, w)
    ip = F.pad(idx, (p[2], p[2], p[1], p[1], p[0], p[0]), value=-1.0)
    unf = lambda a: a.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2]).reshape(*a.shape[:2], *[pool_out(i, kk, ss, pp) for i, kk, ss, pp in zip((t, h, w), k, s, p)], -1)
    return unf(xp), unf(ip).long()


def pool_route(x, dy, k, s, p, pick="first"):
    """Max-pool backward restated: every window sends its dy to ONE of its maxima -- the first in scan order (the contract of
    pasn_maxpool3d_bwd and what torch's CPU kernel records), or the last (the corruption the bounds must detect)."""
    n, c, t, h, w = x.shape
    win, lin = pool_windows(x, k, s, p)
    kk = win.shape[-1]
    is_max = win == win.max(dim=-1, keepdim=True).values
    order = torch.arange(kk, 0, -1) if pick == "first" else torch.arange(1, kk + 1)
    slot = (is_max * order).argmax(dim=-1, keepdim=True)
    target = lin.expand_as(win).gather(-1, slot).squeeze(-1)              # (N, C, To, Ho, Wo) or (1, 1, ...) broadcast
    dx = torch.zeros(n, c, t * h * w, dtype=dy.dtype)
    dx.scatter_add_(2, target.reshape(n, c, -1), dy.reshape(n, c, -1))
    return dx.view(n, c, t, h, w)


def maxpool_case(i, dtype=torch.float32):
    """relu(randn) with the zeros of a real post-ReLU map: besides the half of the entries the ReLU clips one by one, 4 x 4 spatial blocks
    are dark as a whole (independent zeros alone leave a 3 x 3 window all-zero once in 512 times; with the blocks more than a fifth of
    the windows have a tied, zero maximum, as behind the ResNet stem).  The first channel group of clip 0 is all zeros (every window
    tied, the border windows with their first in-range element away from the window's origin); in bf16 one plane holds four distinct
    values only.  Reference: F.max_pool3d and its autograd in fp64."""
    n, c, thw, k, s, p = MAXPOOL_CASES[i]
    g = torch.Generator().manual_seed(40 + i)
    x = torch.relu(torch.randn(n, c, *thw, generator=g))
    lit = (torch.rand(n, c, 1, (thw[1] + 3) // 4, (thw[2] + 3) // 4, generator=g) > 0.35).float()
    x = x * lit.repeat_interleave(4, dim=3).repeat_interleave(4, dim=4)[..., :thw[1], :thw[2]]
    x[0, :8] = 0.0
    if dtype == torch.bfloat16:
        x[n - 1, c - 1] = torch.round(torch.rand(*thw, generator=g) * 3) / 2
    x = x.to(dtype).float()
    xr = x.to(F64).requires_grad_()
    y = F.max_pool3d(xr, k, s, p)
    dy = torch.randn(y.shape, generator=g).to(dtype).float()
    y.backward(dy.to(F64))
    return dict(n=n, c=c, cp=(c + 7) // 8 * 8, thw=thw, k=k, s=s, p=p, dtype=dtype, x=x, dy=dy, y=y.detach(), dx=xr.grad)


# ------------------------------------------------------------------------------------------------- ProtoPNet head
# (n, s, d, p, k) drawn at random, and two constructed cases
HEAD_CASES = {"r512": (3, 25, 512, 30, 3), "r128": (2, 49, 128, 12, 3), "s1": (4, 1, 64, 9, 4), "dp16": (2, 9, 12, 33, 3),
              "shared": (2, 12, 40, 10, 3), "exact": (2, 12, 40, 10, 3)}
HEAD_SEEDS = {"r512": 365, "r128": 2, "s1": 1, "dp16": 3, "shared": 1, "exact": 1}  # searched: every arg-min gap above GAP, in both dtypes
HEAD_SHARED = 5  # prototypes 0 .. 4 of the constructed case sit around row 3 of clip 0
GAP = 1e-3       # the two smallest distances of a (clip, prototype) differ by more than GAP * d_min


def head_reference(z, protos, fcw, dlogits, dmin, activation):
    """fp64 autograd of oracle.heads.ppnet_head's expression.  z: (N, S, D)."""
    import oracle

    n, s, d = z.shape
    zz = z.to(F64).requires_grad_()
    pv, fw = protos.to(F64).requires_grad_(), fcw.to(F64).requires_grad_()
    x = zz.permute(0, 2, 1).reshape(n, d, s, 1)
    sd = {"prototype_vectors": pv.view(-1, d, 1, 1), "ones": torch.ones(pv.shape[0], d, 1, 1, dtype=F64), "last_layer.weight": fw}
    out = oracle.heads.ppnet_head(sd, x, "log" if activation == 0 else "linear")
    out["min_distances"].retain_grad()
    ((out["logits"] * dlogits.to(F64)).sum() + (out["min_distances"] * dmin.to(F64)).sum()).backward()
    dist = out["distances"].detach().view(n, -1, s)
    return dict(dist=dist, min_dist=out["min_distances"].detach(), argmin=dist.argmin(dim=2), logits=out["logits"].detach(),
                dz=zz.grad, dprotos=pv.grad, dfc_w=fw.grad, coef=out["min_distances"].grad)


def head_case(tag, dtype=torch.float32, activation=0, with_dmin=True):
    """Latent rows, prototypes and loss weights on both outputs of head A.  In a bf16 case the rows AND the prototypes are bf16 values (the
    forward kernel feeds the prototypes to the matrix cores in the compute dtype; the backward reads them in fp32 -- representable
    prototypes give both one reference).  The constructed cases live on the grid k/16, where every product and sum of the distance
    expansion is exact in fp32: their distances carry no cancellation noise, d == 0 is exactly 0."""
    n, s, d, p, k = HEAD_CASES[tag]
    g = torch.Generator().manual_seed(HEAD_SEEDS[tag])
    if tag in ("shared", "exact"):
        grid = lambda *sh: torch.randint(0, 17, sh, generator=g).float() / 16
        z, protos = grid(n, s, d), grid(p, d)
        if tag == "shared":
            for j in range(HEAD_SHARED):  # distinct small offsets from row 3 of clip 0: +-1/16 on 4 + 2j channels
                off = torch.zeros(d)
                off[3 * j:3 * j + 4 + 2 * j] = (torch.randint(0, 2, (4 + 2 * j,), generator=g).float() * 2 - 1) / 16
                protos[j] = z[0, 3] + off
        else:
            protos[4] = z[1, 7]       # the state right after a prototype push
    else:
        z, protos = torch.rand(n, s, d, generator=g), torch.rand(p, d, generator=g)
    fcw, dlogits = torch.randn(k, p, generator=g), torch.randn(n, k, generator=g)
    dmin = torch.randn(n, p, generator=g) * 0.25 if with_dmin else torch.zeros(n, p)
    z = z.to(dtype).float()
    if dtype == torch.bfloat16:
        protos = protos.to(dtype).float()
    ref = head_reference(z, protos, fcw, dlogits, dmin, activation)
    shared = torch.zeros(n, s, dtype=torch.long).scatter_add_(1, ref["argmin"], torch.ones(n, p, dtype=torch.long))  # prototypes per row
    return dict(n=n, S=s, D=d, Dp=(d + 7) // 8 * 8, P=p, K=k, dtype=dtype, activation=activation, z=z, protos=protos, fcw=fcw,
                dlogits=dlogits, dmin=dmin if with_dmin else None, shared=shared, **ref)


# ------------------------------------------------------------------------------------------------- XProtoNet tail
# (n, s, d, p, k)
XPROTO_CASES = [(3, 37, 64, 30, 3), (2, 300, 12, 30, 3)]


def xproto_case(i, occ_only, dtype=torch.float32):
    """occ = |r|, feat = sum_s occ z, sim = (cos(feat, proto) + 1) / 2, logits = sim W^T with loss weights on logits, sim and occ."""
    n, s, d, p, k = XPROTO_CASES[i]
    g = torch.Generator().manual_seed(11)
    z, r = torch.randn(n, d, s, generator=g).to(dtype).float(), torch.randn(n, p, s, generator=g).to(dtype).float()
    protos, fcw = torch.rand(p, d, generator=g), torch.randn(k, p, generator=g)
    dl, dsm, doc = torch.randn(n, k, generator=g), torch.randn(n, p, generator=g), torch.randn(n, p, s, generator=g)
    zz, rr, pv, fw = (x.to(F64).requires_grad_() for x in (z, r, protos, fcw))
    occ = rr.abs()
    feat = torch.einsum("nps,nds->npd", occ, zz)
    sim = (F.cosine_similarity(feat, pv.unsqueeze(0), dim=2, eps=1e-8) + 1) / 2
    logits = F.linear(sim, fw)
    if occ_only:
        (occ * doc).sum().backward()
    else:
        ((logits * dl).sum() + (sim * dsm).sum() + (occ * doc).sum()).backward()
    return dict(n=n, S=s, D=d, Dp=(d + 7) // 8 * 8, P=p, Pp=(p + 7) // 8 * 8, K=k, dtype=dtype, z=z, r=r, protos=protos, fcw=fcw, dl=dl, dsm=dsm,
                doc=doc, occ=occ.detach(), feat=feat.detach(), sim=sim.detach(), logits=logits.detach(), dr=rr.grad,
                dz=zz.grad, dprotos=pv.grad, dfcw=fw.grad)
