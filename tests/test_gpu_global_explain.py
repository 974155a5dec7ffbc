"""GPU: global explanations.  Kernel level: pasn_topk_xproto_update / pasn_topk_gather / pasn_proto_class_stats on synthetic distances
against torch.sort(stable=True) -- exactly.  Through the models: global_explain.nearest_clips / nearest_maps against the same sort of the
push_forward products the test collects itself, against the push at k = 1, and the DPTrainer methods' files."""
import os
import pickle

import numpy as np
import pytest
import torch

from protoasnet_amd import _lib, global_explain, push, synth
from test_cpu_trainer import TRAIN_CFG
from util import CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")


# ------------------------------------------------------------------------------------------------- kernel level
def _problem(P, K, N, seed, levels=5):
    """Distances from a small set (many ties), labels in [0, K - 1) (class K - 1 is the abstain class: no clip carries it), the
    prototypes class-major; the second batch of CUTS below (rows 1 .. 7) holds no clip of class 1."""
    rng = np.random.default_rng(seed)
    dist = torch.from_numpy(rng.integers(0, levels, (N, P)).astype(np.float32) / levels)
    labels = torch.from_numpy(rng.integers(0, K - 1, (N,)).astype(np.int64))
    labels[1:8] = torch.from_numpy(rng.integers(0, 2, (7,)).astype(np.int64)) * 2  # classes 0 and 2 only
    proto_class = (torch.arange(P) // (P // K)).clamp(max=K - 1).to(torch.int32)
    return dist, labels, proto_class


def _cuts(N, sizes):
    out, at = [], 0
    for s in sizes:
        if at >= N:
            break
        out.append((at, min(at + s, N)))
        at += s
    if at < N:
        out.append((at, N))
    return out


CUTS_A = (1, 7, 64, 70, 8)       # B = 1, a batch without class 1, one full ballot round, one of two rounds
CUTS_B = (33, 2, 100, 5, 1, 9)


def _sweep(dist, labels, proto_class, mask, k, cuts, payloads=(), K=None):
    """One sweep over the rows cut into batches: ``payloads`` = (name, tensor (N, [P,] ...), per_proto).  Returns the state and, with
    ``K``, the class sums / counts."""
    N, P = dist.shape
    st = global_explain.TopKState(P, k, DEV)
    pc, mk = proto_class.to(DEV), mask.to(DEV)
    csum = torch.zeros((P, K), dtype=torch.float64, device=DEV) if K else None
    ccnt = torch.zeros((K,), dtype=torch.int64, device=DEV) if K else None
    for lo, hi in cuts:
        d, lab = dist[lo:hi].to(DEV).contiguous(), labels[lo:hi].to(DEV).contiguous()
        st.update(d, lab, pc, mk, lo)
        for name, t, per_proto in payloads:
            st.gather(name, t[lo:hi].to(DEV), per_proto, lo, fill=0)
        if K:
            _lib.check(_lib.lib().pasn_proto_class_stats(d.data_ptr(), lab.data_ptr(), hi - lo, P, K, csum.data_ptr(), ccnt.data_ptr(),
                                                         _lib.current_stream()))
    torch.cuda.synchronize()
    return st, csum, ccnt


def _sorted_reference(dist, labels, proto_class, mask, k):
    """torch.sort(stable=True) over each prototype's eligible column in clip order, truncated / padded to k."""
    N, P = dist.shape
    want_d = torch.full((P, k), INF)
    want_i = torch.full((P, k), -1, dtype=torch.int64)
    for j in range(P):
        rows = torch.arange(N) if not int(mask[j]) else (labels == int(proto_class[j])).nonzero().flatten()
        v, o = torch.sort(dist[rows, j], stable=True)
        n = min(k, rows.numel())
        want_d[j, :n], want_i[j, :n] = v[:n], rows[o[:n]]
    return want_d, want_i


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("P,N", [(40, 150), (1100, 90)], ids=["P40", "P1100"])
def test_topk_rows_equal_a_stable_sort(P, N, k):
    K = 4
    dist, labels, proto_class = _problem(P, K, N, seed=P + k)
    mask = push.xproto_class_mask(P, K, True, True)  # class specific, the abstention block compares with every clip
    want_d, want_i = _sorted_reference(dist, labels, proto_class, mask, k)
    states = [_sweep(dist, labels, proto_class, mask, k, _cuts(N, sizes))[0] for sizes in (CUTS_A, CUTS_B, (N,))]
    for st in states:
        assert torch.equal(st.dist.cpu(), want_d)
        assert torch.equal(st.index.cpu(), want_i)
        assert torch.equal(torch.sort(st.slot.cpu(), dim=1).values, torch.arange(k, dtype=torch.int32).repeat(P, 1))
    if k == 64 and N == 90:
        assert bool((want_i[:, -1] < 0).any()) and bool((want_i[-1] >= 0).all())  # class rows end in padding, generic rows are full
    # not class specific: every clip is eligible for every prototype
    none = push.xproto_class_mask(P, K, False, True)
    st = _sweep(dist, labels, proto_class, none, k, _cuts(N, CUTS_A))[0]
    want_d, want_i = _sorted_reference(dist, labels, proto_class, none, k)
    assert torch.equal(st.dist.cpu(), want_d) and torch.equal(st.index.cpu(), want_i)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_payloads_follow_the_winners_bit_for_bit(k):
    P, K, N = 40, 4, 150
    dist, labels, proto_class = _problem(P, K, N, seed=77 + k)
    mask = push.xproto_class_mask(P, K, True, True)
    rng = np.random.default_rng(3)
    maps7 = torch.from_numpy(rng.standard_normal((N, P, 1, 7)).astype(np.float32))    # 28-byte rows: 4-byte words
    maps49 = torch.from_numpy(rng.standard_normal((N, P, 1, 7, 7)).astype(np.float32))  # 196-byte rows, odd element count
    maps8 = torch.from_numpy(rng.standard_normal((N, P, 2, 2, 2)).astype(np.float32))  # 32-byte rows: 16-byte words
    logits = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))         # 16-byte rows shared by all prototypes
    logits3 = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32))        # 12-byte rows
    codes = torch.from_numpy(rng.integers(0, 255, (N, 3)).astype(np.uint8))           # 3-byte rows: byte copies
    halves = torch.from_numpy(rng.standard_normal((N, P, 3)).astype(np.float32)).to(torch.bfloat16)  # 6-byte rows: 2-byte words
    payloads = [("maps7", maps7, True), ("maps49", maps49, True), ("maps8", maps8, True), ("logits", logits, False),
                ("logits3", logits3, False), ("labels", labels, False), ("codes", codes, False), ("halves", halves, True)]
    resolved = []
    for sizes in (CUTS_A, CUTS_B):
        st = _sweep(dist, labels, proto_class, mask, k, _cuts(N, sizes), payloads)[0]
        index, slot = st.index.cpu(), st.slot.cpu().long()
        valid = index >= 0
        src = index.clamp(min=0)
        ar = torch.arange(P)[:, None]
        for name, t, per_proto in payloads:
            store = st.stores[name].cpu()
            got = store[ar, slot]                                  # store[j][slot[j][e]]
            want = t[src, ar] if per_proto else t[src]             # the payload row of top_index[j][e]
            sel = valid.view((P, k) + (1,) * (want.dim() - 2)).expand_as(want)
            assert torch.equal(_bits(got[sel]), _bits(want[sel])), name
            assert torch.equal(_bits(st.resolved(name).cpu()[sel]), _bits(want[sel])), name
        resolved.append({name: st.resolved(name).cpu() for name, _, _ in payloads})
    for name in resolved[0]:  # another batching of the same rows: the same winners carry the same payload
        assert torch.equal(_bits(resolved[0][name]), _bits(resolved[1][name])), name


def test_two_sweeps_are_bitwise_equal_and_class_sums_are_tight():
    P, K, N = 1100, 4, 333
    rng = np.random.default_rng(21)
    dist = torch.from_numpy(rng.random((N, P)).astype(np.float32) * 2)  # similarities 1 - d of both signs
    labels = torch.from_numpy(rng.integers(-1, K + 2, (N,)).astype(np.int64))  # labels outside [0, K) are skipped by the sums
    proto_class = (torch.arange(P) // (P // K)).clamp(max=K - 1).to(torch.int32)
    mask = push.xproto_class_mask(P, K, True, True)
    maps = torch.from_numpy(rng.standard_normal((N, P, 1, 5)).astype(np.float32))
    payloads = [("maps", maps, True), ("labels", labels, False)]
    cuts = _cuts(N, (64, 1, 130, 17, 100))
    a, a_sum, a_cnt = _sweep(dist, labels, proto_class, mask, 10, cuts, payloads, K=K)
    b, b_sum, b_cnt = _sweep(dist, labels, proto_class, mask, 10, cuts, payloads, K=K)
    for x, y in ((a.dist, b.dist), (a.index, b.index), (a.slot, b.slot), (a.stores["maps"], b.stores["maps"]),
                 (a.stores["labels"], b.stores["labels"]), (a_sum, b_sum), (a_cnt, b_cnt)):
        assert torch.equal(_bits(x), _bits(y))
    sim = (1 - dist.to(DEV)).double().cpu()  # the fp32 similarity, as the model returns it, summed in float64
    eps = 2.0 ** -53
    for c in range(K):
        rows = labels == c
        want = sim[rows].sum(0)
        bound = N * eps * sim[rows].abs().sum(0)  # the bound of a reordered fp64 sum of these addends
        err = (a_sum[:, c].cpu() - want).abs()
        print(f"class {c}: {int(rows.sum())} rows, max |sum error| {float(err.max()):.3g}, smallest bound {float(bound.min()):.3g}")
        assert bool((err <= bound).all()), f"class {c}: {float((err - bound).max()):.3g} over the bound"
        assert int(a_cnt[c]) == int(rows.sum())
    assert int(a_cnt.sum()) == int(((labels >= 0) & (labels < K)).sum())


# ------------------------------------------------------------------------------------------------- through the models
class _Loader:
    def __init__(self, batches, batch_size):
        self.batches, self.batch_size = batches, batch_size

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _clip_loader(shape, labels, sizes, seed0):
    """In-memory loader, one seed per clip, an uneven last batch; also the flat dataset ``[{"cine": clip}]``."""
    clips = [synth.echo_clips((1,) + tuple(shape), seed=seed0 + n)[0] for n in range(len(labels))]
    batches, at = [], 0
    for bi, s in enumerate(sizes):
        batches.append({"cine": torch.stack(clips[at:at + s]), "target_AS": torch.tensor(labels[at:at + s], dtype=torch.int64),
                        "filename": [f"clip{at + a}" for a in range(s)]})
        at += s
    assert at == len(labels)
    return _Loader(batches, sizes[0]), [{"cine": c} for c in clips]


MODELS = [(CFG_VIDEO_X3D, (3, 4, 64, 64), [0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1], (4, 4, 3)),
          (CFG_XPROTO, (3, 224, 224), [0, 1, 2, 2, 1, 0, 1, 2, 0, 2], (3, 3, 3, 1))]


@pytest.mark.parametrize("cfg,shape,labels,sizes", MODELS, ids=["video_x3d_s", "xprotonet_resnet18"])
def test_nearest_clips_vs_sorted_push_forward(cfg, shape, labels, sizes):
    m = synth_model(cfg).to(DEV).eval()
    loader, dataset = _clip_loader(shape, labels, sizes, seed0=400)
    P, K, k = m.num_prototypes, m.num_classes, 4
    pd, occ, logits = [], [], []
    with torch.no_grad():
        for s in loader:
            _, d, o, lg = m.push_forward(s["cine"].to(DEV))
            pd.append(d.cpu()), occ.append(o.cpu()), logits.append(lg.cpu())
    pd, occ, logits = torch.cat(pd), torch.cat(occ), torch.cat(logits)
    lab = torch.tensor(labels)
    proto_class = push._proto_classes(m)
    ar = torch.arange(P)[:, None]
    for class_specific in (False, True):
        r = global_explain.nearest_clips(loader, m, k=k, class_specific=class_specific, keep_sim_scores=True, log=lambda *_: None)
        torch.cuda.synchronize()
        mask = push.xproto_class_mask(P, K, class_specific, True)
        want_d, want_i = _sorted_reference(pd, lab, proto_class, mask, k)
        assert torch.equal(r.dist.cpu(), want_d) and torch.equal(r.index.cpu(), want_i)
        valid, src = want_i >= 0, want_i.clamp(min=0)
        assert torch.equal(r.similarity.cpu()[valid], (1 - want_d)[valid])
        assert torch.equal(r.labels.cpu(), torch.where(valid, lab[src], torch.full_like(src, -1)))
        assert torch.equal(r.logits.cpu()[valid], logits[src][valid])
        assert tuple(r.occurrence_maps.shape) == (P, k) + tuple(occ.shape[2:])
        assert torch.equal(r.occurrence_maps.cpu()[valid], occ[src, ar][valid])
        assert r.filenames == [[f"clip{int(g)}" if g >= 0 else None for g in row] for row in want_i]
        assert torch.equal(r.sim_scores.cpu(), 1 - pd) and torch.equal(r.targets.cpu(), lab)
        mean, purity, margin, ranking = global_explain.ranking_stats(
            torch.stack([(1 - pd)[lab == c].double().sum(0) for c in range(K)], dim=1), torch.bincount(lab, minlength=K), proto_class,
            r.labels.cpu(), want_i, K - 1)
        assert torch.allclose(r.class_mean_similarity.cpu(), mean, rtol=1e-12, atol=0)
        assert torch.equal(r.class_count.cpu(), torch.bincount(lab, minlength=K))
        assert torch.equal(r.purity.cpu(), purity)
        assert sorted(r.ranking.tolist()) == list(range(P)) and bool((r.margin[r.ranking][:-1] >= r.margin[r.ranking][1:]).all())
    assert not m.training

    # ---- k = 1, class specific: the push's distances exactly; its indices wherever the column's minimum is unique
    r1 = global_explain.nearest_clips(loader, m, k=1, class_specific=True, log=lambda *_: None)
    pushed = push.push_prototypes(loader, m, class_specific=True, abstain_class=True, replace_prototypes=False, log=lambda *_: None)
    torch.cuda.synchronize()
    assert torch.equal(r1.dist[:, 0], pushed["proto_dist"])
    mask = push.xproto_class_mask(P, K, True, True)
    unique = torch.zeros(P, dtype=torch.bool)
    for j in range(P):
        col = pd[:, j] if not int(mask[j]) else pd[lab == int(proto_class[j]), j]
        unique[j] = col.numel() == 0 or int((col == col.min()).sum()) == 1
    tied = int((~unique).sum())
    print(f"prototypes with a tied minimum: {tied} of {P}")
    assert tied <= 0.05 * P, f"{tied} of {P} prototypes have a tied minimum: the clips are not distinct enough for this comparison"
    assert torch.equal(r1.index[:, 0].cpu()[unique], pushed["proto_index"].cpu()[unique])
    # where the minimum IS tied the rules differ by design: the lower index here, the later clip in the push
    assert bool((r1.index[:, 0].cpu()[~unique] <= pushed["proto_index"].cpu()[~unique]).all())

    # ---- nearest_maps == model.explain maps of the same clip (in its loader batch) and prototype
    r = global_explain.nearest_clips(loader, m, k=3, log=lambda *_: None)
    lut = np.random.default_rng(1).random((256, 3)).astype(np.float32)
    protos = [0, P // 2, P - 1]
    maps_all, ov_all = [], []
    for s in loader:
        e = m.explain(s["cine"].to(DEV), maps="float", lut=lut)
        maps_all.append(e.maps.cpu()), ov_all.append(e.overlays.cpu())
    maps_all, ov_all = torch.cat(maps_all), torch.cat(ov_all)  # (N, P, [To,] Ho, Wo[, 3])
    got = global_explain.nearest_maps(r, dataset=dataset, maps="float", lut=lut, prototypes=protos)
    clips = torch.stack([torch.stack([dataset[int(g)]["cine"] for g in r.index[j].cpu()]) for j in protos])
    got2 = global_explain.nearest_maps(r, clips=clips, maps="float", prototypes=protos)
    torch.cuda.synchronize()
    assert got["prototypes"].tolist() == protos and got2["overlays"] is None
    for row, j in enumerate(protos):
        idx = r.index[j].cpu()
        assert bool((idx >= 0).all())
        assert torch.equal(got["maps"][row].cpu(), maps_all[idx, j])
        assert torch.equal(got2["maps"][row].cpu(), maps_all[idx, j])
        assert torch.equal(got["overlays"][row].cpu(), ov_all[idx, j])


def _snapshot(trainer):
    m = trainer.model
    state = {f"p.{n}": p.detach().clone() for n, p in m.named_parameters()}
    state.update({f"b.{n}": b.detach().clone() for n, b in m.named_buffers()})
    for gi, group in enumerate(trainer.optimizer.param_groups):
        for pi, p in enumerate(group["params"]):
            for key, v in trainer.optimizer.state.get(p, {}).items():
                state[f"o.{gi}.{pi}.{key}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    return state


@pytest.mark.timeout(900)
def test_trainer_sim_scores_and_explain_global(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    tc = dict(TRAIN_CFG, accumulation_steps=1, save=False)
    cfg = {"abstain_class": False, "save_dir": str(tmp_path), "train": tc, "data": {"augmentation": False, "normalize": True}}
    train, _ = _clip_loader((3, 4, 64, 64), [0, 1, 1, 0], (2, 2), seed0=900)
    val, _ = _clip_loader((3, 4, 64, 64), [0, 1, 1, 0, 1, 0, 0], (3, 3, 1), seed0=950)
    g = torch.Generator().manual_seed(5)
    grey = _Loader([{"cine": torch.randint(0, 256, (b, 1, 4, 64, 64), generator=g, dtype=torch.uint8),
                     "target_AS": torch.arange(b) % 2, "filename": [f"g{b}_{a}" for a in range(b)]} for b in (3, 2)], 3)
    t = DPTrainer(m, cfg, {"train": train, "val": val, "test": grey}, log=lambda *_: None)
    t.run_epoch(0, "train")  # the optimizer has state, the norm layers moved
    t.current_epoch = 5
    m.train()
    before = _snapshot(t)
    assert any(k.startswith("o.") for k in before)

    for mode, loader in (("val", val), ("test", grey)):
        assert t.get_sim_scores(mode) is None
        assert m.training  # left in the mode it was in
        d = tmp_path / "ranking_prototypes"
        assert {f"sim_scores_{mode}_epoch5.pth", f"targets_{mode}.pth"} <= set(os.listdir(d))
        sims, targets = t.load_sim_scores(5, mode)
        n = sum(len(s["target_AS"]) for s in loader)
        assert sims.dtype == torch.float32 and sims.device.type == "cpu" and tuple(sims.shape) == (n, m.num_prototypes)
        assert targets.dtype == torch.float32 and targets.device.type == "cpu" and tuple(targets.shape) == (n,)
        m.eval()
        with torch.no_grad():
            want = torch.cat([m(t.prepare_input(s["cine"]))[1].cpu() for s in loader])
        m.train()
        assert torch.equal(sims, want)
        assert torch.equal(targets, torch.cat([s["target_AS"] for s in loader]).float())
        assert torch.equal(torch.load(d / f"sim_scores_{mode}_epoch5.pth"), sims)

    r = t.explain_global("val", k=3)
    assert m.training
    path = tmp_path / "global" / "val" / "epoch-5" / "nearest_info.pickle"
    with open(path, "rb") as handle:
        info = pickle.load(handle)
    assert sorted(info) == sorted(global_explain.GlobalExplanation.FIELDS)
    P, K = m.num_prototypes, m.num_classes
    shapes = {"dist": (P, 3), "similarity": (P, 3), "index": (P, 3), "labels": (P, 3), "logits": (P, 3, K), "filenames": (P, 3),
              "class_mean_similarity": (P, K), "class_count": (K,), "purity": (P,), "margin": (P,), "ranking": (P,), "prototype_class": (P,)}
    for key, shape in shapes.items():
        assert isinstance(info[key], np.ndarray) and info[key].shape == shape, key
    assert info["occurrence_maps"].shape[:3] == (P, 3, 1) and info["occurrence_maps"].ndim == 6
    assert np.array_equal(info["index"], r.index.cpu().numpy()) and np.array_equal(info["dist"], r.dist.cpu().numpy())
    assert info["filenames"][0, 0] == f"clip{int(r.index[0, 0])}"
    rg = t.explain_global("test", k=2)  # grey batches go through prepare_input
    assert tuple(rg.index.shape) == (P, 2) and bool((rg.index >= 0).all())

    after = _snapshot(t)
    assert sorted(after) == sorted(before)
    for key, v in before.items():
        assert torch.equal(_bits(v), _bits(after[key])), f"{key} changed"
