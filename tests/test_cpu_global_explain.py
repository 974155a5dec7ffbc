"""CPU: the host side of the global explanations (protoasnet_amd.global_explain): the C-ABI surface and its argument checks, the pure
merge of shards, the ranking statistics, and the reference's ``ranking_prototypes`` file names."""
import os
import re

import pytest
import torch

from protoasnet_amd import _lib, global_explain, model_builder
from protoasnet_amd.trainer import DPTrainer
from util import CFG_PPNET

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pasn_topk_xproto_update", "pasn_topk_gather", "pasn_proto_class_stats")
INF = float("inf")


def test_symbols_declared_bound_and_exported():
    text = open(os.path.join(REPO, "include", "protoasnet_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the header cites the reference lines the entry points stand in for, and leaves NaN distances unspecified
    assert "XProtoNet_Base.py:613-656" in text and "push_abs_revision.py:288-307" in text
    assert re.search(r"NaN distances give an unspecified", text)
    assert "global_explain.hip" in open(os.path.join(REPO, "protoasnet_amd", "build.py")).read()


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def update(k=10, P=40, B=4, state=(fake, fake, fake), base=0):
        return lib.pasn_topk_xproto_update(fake, fake, fake, fake, state[0], state[1], state[2], B, P, k, base, 0)

    for kw, what in ((dict(k=0), "k must lie"), (dict(k=65), "k must lie"), (dict(k=-3), "k must lie"), (dict(P=4097), "P must lie"),
                     (dict(P=0), "P must lie"), (dict(B=0), "empty batch"), (dict(base=-1), "negative index base"),
                     (dict(state=(0, fake, fake)), "null state"), (dict(state=(fake, 0, fake)), "null state"),
                     (dict(state=(fake, fake, 0)), "null state")):
        with pytest.raises(ValueError, match=what):
            _lib.check(update(**kw))
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(lib.pasn_topk_xproto_update(0, fake, fake, fake, fake, fake, fake, 4, 40, 10, 0, 0))

    def gather(k=10, P=40, B=4, row=49, eb=4, state=(fake, fake), payload=fake, store=fake):
        return lib.pasn_topk_gather(state[0], state[1], payload, store, B, P, k, row, eb, 1, 0, 0)

    for kw, what in ((dict(k=65), "k must lie"), (dict(k=0), "k must lie"), (dict(P=5000), "P must lie"), (dict(row=0), "empty payload row"),
                     (dict(eb=3), "elem_bytes"), (dict(eb=16), "elem_bytes"), (dict(state=(0, fake)), "null state"),
                     (dict(store=0), "null pointer"), (dict(payload=258, eb=4), "not aligned")):
        with pytest.raises(ValueError, match=what):
            _lib.check(gather(**kw))
    for args, what in (((fake, fake, 4, 40, 0, fake, fake, 0), "K must lie"), ((fake, fake, 4, 40, 65, fake, fake, 0), "K must lie"),
                       ((fake, fake, 4, 4097, 4, fake, fake, 0), "P must lie"), ((fake, fake, 4, 40, 4, 0, fake, 0), "null state"),
                       ((fake, fake, 0, 40, 4, fake, fake, 0), "empty batch")):
        with pytest.raises(ValueError, match=what):
            _lib.check(lib.pasn_proto_class_stats(*args))
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        global_explain.TopKState(4, 65, "cpu")
    with pytest.raises(ValueError):
        global_explain.TopKState(4, 0, "cpu")


def test_ppnet_is_refused():
    m = model_builder.build(CFG_PPNET).eval()
    with pytest.raises(NotImplementedError, match="PPNet"):
        global_explain.nearest_clips([], m)


# ------------------------------------------------------------------------------------------------- merge_topk
def _reference_merge(shards, k):
    """A stable sort of the union, per prototype, in plain Python: valid entries by (distance, index), then padding."""
    P = shards[0][0].shape[0]
    dist, index, pay = [], [], []
    for j in range(P):
        union = []
        for d, i, p in shards:
            union += [(float(d[j, e]), int(i[j, e]), p[j, e].clone()) for e in range(d.shape[1]) if int(i[j, e]) >= 0]
        union = sorted(union, key=lambda t: (t[0], t[1]))[:k]
        pad = k - len(union)
        dist.append([u[0] for u in union] + [INF] * pad)
        index.append([u[1] for u in union] + [-1] * pad)
        pay.append(torch.stack([u[2] for u in union] + [torch.zeros_like(shards[0][2][0, 0])] * pad))
    return torch.tensor(dist, dtype=torch.float32), torch.tensor(index, dtype=torch.int64), torch.stack(pay)


def _shard(rows, k, width=3):
    """rows: per prototype a list of (dist, index) in row order; padded to k.  The payload row of clip g is g + [0, 0.25, 0.5]."""
    P = len(rows)
    d = torch.full((P, k), INF)
    i = torch.full((P, k), -1, dtype=torch.int64)
    p = torch.zeros((P, k, width))
    for j, row in enumerate(rows):
        for e, (dv, iv) in enumerate(row):
            d[j, e], i[j, e] = dv, iv
            p[j, e] = iv + torch.arange(width) * 0.25
    return d, i, p


def test_merge_topk_equals_a_stable_sort_of_the_union():
    k = 3
    a = _shard([[(0.1, 2), (0.5, 0), (0.5, 1)], [(0.2, 0), (0.2, 1), (0.2, 2)], [], [(0.3, 1)]], k)
    b = _shard([[(0.1, 5), (0.5, 3), (0.7, 4)], [(0.2, 3), (0.2, 4), (0.9, 5)], [(0.4, 3)], []], k)          # ties across shards
    c = _shard([[(0.05, 8), (0.1, 6), (0.5, 7)], [(0.1, 7), (0.2, 6), (0.2, 8)], [(0.4, 6), (0.4, 7)], []], k)  # a shard after an empty row
    for shards in ([a, b, c], [c, a, b], [a], [b, c]):
        got = global_explain.merge_topk(shards)
        want = _reference_merge(shards, k)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    d, i, _ = global_explain.merge_topk([a, b, c])
    assert i[1].tolist() == [7, 0, 1]          # the tie at 0.2 keeps the lower global index first
    assert i[0].tolist() == [8, 2, 5] and d[0].tolist() == pytest.approx([0.05, 0.1, 0.1])
    assert i[3].tolist() == [1, -1, -1] and d[3, 1:].tolist() == [INF, INF]


def test_merge_topk_k_larger_than_the_union_and_integer_payloads():
    narrow_a = _shard([[(0.3, 0)], [(0.6, 1)]], 1)
    narrow_b = _shard([[(0.2, 2)], [(0.6, 3)]], 1)
    wide = _shard([[], []], 5)  # the first shard sets k = 5; the union holds two clips per row
    d, i, p = global_explain.merge_topk([wide, narrow_a, narrow_b])
    assert i.tolist() == [[2, 0, -1, -1, -1], [1, 3, -1, -1, -1]]
    assert d[:, 2:].eq(INF).all() and p[:, 2:].eq(0).all()
    assert torch.equal(p[0, 0], torch.tensor([2.0, 2.25, 2.5]))
    lab = torch.tensor([[4], [5]])
    d, i, labels = global_explain.merge_topk([(narrow_a[0], narrow_a[1], lab), (torch.full((2, 1), INF), torch.full((2, 1), -1), lab * 0)])
    assert labels.tolist() == [[4], [5]]
    d, i, labels = global_explain.merge_topk([(torch.full((2, 2), INF), torch.full((2, 2), -1), torch.zeros((2, 2), dtype=torch.int64)),
                                              (narrow_a[0], narrow_a[1], lab)])
    assert labels.tolist() == [[4, -1], [5, -1]]  # empty entries of an integer payload read -1
    # a (+inf) distance of a real clip sorts before the empty entries
    d, i, _ = global_explain.merge_topk([_shard([[(INF, 9)]], 2), _shard([[(0.5, 10)]], 2)])
    assert i.tolist() == [[10, 9]]


# ------------------------------------------------------------------------------------------------- ranking statistics
def test_purity_margin_ranking_from_hand_made_sums():
    # K = 4 (three real classes + abstain), P = 5: prototypes of classes 0, 1, 1, 2 and one abstention prototype; class 2 has NO clip
    count = torch.tensor([4, 2, 0, 0])
    sums = torch.tensor([[3.2, 0.4, 0.0, 0.0],    # mean .8 / .2        -> margin  .6
                         [1.2, 1.6, 0.0, 0.0],    # mean .3 / .8        -> margin  .5
                         [2.0, 1.0, 0.0, 0.0],    # mean .5 / .5        -> margin  0
                         [2.0, 1.8, 0.0, 0.0],    # own class 2 empty   -> margin  0 - .9
                         [0.4, 1.2, 0.0, 0.0]],   # abstention prototype -> margin 0 - .6
                        dtype=torch.float64)
    pc = torch.tensor([0, 1, 1, 2, 3])
    labels = torch.tensor([[0, 0, 1], [1, 0, -1], [0, 0, 0], [-1, -1, -1], [1, 1, 0]])
    index = torch.tensor([[3, 1, 4], [5, 0, -1], [0, 1, 2], [-1, -1, -1], [4, 5, 2]])
    mean, purity, margin, ranking = global_explain.ranking_stats(sums, count, pc, labels, index, num_real_classes=3)
    assert torch.isfinite(mean).all() and torch.isfinite(margin).all() and torch.isfinite(purity).all()
    assert mean[:, 2:].eq(0).all()  # a class without clips: mean 0, no division by zero
    assert mean[:, :2].flatten().tolist() == pytest.approx([.8, .2, .3, .8, .5, .5, .5, .9, .1, .6])
    assert purity.tolist() == pytest.approx([2 / 3, 1 / 2, 0.0, 0.0, 0.0])
    assert margin.tolist() == pytest.approx([0.6, 0.5, 0.0, -0.9, -0.6])
    assert ranking.tolist() == [0, 1, 2, 4, 3]
    # equal margins: the lower index first; one class only: nothing to subtract
    mean, _, margin, ranking = global_explain.ranking_stats(torch.ones((3, 2), dtype=torch.float64), torch.tensor([2, 0]),
                                                            torch.tensor([0, 0, 1]), torch.zeros((3, 1), dtype=torch.int64),
                                                            torch.zeros((3, 1), dtype=torch.int64), num_real_classes=2)
    assert margin.tolist() == [0.5, 0.5, -0.5] and ranking.tolist() == [0, 1, 2]


def test_filenames_follow_the_global_index():
    names = {0: ["a0", "a1", "a2"], 3: ["b0"], 4: ["c0", "c1"]}
    index = torch.tensor([[4, 0, 3], [5, 2, -1]])
    assert global_explain._filenames(names, index) == [["c0", "a0", "b0"], ["c1", "a2", None]]


def _filenames_by_base_scan(names, index):
    """The push's former spelling: per index the largest batch base at or below it."""
    bases = sorted(names)
    files = []
    for g in index.tolist():
        base = max([b for b in bases if b <= g], default=None) if g >= 0 else None
        files.append(names[base][g - base] if base is not None and g - base < len(names[base]) else None)
    return files


def _filenames_by_searchsorted(names, index):
    """The global explanation's former spelling, row by row."""
    import numpy as np

    bases = np.array(sorted(names), dtype=np.int64)
    out = []
    for row in index.numpy().astype(np.int64):
        files = []
        for g in row:
            at = int(np.searchsorted(bases, g, side="right")) - 1 if g >= 0 and bases.size else -1
            batch = names[int(bases[at])] if at >= 0 else []
            off = int(g - bases[at]) if at >= 0 else 0
            files.append(batch[off] if at >= 0 and off < len(batch) else None)
        out.append(files)
    return out


def test_filenames_at_equals_both_former_spellings():
    from protoasnet_amd.sweep import filenames_at

    assert global_explain._filenames is filenames_at
    hand = {0: ["a0", "a1", "a2"], 3: ["b0"], 4: ["c0", "c1"]}
    cases = [(hand, torch.tensor([[4, 0, 3], [5, 2, -1]])),
             # the push's cases: never won, an index equal to a base, an index past the last batch's names, "" defaults, no names at all
             ({0: ["", ""], 2: ["x", "y"], 4: ["z"]}, torch.tensor([[-1, 0, 2, 4], [5, 9, 3, 1]])),
             ({}, torch.tensor([[-1, 0, 7]]))]
    for names, index in cases:
        want = _filenames_by_searchsorted(names, index)
        assert filenames_at(names, index) == want
        assert [_filenames_by_base_scan(names, row) for row in index] == want
        assert filenames_at(names, index.flatten()) == [f for row in want for f in row]  # the push's (P,) index: a flat list
    assert filenames_at(hand, torch.tensor([[4, 0, 3], [5, 2, -1]])) == [["c0", "a0", "b0"], ["c1", "a2", None]]
    assert filenames_at({0: ["", ""], 2: ["x", "y"], 4: ["z"]}, torch.tensor([-1, 2, 5, 4])) == [None, "x", None, "z"]
    assert filenames_at({}, torch.tensor([-1, 0])) == [None, None]


# ------------------------------------------------------------------------------------------------- the reference's file names
class _Agent:
    """The two methods under test need ``config`` only."""

    _sim_scores_paths = DPTrainer._sim_scores_paths
    load_sim_scores = DPTrainer.load_sim_scores

    def __init__(self, save_dir):
        self.config = {"save_dir": save_dir}


def test_ranking_prototypes_file_names(tmp_path):
    agent = _Agent(str(tmp_path))
    sim_path, target_path = agent._sim_scores_paths(7, "val")
    assert sim_path == os.path.join(str(tmp_path), "ranking_prototypes", "sim_scores_val_epoch7.pth")   # XProtoNet_Base.py:642-649
    assert target_path == os.path.join(str(tmp_path), "ranking_prototypes", "targets_val.pth")           # XProtoNet_Base.py:650-653
    os.makedirs(os.path.dirname(sim_path))
    sims, targets = torch.rand(5, 3), torch.tensor([0.0, 1.0, 2.0, 1.0, 0.0])
    torch.save(sims, sim_path)
    torch.save(targets, target_path)
    got_s, got_t = agent.load_sim_scores(7, "val")
    assert torch.equal(got_s, sims) and torch.equal(got_t, targets)
    for name in ("get_sim_scores", "load_sim_scores", "explain_global"):
        assert callable(getattr(DPTrainer, name))
