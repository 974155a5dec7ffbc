"""CPU, world_size 2, gloo: the sharded push path (contiguous batch shards -> all_gather -> deterministic merge) gives
every rank exactly the winners of a single-process sweep.  The per-batch device kernel is replaced by the restated
reference loop here (no GPU in this container); the kernel itself is checked index-exact on the GPU box."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _make_batches():
    rng = np.random.default_rng(3)
    P, D, B, nb, K = 12, 5, 4, 7, 3
    ident = oracle.heads.prototype_class_identity(P, K).numpy()
    batches = [(rng.standard_normal((B, P, D)).astype(np.float32), (np.round(rng.random((B, P)) * 4) / 4).astype(np.float32),
                rng.integers(0, K, B)) for _ in range(nb)]
    return P, D, B, nb, K, ident, batches


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from protoasnet_amd.push import PushState, _all_gather_states, merge_ppnet, merge_xproto, shard_batches

    P, D, B, nb, K, ident, batches = _make_batches()
    mine = shard_batches(nb, rank, world)
    d, f, w = oracle.push.xproto_push_select([batches[i] for i in mine], ident, K, True, False)
    st = PushState(P, D, "cpu")
    st.dist.copy_(torch.from_numpy(d).float())
    st.index.copy_(torch.tensor([-1 if x is None else (mine.start + x[0]) * B + x[1] for x in w]))
    st.vec.copy_(torch.stack([torch.zeros(D) if v is None else torch.from_numpy(v) for v in f]))
    md, mi, mv = _all_gather_states(st, merge_xproto)
    # PPNet-rule state through the same exchange (2-column index)
    sp = PushState(2, 2, "cpu", ppnet=True)
    sp.dist.copy_(torch.tensor([0.5, 0.25]))
    sp.index.copy_(torch.tensor([[4, 1], [9, 0]]) if rank == 0 else torch.tensor([[2, 7], [9, 3]]))
    sp.vec.fill_(float(rank))
    pd, pi, pv = _all_gather_states(sp, merge_ppnet)
    # the winners' records (occurrence maps, clips, ...) of a sharded push: each prototype's record comes from the rank that owns its
    # final winner, one sum-reduce to rank 0; rank 1 has seen no batch that saves records for prototype 0 ...
    from protoasnet_amd.push import _reduce_records

    local = torch.tensor([3, -1, 7]) if rank == 0 else torch.tensor([12, 11, 9])
    merged_idx = torch.tensor([3, 11, 9])  # prototype 0 won by rank 0, prototypes 1 and 2 by rank 1
    rec = [torch.full((3, 2, 2), float(rank + 1)), torch.tensor([10, 20, 30]) * (rank + 1)]
    rr, names = _reduce_records(rec, {0: ["a", "b"]} if rank == 0 else {8: ["c"]}, local, merged_idx, "cpu")
    torch.save({"dist": md, "index": mi, "vec": mv, "pindex": pi, "pvec": pv, "rec0": rr[0], "rec1": rr[1], "names": names},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_push_merge_world2(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    P, D, B, nb, K, ident, batches = _make_batches()
    full_d, full_f, full_w = oracle.push.xproto_push_select(batches, ident, K, True, False)
    want_idx = [w[0] * B + w[1] for w in full_w]
    outs = [torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(world)]
    for o in outs:  # every rank ends with the same, correct winners -- no broadcast needed afterwards
        assert o["index"].tolist() == want_idx
        assert torch.equal(o["vec"], torch.stack([torch.from_numpy(v) for v in full_f]))
        assert np.array_equal(o["dist"].numpy(), full_d.astype(np.float32))
        assert o["pindex"].tolist() == [[2, 7], [9, 0]] and o["pvec"].tolist() == [[1.0, 1.0], [0.0, 0.0]]
        assert o["names"] == {0: ["a", "b"], 8: ["c"]}
    assert outs[0]["rec0"][:, 0, 0].tolist() == [1.0, 2.0, 2.0] and outs[0]["rec1"].tolist() == [10, 40, 60]  # on rank 0, the writer


def test_sharded_push_without_a_process_group_is_refused():
    """world_size > 1 with no initialised group used to push from the local shard only, silently."""
    from protoasnet_amd.push import _require_group

    with pytest.raises(RuntimeError, match="torch.distributed"):
        _require_group(2)
    _require_group(1)


def test_saving_push_names_its_prototype_limit_before_the_sweep(tmp_path):
    """The winners' records follow them through pasn_topk_gather (P <= 4096): a saving push with more prototypes says so before it
    touches the loader, for both model kinds."""
    from protoasnet_amd import push

    class Model(torch.nn.Module):
        num_prototypes, num_classes, prototype_shape = 4100, 4, (4100, 8, 1, 1)
        prototype_class_identity = torch.zeros(4100, 4)

        def __init__(self):
            super().__init__()
            self.prototype_vectors = torch.nn.Parameter(torch.zeros(self.prototype_shape))

    class Untouched:
        batch_size = 4

        def __len__(self):
            return 3

        def __iter__(self):
            raise AssertionError("the sweep started")

    for fn in (push.push_prototypes, push.push_prototypes_ppnet):
        with pytest.raises(ValueError, match="at most 4096 prototypes"):
            fn(Untouched(), Model(), root_dir_for_saving_prototypes=str(tmp_path), log=lambda *_: None)


def test_shard_iteration_offsets_come_from_the_sampler_not_the_rank():
    """A torch DataLoader is re-instantiated over the rank's slice of its batch_sampler: foreign batches are never loaded and the
    global clip offsets are the sampler's prefix sums (ragged batches included), identical on every rank."""
    from protoasnet_amd.push import _iter_shard

    loaded = []

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 11

        def __getitem__(self, i):
            loaded.append(i)
            return {"cine": torch.full((1,), float(i)), "target_AS": torch.tensor(i % 3), "filename": str(i)}

    sampler = [[0, 1, 2], [3, 4], [5, 6, 7, 8], [9], [10]]  # ragged on purpose
    dl = torch.utils.data.DataLoader(DS(), batch_sampler=sampler)
    got = {r: [(i, base, s["cine"].flatten().tolist()) for i, base, s in _iter_shard(dl, r, 2)] for r in range(2)}
    assert [g[:2] for g in got[0]] == [(0, 0), (1, 3), (2, 5)] and [g[:2] for g in got[1]] == [(3, 9), (4, 10)]
    assert got[1][0][2] == [9.0]
    loaded.clear()
    list(_iter_shard(dl, 1, 2))
    assert sorted(loaded) == [9, 10]  # rank 1 loaded only its own clips


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from protoasnet_amd.dp import allreduce_gradients

    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in ((7, 3, 1, 1, 1), (5,), (2, 9), (4,))]
    g = torch.Generator().manual_seed(100 + rank)
    for i, p in enumerate(params):
        if i != 3:  # a parameter without a gradient (frozen / unused) is skipped on every rank alike
            p.grad = torch.randn(p.shape, generator=g)
    nbytes = allreduce_gradients(params)
    torch.save({"grads": [None if p.grad is None else p.grad.clone() for p in params], "nbytes": nbytes}, os.path.join(out_dir, f"dp{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_gradient_bucket_allreduce_world2(tmp_path):
    """The data-parallel training exchange (one flat fp32 bucket, averaged): every rank ends with the mean of the ranks' gradients."""
    world, port = 2, _free_port()
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    shapes = ((7, 3, 1, 1, 1), (5,), (2, 9))
    want = []
    for s in shapes:
        want.append(torch.zeros(s))
    per_rank = []
    for r in range(world):
        g = torch.Generator().manual_seed(100 + r)
        per_rank.append([torch.randn(s, generator=g) for s in shapes])
    mean = [(per_rank[0][i] + per_rank[1][i]) / 2 for i in range(len(shapes))]
    for r in range(world):
        o = torch.load(os.path.join(tmp_path, f"dp{r}.pt"))
        assert o["grads"][3] is None and o["nbytes"] == sum(t.numel() for t in mean) * 4
        for got, ref in zip(o["grads"][:3], mean):
            assert torch.allclose(got, ref, atol=1e-6)


def _dp_inplace_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from protoasnet_amd import dp

    # gradients laid out the way train.TrainPlan.backward returns them: views of ONE zero-initialised flat buffer, 64-float slots
    shapes = ((7, 3, 1, 1, 1), (5,), (2, 9))
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    G = torch.zeros(64 * 3)
    g = torch.Generator().manual_seed(100 + rank)
    for i, p in enumerate(params):
        v = G[64 * i: 64 * i + p.numel()].view_as(p)
        v.copy_(torch.randn(p.shape, generator=g))
        p.grad = v
    flat = dp.flat_gradient_view([p.grad for p in params])
    assert flat is not None and flat.data_ptr() == G.data_ptr() and flat.numel() == 128 + 18
    ptrs = [p.grad.data_ptr() for p in params]
    nbytes = dp.allreduce_gradients(params)
    assert [p.grad.data_ptr() for p in params] == ptrs  # reduced where they lie
    assert float(G[21:64].abs().max()) == 0.0 and float(G[69:128].abs().max()) == 0.0  # the alignment gaps stay zero
    torch.save({"grads": [p.grad.clone() for p in params], "nbytes": nbytes}, os.path.join(out_dir, f"ip{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_gradient_allreduce_in_place_on_the_flat_training_buffer(tmp_path):
    """When every gradient is a view of one flat buffer (what the compiled backward pass produces) the exchange runs in place on that
    buffer -- no flatten / unflatten / copy back -- and gives the same means; anything else falls back to a fresh bucket."""
    from protoasnet_amd import dp

    world, port = 2, _free_port()
    mp.spawn(_dp_inplace_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    shapes = ((7, 3, 1, 1, 1), (5,), (2, 9))
    per_rank = []
    for r in range(world):
        g = torch.Generator().manual_seed(100 + r)
        per_rank.append([torch.randn(s, generator=g) for s in shapes])
    for r in range(world):
        o = torch.load(os.path.join(tmp_path, f"ip{r}.pt"))
        assert o["nbytes"] == (128 + 18) * 4
        for i, got in enumerate(o["grads"]):
            assert torch.allclose(got, (per_rank[0][i] + per_rank[1][i]) / 2, atol=1e-6)
    # not one storage / not dense / a sparse span: no in-place view
    a, b = torch.zeros(8), torch.zeros(8)
    assert dp.flat_gradient_view([a, b]) is None
    big = torch.zeros(4096)
    assert dp.flat_gradient_view([big[:8], big[4000:4008]]) is None
    assert dp.flat_gradient_view([big[:16].view(4, 4).t()]) is None
    assert dp.flat_gradient_view([big[:8], big[8:16].double()]) is None
    assert dp.flat_gradient_view([]) is None
    v = dp.flat_gradient_view([big[64:72], big[0:8]])
    assert v is not None and v.data_ptr() == big.data_ptr() and v.numel() == 72


def _run_bench(args, env_extra=None, timeout=300):
    import json
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


@pytest.mark.timeout(300)
def test_bench_gpus2_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher: the parent starts two rank processes itself and the line says n_gpus 2
    (round 1 silently ran one rank); the collective really saw both ranks.  --dry-run: no device work in this container."""
    r, line = _run_bench(["--gpus", "2", "--dry-run", "--steps", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["collective_backend"] == "gloo"
    assert line["data"] == "dry-run" and line["metric"].startswith("dry-run")  # cannot be mistaken for a measurement


@pytest.mark.timeout(120)
def test_bench_refuses_world_size_mismatch():
    r, line = _run_bench(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "4", "RANK": "0"})
    assert r.returncode != 0 and line is None and "WORLD_SIZE=4" in r.stderr


@pytest.mark.timeout(120)
def test_bench_needs_the_gpu_and_says_so():
    """No silent CPU fallback: without a GPU the real benchmark refuses to run."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r, line = _run_bench(["--steps", "1", "--warmup", "1"])
    assert r.returncode != 0 and line is None


def test_bench_dump_outputs_writes_float32_within_the_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as <name>.npy in float32; above the budget, a fixed sample of each array (same elements in every
    run) that keeps all files together within it."""
    import bench

    small = {"logits": torch.randn(4, 3, dtype=torch.bfloat16), "similarity": torch.rand(4, 30)}
    bench._dump_outputs(str(tmp_path / "small"), small)
    for name, t in small.items():
        a = np.load(tmp_path / "small" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy()), name
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    big = {"similarity": torch.rand(8, 30), "occurrence_map": torch.rand(8, 30, 1, 4, 14, 14)}
    for run in ("a", "b"):
        bench._dump_outputs(str(tmp_path / run), big)
    assert sum(os.path.getsize(tmp_path / "a" / f"{name}.npy") for name in big) <= 64 << 10
    for name, t in big.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < t.numel() and np.array_equal(a, b), name
        assert np.isin(a, t.numpy().reshape(-1)).all(), name
