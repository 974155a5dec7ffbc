"""CPU: the host side of the library optimizer (protoasnet_amd/optim.py): bindings, the block tables, FlatAdam's refusals and its
checkpoint format, the trainer option.  The kernels run in tests/test_gpu_optim.py."""
import os
import re

import numpy as np
import pytest
import torch

import optim_cases
from conftest import REPO
from protoasnet_amd import _lib, optim
from test_cpu_trainer import TRAIN_CFG, Toy, _batches


def test_optimizer_entry_points_are_declared_bound_and_exported():
    import protoasnet_amd.build

    header = open(os.path.join(REPO, "include", "protoasnet_amd.h")).read()
    lib = _lib.lib()
    for name in ("pasn_adam_step", "pasn_grad_accumulate", "pasn_optim_chunk"):
        assert name + "(" in header
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "optim.hip" in protoasnet_amd.build.SOURCES
    assert f"#define PASN_OPTIM_MAX_GROUPS {_lib.OPTIM_MAX_GROUPS}\n" in header
    assert optim.optim_chunk() > 0 and optim.optim_chunk() % 1024 == 0  # 256 threads x whole 16-byte accesses


def test_block_tables_cover_every_element_exactly_once():
    C = optim.optim_chunk()
    sizes = [1, 3, C - 1, C, C + 1, 2 * C + 5]
    bj, bc = optim.build_block_tables(sizes, C)
    assert bj.dtype == np.int32 and bc.dtype == np.int32 and len(bj) == len(bc) == sum(-(-n // C) for n in sizes)
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for j, c in zip(bj.tolist(), bc.tolist()):
        assert 0 <= j < len(sizes) and c * C < sizes[j]  # no block without work
        seen[j][c * C: min((c + 1) * C, sizes[j])] += 1
    for n, s in zip(sizes, seen):
        assert (s == 1).all(), n
    again = optim.build_block_tables(sizes, C)
    assert np.array_equal(again[0], bj) and np.array_equal(again[1], bc)  # a pure function
    with pytest.raises(ValueError):
        optim.build_block_tables([4, 0], C)


def test_job_structs_match_the_header():
    header = open(os.path.join(REPO, "include", "protoasnet_amd.h")).read()
    for name, dt in (("pasn_adam_job", optim.ADAM_JOB), ("pasn_accum_job", optim.ACCUM_JOB)):
        body = header[header.index("typedef struct " + name):]
        body = body[body.index("{") + 1: body.index("}")]
        fields = re.findall(r"(\w+)\s*[,;]", body)
        assert fields == list(dt.names), (fields, dt.names)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "decoupled_weight_decay"])
def test_flat_adam_refuses_the_variants_no_config_selects(flag):
    with pytest.raises(ValueError, match="amsgrad=False, maximize=False, decoupled_weight_decay=False"):
        optim.FlatAdam([torch.nn.Parameter(torch.zeros(3))], **{flag: True})


def test_flat_adam_refuses_cpu_parameters_at_step():
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.FlatAdam([p], lr=1e-3)
    opt.step()  # no gradient: nothing to do, nothing to refuse
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(3))


def _two_group_params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 7, 3, 4)]


def _specs(ps):
    return [{"params": ps[:2], "lr": 1e-2, "weight_decay": 1e-3}, {"params": ps[2:], "lr": 3e-3}]


def test_float64_restatement_is_torch_adam():
    """The yardstick of the GPU parity tests against torch.optim.Adam itself, on the CPU: mixed groups, a parameter skipped on alternate
    steps, lr halved half way.  Bound: fp32 storage of p rounds once per step, half an ulp of max |p| each."""
    ps = _two_group_params(0)
    opt = torch.optim.Adam(_specs(ps))
    ref = optim_cases.AdamRef(ps, [0, 0, 1, 1], opt.param_groups)
    g = torch.Generator().manual_seed(1)
    for k in range(6):
        grads = [None if (i == 1 and k % 2) else torch.randn(p.shape, generator=g) for i, p in enumerate(ps)]
        for p, gr in zip(ps, grads):
            p.grad = gr
        if k == 3:
            for h in opt.param_groups:
                h["lr"] *= 0.5
        opt.step()
        ref.step(grads)
    for i, p in enumerate(ps):
        assert optim_cases.max_err(p, ref.p[i]) <= 6 * 0.5 * optim_cases.ulp32(float(ref.p[i].abs().max()))
        assert int(opt.state[p]["step"]) == ref.t[i]
    assert ref.t == [6, 3, 6, 6]


def test_flat_adam_state_dict_is_torch_adams():
    ps_t, ps_f = _two_group_params(0), _two_group_params(0)
    adam, flat = torch.optim.Adam(_specs(ps_t)), optim.FlatAdam(_specs(ps_f))
    fresh_t, fresh_f = adam.state_dict(), flat.state_dict()
    assert fresh_f["param_groups"] == fresh_t["param_groups"] and fresh_f["state"] == {} == fresh_t["state"]
    assert list(fresh_f["param_groups"][0]) == list(fresh_t["param_groups"][0])
    g = torch.Generator().manual_seed(1)
    for k in range(3):  # parameter 1 holds a gradient in one step of three, parameter 3 in none: no state
        for i, p in enumerate(ps_t):
            p.grad = None if (i == 3 or (i == 1 and k != 1)) else torch.randn(p.shape, generator=g)
        adam.step()
    adam.param_groups[1]["lr"] = 7e-4  # as a scheduler leaves it
    ck = adam.state_dict()
    flat.load_state_dict(ck)
    back = flat.state_dict()
    assert back["param_groups"] == ck["param_groups"]
    assert sorted(back["state"]) == sorted(ck["state"]) == [0, 1, 2]
    for i, st in ck["state"].items():
        assert list(back["state"][i]) == list(st) == ["step", "exp_avg", "exp_avg_sq"]
        assert back["state"][i]["step"].dtype == st["step"].dtype and back["state"][i]["step"].shape == st["step"].shape == ()
        assert back["state"][i]["step"].device.type == "cpu" and float(back["state"][i]["step"]) == float(st["step"]) == (1.0 if i == 1 else 3.0)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], st[k])
    again = torch.optim.Adam(_specs(_two_group_params(0)))
    again.load_state_dict(back)  # and the other way
    assert float(again.state[again.param_groups[0]["params"][1]]["step"]) == 1.0
    for sched in (torch.optim.lr_scheduler.StepLR(flat, step_size=1, gamma=0.5),
                  torch.optim.lr_scheduler.ReduceLROnPlateau(flat, mode="max", factor=0.5, patience=0)):
        assert sched.optimizer is flat


def test_loading_a_checkpoint_resets_what_it_does_not_hold():
    """A parameter without an entry in the loaded state starts over, step count included, as under torch.optim.Adam."""
    ps_t, ps_f = _two_group_params(0), _two_group_params(0)
    adam, flat = torch.optim.Adam(_specs(ps_t)), optim.FlatAdam(_specs(ps_f))
    for p in ps_t:
        p.grad = torch.ones_like(p)
    adam.step()
    adam.step()
    flat.load_state_dict(adam.state_dict())
    assert [int(v["step"]) for v in flat.state_dict()["state"].values()] == [2, 2, 2, 2]
    fresh = torch.optim.Adam(_specs(_two_group_params(0)))
    fresh.param_groups[0]["params"][0].grad = torch.ones(5)
    fresh.step()  # state for parameter 0 only
    flat.load_state_dict(fresh.state_dict())
    sd = flat.state_dict()
    assert sorted(sd["state"]) == [0] and int(sd["state"][0]["step"]) == 1
    assert flat._loaded_steps == {ps_f[0]: 1}


def test_default_trainer_keeps_torch_adam_and_the_option_refuses_other_optimizers(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    b = _batches(1, 2)
    cfg = {"abstain_class": True, "save_dir": str(tmp_path), "train": dict(TRAIN_CFG)}
    t = DPTrainer(Toy(), cfg, {"train": b, "val": b}, log=lambda *_: None)
    assert type(t.optimizer) is torch.optim.Adam and t.accumulator is None
    off = DPTrainer(Toy(), dict(cfg, train=dict(TRAIN_CFG, fused_optimizer=False)), {"train": b, "val": b}, log=lambda *_: None)
    assert type(off.optimizer) is torch.optim.Adam and off.accumulator is None
    on = DPTrainer(Toy(), dict(cfg, train=dict(TRAIN_CFG, fused_optimizer=True)), {"train": b, "val": b}, log=lambda *_: None)
    assert type(on.optimizer) is optim.FlatAdam and isinstance(on.accumulator, optim.GradAccumulator)
    assert [{k: v for k, v in g.items() if k != "params"} for g in on.optimizer.param_groups] == \
           [{k: v for k, v in g.items() if k != "params"} for g in t.optimizer.param_groups]
    assert [id(p) for p in on.accumulator.params] == [id(p) for p in on.params]
    sgd = dict(TRAIN_CFG, fused_optimizer=True, optimizer={"name": "SGD", "mode": "lr_same", "lr_same": 1e-3})
    with pytest.raises(ValueError, match="fused_optimizer"):
        DPTrainer(Toy(), dict(cfg, train=sgd), {"train": b, "val": b}, log=lambda *_: None)
