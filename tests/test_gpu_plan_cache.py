"""One eviction rule for the compiled device state (plan.PlanCache): after a ``tuning_reload()`` or a parameter that moved, the trunk
plans, the head chains' packed weights, the training runners and the captured graphs of the older generation are gone -- not kept next
to the ones that replace them."""
import pytest
import torch

from protoasnet_amd import _lib, synth
from protoasnet_amd.nets import PointwiseChain
from test_gpu_train import SHAPE, _train_model
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLIP = (1, 3, 4, 64, 64)


def _chain_values(m):
    return [v for c in m.modules() if isinstance(c, PointwiseChain) for v in c._cache.values()]


def test_trunk_and_head_chains_keep_one_generation_across_a_tuning_reload():
    m = synth_model(CFG_VIDEO_X3D).to(DEV).eval()
    x = synth.echo_clips(CLIP).to(DEV)
    with torch.no_grad():
        first = [t.clone() for t in m(x)]
        old_plans, old_chain = m.cnn_backbone._plans.values(), _chain_values(m)
        assert len(old_plans) == 1 and len(old_chain) == 2  # add-on + occurrence module: one set of packed weights each
        _lib.tuning_reload()
        second = m(x)
    assert len(m.cnn_backbone._plans) == 1 and m.cnn_backbone._plans.values()[0] is not old_plans[0]
    new_chain = _chain_values(m)
    assert len(new_chain) == 2 and not any(v is o for v in new_chain for o in old_chain)
    for a, b in zip(second, first):
        assert torch.equal(a, b)


def test_training_runners_of_a_moved_parameter_or_an_older_epoch_leave():
    m = _train_model(kink_free=True)
    x = synth.echo_clips(SHAPE).to(DEV)
    x4 = synth.echo_clips((4,) + SHAPE[1:]).to(DEV)
    m(x)
    m(x4)
    assert len(m._train_runners) == 2
    p = m.add_on_layers[0].weight
    p.data = p.data.clone()  # what a load_state_dict / .to() that reallocates does: the runners hold the old address
    m(x)
    assert len(m._train_runners) == 1  # the other shape's runner can never hit again: it leaves too
    first = m._train_runners.values()[0]
    assert m(x)[0].shape[0] == SHAPE[0] and m._train_runners.values()[0] is first
    _lib.tuning_reload()
    m(x)
    assert len(m._train_runners) == 1 and m._train_runners.values()[0] is not first


def test_captured_graphs_keep_one_generation_across_a_tuning_reload():
    from protoasnet_amd.graph import GraphedForward

    m = synth_model(CFG_VIDEO_X3D).to(DEV).eval().set_compute_dtype(torch.bfloat16)
    x = synth.echo_clips(CLIP).to(DEV).bfloat16()
    with torch.no_grad():
        want = [t.clone() for t in m(x)]
    g = GraphedForward(m)
    for a, b in zip(g(x), want):
        assert torch.equal(a, b)
    assert g.captures == 1 and len(g._graphs) == 1
    _lib.tuning_reload()
    got = g(x)
    assert g.captures == 2 and len(g._graphs) == 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    g(x)
    assert g.captures == 2
