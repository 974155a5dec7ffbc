"""plan.PlanCache -- the one cache under the trunk plans, the head chains' packed weights, the training runners and the captured
graphs -- and plan.tensor_signature, without a GPU: a counter stands in for the signature, ``_lib.tuning_reload()`` moves the epoch."""
import torch

from protoasnet_amd import _lib
from protoasnet_amd.plan import PlanCache, tensor_signature


class _Maker:
    """``make`` callables that count their calls and return a fresh object per call."""

    def __init__(self):
        self.calls = []

    def __call__(self, tag):
        def make():
            self.calls.append(tag)
            return [tag, len(self.calls)]

        return make


def test_hit_and_miss_call_make_once_per_miss():
    sig, mk = [0], _Maker()
    c = PlanCache(lambda: sig[0])
    a = c.lookup("a", mk("a"))
    assert c.lookup("a", mk("a")) is a and c.lookup("a", mk("a")) is a
    b = c.lookup("b", mk("b"))
    assert b is not a and c.lookup("b", mk("b")) is b and c.lookup("a", mk("a")) is a
    assert mk.calls == ["a", "b"] and len(c) == 2


def test_signature_change_drops_every_older_entry():
    sig, mk = [0], _Maker()
    c = PlanCache(lambda: sig[0])
    old = [c.lookup(k, mk(k)) for k in ("a", "b", "c")]
    sig[0] += 1
    seen = []

    def make():  # the stale generation is gone BEFORE the new entry is built: two generations never coexist
        seen.append(len(c))
        return "new a"

    assert c.lookup("a", make) == "new a"
    assert seen == [0] and len(c) == 1 and c.values() == ["new a"]
    assert c.lookup("b", mk("b")) is not old[1] and len(c) == 2
    sig[0] -= 1  # an entry is good only under the stamp it was built with: the earlier signature coming back revives nothing
    assert c.lookup("c", mk("c")) is not old[2] and len(c) == 1
    assert mk.calls == ["a", "b", "c", "b", "c"]


def test_epoch_change_drops_every_older_entry():
    mk = _Maker()
    c = PlanCache(lambda: ())
    old = [c.lookup(k, mk(k)) for k in ("a", "b", "c")]
    _lib.tuning_reload()
    assert len(c) == 3  # nothing leaves until a lookup misses
    new = c.lookup("b", mk("b"))
    assert new is not old[1] and c.values() == [new]
    assert c.lookup("b", mk("b")) is new
    assert mk.calls == ["a", "b", "c", "b"]


def test_max_entries_evicts_least_recently_used_and_reports_each_key():
    evicted, mk = [], _Maker()
    c = PlanCache(lambda: (), max_entries=2, on_evict=evicted.append)
    a = c.lookup("a", mk("a"))
    c.lookup("b", mk("b"))
    assert c.lookup("a", mk("a")) is a  # a hit refreshes recency: "b" is now the oldest
    c.lookup("c", mk("c"))
    assert evicted == ["b"] and len(c) == 2
    assert c.lookup("a", mk("a")) is a
    c.lookup("d", mk("d"))
    assert evicted == ["b", "c"] and [v[0] for v in c.values()] == ["a", "d"]
    c.max_entries = 1
    c.lookup("e", mk("e"))  # more than one entry over the cap: each one reported, oldest first
    assert evicted == ["b", "c", "a", "d"] and [v[0] for v in c.values()] == ["e"]
    assert mk.calls == ["a", "b", "c", "d", "e"]
    quiet = PlanCache(lambda: (), max_entries=1)  # no callback: evicts silently
    quiet.lookup("a", mk("a"))
    quiet.lookup("b", mk("b"))
    assert [v[0] for v in quiet.values()] == ["b"]


def test_values_are_least_recently_used_first_and_clear_empties():
    mk = _Maker()
    c = PlanCache(lambda: ())
    assert len(c) == 0 and c.values() == []
    for k in ("a", "b", "c"):
        c.lookup(k, mk(k))
    c.lookup("a", mk("a"))
    vals = c.values()
    assert [v[0] for v in vals] == ["b", "c", "a"]
    c.clear()
    assert len(c) == 0 and c.values() == []
    assert [v[0] for v in vals] == ["b", "c", "a"]  # the list handed out is the caller's: it keeps the values alive
    c.lookup("a", mk("a"))
    assert mk.calls == ["a", "b", "c", "a"]


def test_make_that_raises_stores_nothing():
    c = PlanCache(lambda: ())

    def boom():
        raise NotImplementedError("no launch list")

    for _ in range(2):
        try:
            c.lookup("a", boom)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("the error of make() must reach the caller")
    assert len(c) == 0


def test_tensor_signature_moves_on_in_place_ops_not_on_data_writes():
    p, q = torch.nn.Parameter(torch.ones(4)), torch.zeros(3)
    s0 = tensor_signature([p, q])
    assert s0 == ((p.data_ptr(), p._version), (q.data_ptr(), q._version)) and tensor_signature([p, q]) == s0
    assert tensor_signature(iter([p, q])) == s0  # a generator such as module.parameters() will do
    with torch.no_grad():
        p.mul_(2.0)
    s1 = tensor_signature([p, q])
    assert s1 != s0 and s1[1] == s0[1]
    p.data.copy_(torch.full((4,), 7.0))  # the blind spot: a write through .data bumps no counter (callers use invalidate_plans() / clear())
    assert tensor_signature([p, q]) == s1
    p.data = p.data.clone()  # new storage: the address moves
    assert tensor_signature([p, q]) != s1
