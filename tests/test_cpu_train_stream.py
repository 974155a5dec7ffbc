"""CPU: the training tape's call stream is frozen.  Every case of tests/golden/make_train_stream_snapshot.py::TRAIN_CASES compiles a
``TrainRunner`` on the CPU (no activation is allocated), replays its ops against the recording stand-in of the library and compares
with tests/golden/train_call_stream_digests.json: per op its name / stream kind / join / touched bytes, the entry point, every scalar,
every descriptor field, the buffer dataflow (gradient slots as offsets into the flat gradient buffer), live parameters by name and kept
operands by their bytes; per case the arena plan, the gradient slots and the native packer's job rows.  The file holds one SHA-256 per
case over all of that (the exact comparison) and one character per op and field to name the first op and field that moved."""
import json
import os
import sys

import pytest

from conftest import GOLDEN
from protoasnet_amd import _lib

sys.path.insert(0, GOLDEN)
import make_train_stream_snapshot as snap  # noqa: E402


def _first(got: str, want: str) -> int:
    return next((j for j in range(max(len(got), len(want))) if got[j: j + 1] != want[j: j + 1]), -1)


@pytest.mark.parametrize("case", snap.TRAIN_CASES, ids=[c[0] for c in snap.TRAIN_CASES])
def test_training_call_stream_is_the_committed_one(case, monkeypatch):
    """A refactor of train.py / plan.py must leave this stream as it is: the order of buffer creation decides arena offsets, the order
    of side launches and joins decides live ranges, and a wrong one otherwise shows only as a numeric failure on the GPU.  Regenerate
    the file when a change of the training launch list is intended (and say so in the commit)."""
    for k in [k for k in os.environ if k.startswith("PASN_")]:
        monkeypatch.delenv(k)
    _lib.tuning_reload()
    golden = json.load(open(os.path.join(GOLDEN, "train_call_stream_digests.json")))
    fields, want = golden["fields"], golden["cases"][case[0]]
    assert fields == list(snap.TRAIN_FIELDS)
    got = snap.train_call_stream(case)
    print(f"{case[0]}: {got['n_ops']} ops, plan {got['plan']}")
    nf = len(fields)
    for i in range(min(got["n_ops"], want["n_ops"])):
        g, w = got["ops"][nf * i: nf * (i + 1)], want["ops"][nf * i: nf * (i + 1)]
        if g != w:
            diff = [f for j, f in enumerate(fields) if g[j] != w[j]]
            pytest.fail(f"op {i} ({got['plan']['n_fwd']} forward ops): first differing field {diff[0]!r} (all differing: {diff})")
    assert got["n_ops"] == want["n_ops"], f"{got['n_ops']} ops, recorded {want['n_ops']}"
    for key, w in want["plan"].items():
        g = got["plan"][key]
        if g != w and isinstance(w, str):
            pytest.fail(f"plan[{key!r}]: first differing {'block of 16 buffers' if key == 'offsets' else 'row'} {_first(g, w)}")
        assert g == w, f"plan[{key!r}] = {g}, recorded {w}"
    assert set(got["plan"]) == set(want["plan"])
    # the marks above only locate a difference; the comparison itself is exact
    assert got["sha"] == want["sha"], "the stream differs from the recorded one in a field whose one-character mark happens to agree"


def test_every_switch_case_differs_from_its_default():
    """The switch cases are not vacuous: each recorded stream differs from the default stream of the same model and shape."""
    cases = json.load(open(os.path.join(GOLDEN, "train_call_stream_digests.json")))["cases"]
    assert set(cases) == {c[0] for c in snap.TRAIN_CASES}
    for sw, base in snap.SWITCH_BASE.items():
        assert cases[sw]["sha"] != cases[base]["sha"], sw
