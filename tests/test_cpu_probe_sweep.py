"""CPU: the library's geometry probes are frozen.  tests/golden/probe_sweep.json holds, per (descriptor group, probe, environment), one
digest of what the routing and sizing questions of csrc/conv.hip and csrc/wgrad.hip answer -- over every descriptor the compiled plans
and training tapes pass to the library and over a synthetic grid across the rungs of the ladders, under the default environment and
under each routing switch those ladders read (tests/golden/make_probe_sweep.py).  Runs no kernel."""
import os
import sys

import pytest

from conftest import GOLDEN
from protoasnet_amd import _lib

sys.path.insert(0, GOLDEN)
import make_probe_sweep as snap  # noqa: E402

_GOLDEN = snap.load_golden()
_GROUPS = {}


def _groups():
    if not _GROUPS:
        _GROUPS.update(snap.stored_groups(_GOLDEN))
        _GROUPS.update(snap.grid_descs())
    return _GROUPS


def test_the_file_covers_every_probe_environment_and_case():
    import make_routing_snapshot
    import make_train_stream_snapshot

    assert _GOLDEN["fields"] == [f for f, _ in _lib.ConvDesc._fields_]
    assert _GOLDEN["envs"] == [e for e, _ in snap.ENVS] and _GOLDEN["probes"] == list(snap.PROBES)
    want = ({f"plan:{c[0]}" for c in make_routing_snapshot.CASES} | {f"train:{c[0]}" for c in make_train_stream_snapshot.TRAIN_CASES}
            | set(snap.grid_descs()))
    assert set(_GOLDEN["digests"]) == want == set(_groups())
    for g, (singles, pairs) in _groups().items():
        assert singles, g
    # every environment moves at least one digest against its base (no vacuous environment).  The four of SIZING_BLIND are exempt: on this
    # grid the sizing cannot see them alone (see make_probe_sweep.py); a descriptor on which they do show would be no regression.
    at = lambda cell, env: cell.get(env, cell["default"])
    for env in _GOLDEN["envs"][1:]:
        base = snap.ENV_BASE.get(env, "default")
        moves = any(at(cell, env) != at(cell, base) for per in _GOLDEN["digests"].values() for cell in per.values())
        assert moves or env in snap.SIZING_BLIND, env


@pytest.mark.parametrize("env_name,env", snap.ENVS, ids=[e for e, _ in snap.ENVS])
def test_probe_answers_are_the_committed_ones(env_name, env, monkeypatch):
    """A refactor of the host dispatch must leave every answer as it is; an intended routing change regenerates the file on purpose
    (and says so in the commit).  On a mismatch the answers are listed per descriptor: the digest only says that one moved."""
    for k in [k for k in os.environ if k.startswith("PASN_")]:
        monkeypatch.delenv(k)
    moved = []
    with _lib.tuning_env(**env):
        for g, (singles, pairs) in _groups().items():
            for p in snap.PROBES:
                rows = snap.answers(p, singles, pairs)
                cell = _GOLDEN["digests"][g][p]
                want = cell.get(env_name, cell["default"])  # an environment's cell is stored only where it differs from the default
                if snap.digest(rows) != want:
                    moved.append((g, p))
                    print(f"{g} / {p} / {env_name}: digest moved; answers now, in the blocks that differ:")
                    for d, a in snap.moved_blocks(rows, want):
                        print("  ", d, "->", a)
    assert not moved, f"probe answers moved under {env_name}: {moved} (the answers per descriptor are printed above)"
