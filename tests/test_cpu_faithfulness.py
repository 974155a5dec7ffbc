"""CPU: explanation faithfulness -- the C-ABI / Python surface with its argument checks (no device), step_counts by hand, and the numpy
restatement of tests/faithfulness_cases.py (what the GPU tests hold the kernels to) against the definition, voxel by voxel."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import faithfulness_cases as fc
import protoasnet_amd
from protoasnet_amd import _lib, faithfulness, model_builder
from util import CFG_PPNET, CFG_XPROTO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_perturb_steps_workspace_bytes", "pasn_perturb_steps", "pasn_perturb_apply", "pasn_perturb_curves")


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pasn_\w+)", nm))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
        assert getattr(lib, name) is not None
    assert "faithfulness" in protoasnet_amd.__all__ and protoasnet_amd.faithfulness is faithfulness
    assert "perturb.hip" in protoasnet_amd.build.SOURCES


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def steps(M=6, V=1000, S1=11, **null):
        p = dict(maps=fake, counts=fake, steps=fake, workspace=fake)
        p.update(null)
        return lib.pasn_perturb_steps(p["maps"], p["counts"], M, V, S1, p["steps"], p["workspace"], 0)

    size = lib.pasn_perturb_steps_workspace_bytes
    for S1 in (0, 65):
        assert steps(S1=S1) == 1 and size(6, 1000, S1) == 0
    with pytest.raises(ValueError, match="S1"):
        _lib.check(steps(S1=65))
    for V in (0, 1 << 31):
        assert steps(V=V) == 1 and size(6, V, 11) == 0
    with pytest.raises(ValueError, match="V must lie"):
        _lib.check(steps(V=1 << 31))
    for M in (0, 65536):
        assert steps(M=M) == 1 and size(M, 1000, 11) == 0
    for k in ("maps", "counts", "steps", "workspace"):
        assert steps(**{k: 0}) == 1, k
    assert steps(maps=264) == 1 and steps(steps=257) == 1  # misaligned
    # the workspace grows with the tiles of 4096 voxels, not with S1; an odd V may need one tile more (rows start anywhere)
    assert size(6, 4096, 1) == size(6, 4096, 64) > 0 and size(6, 4097, 11) > size(6, 4096, 11)
    assert size(12, 802816, 11) == 2 * size(6, 802816, 11) and size(6, 802816, 11) % 16 == 0

    def apply(N=2, C=3, k=2, V=1000, Sc=3, mode=0, dtype=_lib.F32, **null):
        p = dict(x=fake, steps=fake, step_ids=fake, baseline=0, out=fake)
        p.update(null)
        return lib.pasn_perturb_apply(p["x"], p["steps"], p["step_ids"], p["baseline"], 0.0, N, C, k, V, Sc, mode, dtype, p["out"], 0)

    for k in ("x", "steps", "step_ids", "out"):
        assert apply(**{k: 0}) == 1, k
    for bad in (dict(mode=2), dict(mode=-1), dict(dtype=_lib.U8), dict(dtype=_lib.I32), dict(V=0), dict(V=1 << 31), dict(C=0), dict(C=65),
                dict(Sc=0), dict(N=0), dict(k=0), dict(N=256, k=256), dict(x=258), dict(baseline=258, dtype=_lib.F32)):
        assert apply(**bad) == 1, bad
    with pytest.raises(ValueError, match="mode"):
        _lib.check(apply(mode=2))
    with pytest.raises(ValueError, match="dtype"):
        _lib.check(apply(dtype=_lib.U8))

    def curves(N=3, k=2, S1=5, P=12, K=4, K_real=3, V=1000, **null):
        p = dict(sim=fake, logits=fake, sel=fake, cls=fake, counts=fake, curve_sim=fake, curve_prob=fake, auc=fake, acc=0)
        p.update(null)
        return lib.pasn_perturb_curves(p["sim"], p["logits"], p["sel"], p["cls"], p["counts"], N, k, S1, P, K, K_real, V, p["curve_sim"],
                                       p["curve_prob"], p["auc"], p["acc"], 0)

    for k in ("sim", "logits", "sel", "cls", "counts", "curve_sim", "curve_prob", "auc"):
        assert curves(**{k: 0}) == 1, k
    for bad in (dict(S1=0), dict(S1=65), dict(V=0), dict(V=1 << 31), dict(K_real=0), dict(K_real=17, K=17), dict(K=2), dict(K=18), dict(P=0),
                dict(N=0), dict(k=0), dict(N=1 << 12, k=1 << 6)):
        assert curves(**bad) == 1, bad
    with pytest.raises(ValueError, match="S1"):
        _lib.check(curves(S1=65))


def test_python_surface_refuses_what_it_cannot_run():
    with pytest.raises(NotImplementedError):
        faithfulness.perturbation_curves(model_builder.build(CFG_PPNET).eval(), torch.zeros(1, 3, 224, 224))
    m = model_builder.build(CFG_XPROTO).eval()
    assert m.faithfulness.__func__ is type(m).faithfulness  # on the head-B mixin, next to explain
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.faithfulness(x)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.faithfulness(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        faithfulness.removal_steps(torch.zeros(1, 1, 4, 4, dtype=torch.uint8), [0, 16])
    with pytest.raises(TypeError):
        faithfulness.removal_steps(torch.zeros(1, 1, 4, 4), [0, 16])
    with pytest.raises(ValueError, match="mode"):
        faithfulness.perturb(x, torch.zeros(1, 1, 224, 224, dtype=torch.uint8), [0], "blur")
    assert faithfulness.accumulator_size(2, 5) == 2 * 2 * 5 + 2 * 2 + 1


# ---- step_counts ---------------------------------------------------------------------------------------------------------------------------
def test_step_counts_by_hand():
    sc = faithfulness.step_counts
    assert sc(7, steps=2) == [0, 4, 7]                       # 3.5 rounds half up
    assert sc(10, 4) == [0, 3, 5, 8, 10]                     # 2.5 -> 3, 7.5 -> 8
    assert sc(802816, 10) == [802816 * s // 10 + (1 if (802816 * s) % 10 >= 5 else 0) for s in range(11)]
    assert sc(7, fractions=[0.0, 0.5, 1.0]) == [0, 4, 7] and sc(7, fractions=[0.07]) == [0] and sc(7, fractions=[0.08]) == [1]
    for V in (1, 2, 7, 8993, 802816, (1 << 31) - 1):
        for steps in (1, 2, 10, 63):
            c = sc(V, steps)
            assert len(c) == steps + 1 and c[0] == 0 and c[-1] == V and all(b >= a for a, b in zip(c, c[1:]))
            assert all(isinstance(v, int) and abs(v - s * V / steps) <= 0.5 for s, v in enumerate(c))
    for bad in (dict(steps=0), dict(steps=64), dict(steps=2.0), dict(steps=True), dict(fractions=[]), dict(fractions=[0.5, 0.4]),
                dict(fractions=[1.5]), dict(fractions=[0.0] * 65)):
        with pytest.raises(ValueError):
            sc(100, **bad)
    with pytest.raises(ValueError):
        sc(0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_steps_ref_against_the_definition_with_ties():
    rng = np.random.default_rng(11)
    level = rng.integers(0, 4, 50).astype(np.uint8) * 60  # four levels over 50 voxels: every level is a long tie
    level[:5] = 180                                       # and the order inside a tie is the index
    for counts in ([0, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50], [0, 0, 17, 17, 30], [1], [49], [50], [0], list(range(0, 50, 7))):
        want = fc.steps_brute(level, counts)
        got = fc.steps_ref(level[None], counts)[0]
        assert got.dtype == np.uint8 and got.tolist() == want.tolist(), counts
        for s, c in enumerate(counts):
            assert int((got <= s).sum()) == c  # exactly counts[s] voxels are touched at step s
        assert fc._steps_sorted_equal(level[None], counts)
    # the first voxels of the highest level go first; a constant map goes in index order
    assert fc.steps_ref(np.full((1, 6), 9, np.uint8), [2, 4]).tolist() == [[0, 0, 1, 1, 2, 2]]
    assert fc.steps_ref(np.array([[1, 3, 3, 2, 3, 1]], np.uint8), [1, 3, 4, 6]).tolist() == [[3, 0, 1, 2, 1, 3]]


def test_apply_and_curves_restatements_by_hand():
    x = np.arange(12, dtype=np.float32).reshape(1, 2, 6)
    steps = np.array([[[0, 0, 1, 1, 2, 2]]], np.uint8)
    dele = fc.apply_ref(x, steps, [1, 0], 0, fill=-1.0)
    assert dele.shape == (1, 1, 2, 2, 6)
    assert dele[0, 0, 0].tolist() == [[-1, -1, -1, -1, 4, 5], [-1, -1, -1, -1, 10, 11]]
    assert dele[0, 0, 1].tolist() == [[-1, -1, 2, 3, 4, 5], [-1, -1, 8, 9, 10, 11]]
    ins = fc.apply_ref(x, steps, [0], 1, baseline=-x)
    assert ins[0, 0, 0, 0].tolist() == [0, 1, -2, -3, -4, -5]
    # two steps, one prototype, two real classes: the probability of class 1 goes 1/2 -> e / (1 + e)
    sim = np.array([[[[0.25, 0.75], [0.5, 0.125]]]], np.float32)
    logits = np.array([[[[0.0, 0.0, 9.0], [0.0, 1.0, 9.0]]]], np.float32)
    cs, cp, auc = fc.curves_ref(sim, logits, [[1]], [1], [0, 8], 8, K_real=2)
    assert cs.tolist() == [[[0.75, 0.125]]] and np.allclose(cp, [[[0.5, np.e / (1 + np.e)]]], rtol=1e-15)
    assert np.allclose(auc, [[[0.4375, (0.5 + np.e / (1 + np.e)) / 2]]], rtol=1e-15)
    assert fc.trapezoid([1.0, 3.0, 3.0], [0, 2, 8], 8) == 0.25 * 2.0 + 0.75 * 3.0
