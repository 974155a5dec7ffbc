"""CPU: local explanations -- argument validation, the PPNet refusal, the selection rule, and the G8 fixture against the torch
restatement (tests/explain_cases.py) the GPU tests use."""
import numpy as np
import pytest
import torch

from explain_cases import CASES, case_inputs, lut_rgb, norm_maps, overlays, rank_ref
from protoasnet_amd import _lib, explain, model_builder
from util import CFG_PPNET, CFG_XPROTO


def test_ppnet_has_no_local_explanation():
    m = model_builder.build(CFG_PPNET).eval()
    with pytest.raises(NotImplementedError):
        explain.explain_batch(m, torch.zeros(1, 3, 224, 224))


def test_argument_validation():
    m = model_builder.build(CFG_XPROTO).eval()  # 40 prototypes, 4 classes: 10 per class
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(ValueError):
        explain.explain_batch(m, x, maps="png")
    with pytest.raises(RuntimeError, match="GPU only"):
        explain.explain_batch(m, x)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        explain.explain_batch(m, x)
    assert explain._select_count(None, 10, 40) is None
    assert explain._select_count("predicted", 10, 40) == 10
    assert explain._select_count(3, 10, 40) == 3
    for bad in (0, 11, -1):
        with pytest.raises(ValueError):
            explain._select_count(bad, 10, 40)
    with pytest.raises(ValueError):
        explain._select_count("all", 10, 40)
    with pytest.raises(TypeError):
        explain._select_count(2.0, 10, 40)
    with pytest.raises(ValueError):
        explain._check_lut(np.zeros((255, 3)), "cpu")
    with pytest.raises(ValueError):
        explain.prototype_maps({"prototypes_occurrence_maps": np.zeros((3, 1, 4, 4), np.float32),
                                "prototypes_src_imgs": np.zeros((2, 3, 8, 8), np.float32)}, device="cpu")


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first
    with pytest.raises(ValueError, match="multiple of K"):
        _lib.check(lib.pasn_explain_rank(fake, fake, fake, 1, 10, 3, 2, 0, 0, 0, fake, 0, fake, 0, 0))
    with pytest.raises(ValueError, match="k_sel"):
        _lib.check(lib.pasn_explain_rank(fake, fake, fake, 1, 9, 3, 2, 4, 0, 0, fake, 0, fake, fake, 0))
    with pytest.raises(ValueError, match="K_real"):
        _lib.check(lib.pasn_explain_rank(fake, fake, fake, 1, 9, 3, 4, 0, 0, 0, fake, 0, fake, 0, 0))
    args = dict(maps=fake, dt=_lib.F32, ov=0, src=0, sdt=0, sc=1, lut=0)
    with pytest.raises(ValueError, match="k must equal P"):
        _lib.check(lib.pasn_explain_maps(fake, 0, 1, 4, 2, 1, 7, 7, 1, 224, 224, args["maps"], args["dt"], 0, 0, 0, 1, 0, 0.0, 1.0, 0.3, fake, 0))
    with pytest.raises(ValueError, match="nothing to write"):
        _lib.check(lib.pasn_explain_maps(fake, 0, 1, 4, 4, 1, 7, 7, 1, 224, 224, 0, _lib.F32, 0, 0, 0, 1, 0, 0.0, 1.0, 0.3, fake, 0))
    with pytest.raises(ValueError, match="colour table"):
        _lib.check(lib.pasn_explain_maps(fake, 0, 1, 4, 4, 1, 7, 7, 1, 224, 224, 0, _lib.F32, fake, fake, _lib.F32, 3, 0, 0.0, 1.0, 0.3,
                                         fake, 0))
    # a source grid whose interpolated rows do not fit LDS is refused, not served by a slow path
    rc = lib.pasn_explain_maps(fake, 0, 1, 4, 4, 1, 64, 64, 1, 512, 512, fake, _lib.F32, 0, 0, 0, 1, 0, 0.0, 1.0, 0.3, fake, 0)
    assert rc == 3 and b"LDS" in lib.pasn_last_error()
    # workspace: one (min, max) pair per (map, frame, row band)
    ws = lib.pasn_explain_maps_workspace_bytes(8, 40, 40, 8, 14, 14, 32, 112, 112)
    assert ws > 0 and ws % (8 * 40 * 32 * 8) == 0


def test_select_rule_on_a_hand_built_order():
    # 2 classes x 4 prototypes; class 1 holds a tie (0.5 at prototypes 5 and 7): the higher index ranks first
    sim = torch.tensor([[0.1, 0.9, 0.3, 0.2, 0.4, 0.5, 0.0, 0.5]])
    fc_w = torch.arange(16, dtype=torch.float32).reshape(2, 8) / 10
    logits = torch.tensor([[0.0, 2.0, 5.0]])  # the abstain logit (index 2) is the largest but does not count
    contrib, totals, order, rank, pred, sel = rank_ref(sim, fc_w, logits, K_real=2, k_sel=3)
    assert order.tolist() == [[1, 2, 3, 0, 7, 5, 4, 6]]
    assert rank.tolist() == [[3, 0, 1, 2, 2, 1, 3, 0]]
    assert pred.tolist() == [1] and sel.tolist() == [[7, 5, 4]]
    # tie-free: the reference's own expression (np.argsort reversed per class block, local_explainability.py:112-125)
    s = np.random.default_rng(3).permutation(12).astype(np.float32)[None] / 12
    _, _, order, _, _, _ = rank_ref(s, np.ones((3, 12), np.float32), np.zeros((1, 3), np.float32), K_real=2)
    ref = np.concatenate([np.argsort(s[0, c * 4:(c + 1) * 4])[::-1] + 4 * c for c in range(3)])
    assert order[0].tolist() == ref.tolist()
    assert torch.equal(contrib, fc_w[None] * sim[:, None])
    assert torch.allclose(totals.float(), sim @ fc_w.T)


def test_g8_fixture_against_the_torch_restatement(golden):
    g = golden("g8_explain.npz")
    lut = lut_rgb(g["lut_bgr"])
    for name, grid, out, seed in CASES:
        occ, src = case_inputs(grid, out, seed)
        maps = norm_maps(occ, out)
        want = torch.from_numpy(g[f"{name}_maps"])
        assert torch.equal(maps, want), f"{name}: maps"
        assert float(maps.amin(dim=tuple(range(1, maps.dim()))).abs().max()) == 0.0
        ov = overlays(want, src, lut)
        assert torch.equal(ov, torch.from_numpy(g[f"{name}_overlays"])), f"{name}: overlays"


def test_g8_products_layout(golden):
    g = golden("g8_explain.npz")
    assert g["products_keys"].tolist() == ["fc_layer_weights", "occurrence_map_", "protoL_input_", "proto_dist_", "ys_pred"]
    assert g["data_keys"].tolist() == ["filenames", "inputs", "ys_gt"]
    shapes = dict(zip(g["products_keys"].tolist(), g["products_shapes"].tolist()))
    assert shapes["occurrence_map_"] == "(4, 40, 1, 7, 7)" and shapes["ys_pred"] == "(4, 3)" and shapes["protoL_input_"] == "(4, 40, 512)"
    probs = g["products__ys_pred"]
    np.testing.assert_allclose(probs.sum(1), 1.0, rtol=1e-6)
