"""GPU: local explanations (pasn_explain_rank / pasn_explain_maps, protoasnet_amd.explain) against the reference's own helpers (G8)
and against torch.nn.Upsample + the reference's normalisation on the CPU (tests/explain_cases.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import TOL_LOGITS, TOL_SIM, assert_close
from explain_cases import CASES, case_inputs, lut_rgb, norm_maps, overlays, rank_ref, u8_mismatch_ok
from protoasnet_amd import _lib, explain, synth
from util import CFG_VIDEO_R2P1D, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAP_TOL = 2e-6


def _check_float_maps(got, want, name):
    got = got.float().cpu()
    assert_close(got, want, MAP_TOL, 0, name)
    dims = tuple(range(1, got.dim()))
    assert float(got.amin(dim=dims).abs().max()) == 0.0, f"{name}: a map's minimum is not exactly 0"
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0, f"{name}: values outside [0, 1]"


def _proto_info(occ, src):
    return {"prototypes_occurrence_maps": occ, "prototypes_src_imgs": src}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_maps_and_overlays_vs_reference_fixture(golden, case):
    name, grid, out, seed = case
    g = golden("g8_explain.npz")
    occ, src = case_inputs(grid, out, seed)
    lut = lut_rgb(g["lut_bgr"])
    want = torch.from_numpy(g[f"{name}_maps"])
    r = explain.prototype_maps(_proto_info(occ, src), lut=lut, maps="float")
    torch.cuda.synchronize()
    _check_float_maps(r["maps"], want, f"{name} fp32 maps")
    got_u8 = explain.prototype_maps(_proto_info(occ, src), maps="uint8")["maps"]
    if sum(out[-2:]) <= 128:
        # torch's CPU upsample_bilinear2d takes its vectorised kernel for outputs with Ho + Wo <= 128 (another summation order than its
        # generic kernel, which the device follows bit for bit): maps one fp32 ulp apart, e.g. the maximum voxel at 255 (v = 1 since
        # 1e-7 vanishes next to the range) against 254.99997.  Such a voxel may differ by one within the fp32 gate's window.
        err = u8_mismatch_ok(got_u8.cpu(), want, window=255 * MAP_TOL, share=1.0)
    else:
        err = u8_mismatch_ok(got_u8.cpu(), want)
    assert err is None, f"{name}: {err}"
    # overlays on the 0-255 scale, where the uint8 maps agree (a near-integer voxel may pick the neighbouring colour)
    ov, ref_ov = r["overlays"].cpu(), torch.from_numpy(g[f"{name}_overlays"])
    same = (got_u8.cpu() == (want * 255).to(torch.uint8))[..., None].expand_as(ov)
    assert float(((ov - ref_ov).abs() * 255)[same].max()) <= 1e-4, f"{name}: overlays"


REAL = [  # (source grid, clip grid, P): R(2+1)D-18[:-3] video config, X3D-S, ResNet-18 image
    ((8, 14, 14), (32, 112, 112), 40),
    ((16, 7, 7), (16, 224, 224), 30),
    ((7, 7), (224, 224), 40),
]


@pytest.mark.parametrize("grid,out,P", REAL, ids=["r2p1d", "x3d_s", "resnet18_image"])
def test_real_shapes_vs_torch_upsample(grid, out, P):
    rng = np.random.default_rng(5)
    occ = torch.from_numpy(np.abs(rng.standard_normal((1, P, 1) + grid)).astype(np.float32))
    want = norm_maps(occ[0], out)  # (P, *out)
    video = len(grid) == 3
    occ5 = occ.reshape((1, P) + ((grid) if video else (1,) + grid)).to(DEV).contiguous()
    shape3 = out if video else (1,) + out
    m, _ = explain._maps_launch(occ5, None, P, shape3, "float", None, None, 0.3, 0.0, 1.0)
    u8, _ = explain._maps_launch(occ5, None, P, shape3, "uint8", None, None, 0.3, 0.0, 1.0)
    torch.cuda.synchronize()
    _check_float_maps(m.reshape(want.shape), want, f"{grid}->{out} fp32 maps")
    err = u8_mismatch_ok(u8.reshape(want.shape).cpu(), want)
    assert err is None, err
    # a selection table: maps of the listed prototypes, in the listed order
    pick = [P - 1, 0, 7, 7]
    sel = torch.tensor([pick], dtype=torch.int32, device=DEV)
    ms, _ = explain._maps_launch(occ5, sel, len(pick), shape3, "float", None, None, 0.3, 0.0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(ms.reshape((len(pick),) + want.shape[1:]).cpu(), m.reshape(want.shape).cpu()[pick])


def test_rank_kernel_vs_numpy():
    rng = np.random.default_rng(9)
    N, K, G = 5, 4, 1000  # P = 4000: blocks of 1000 (the constructors' default P = 2000 has 500 / 667)
    P = K * G
    sim = torch.from_numpy(rng.permutation(N * P).reshape(N, P).astype(np.float32) / (N * P))  # tie-free
    fc_w = torch.from_numpy(rng.standard_normal((K, P)).astype(np.float32))
    logits = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    outs = _rank(sim, fc_w, logits, K - 1, 7)
    contrib, totals, order, rank, pred, sel = (t.cpu() for t in outs)
    r_contrib, r_totals, r_order, r_rank, r_pred, r_sel = rank_ref(sim, fc_w, logits, K - 1, 7)
    assert torch.equal(contrib, torch.from_numpy(fc_w.numpy()[None] * sim.numpy()[:, None]))  # bitwise numpy's product
    assert float(((totals.double() - r_totals).abs() / r_totals.abs().clamp(min=1e-30)).max()) <= 1e-6
    assert torch.equal(order.long(), r_order) and torch.equal(rank.long(), r_rank)
    assert torch.equal(pred.long(), r_pred) and torch.equal(sel.long(), r_sel)


def test_rank_kernel_tie_rule():
    sim = torch.tensor([[0.5, 0.5, 0.2, 0.5, 0.1, 0.3, 0.3, 0.3]])
    fc_w = torch.ones(2, 8)
    logits = torch.tensor([[1.0, 1.0]])  # tie in the prediction: the lowest index
    contrib, totals, order, rank, pred, sel = (t.cpu() for t in _rank(sim, fc_w, logits, 2, 4))
    assert order.tolist() == [[3, 1, 0, 2, 7, 6, 5, 4]]
    assert rank.tolist() == [[2, 1, 3, 0, 3, 2, 1, 0]]
    assert pred.tolist() == [0] and sel.tolist() == [[3, 1, 0, 2]]


def _rank(sim, fc_w, logits, K_real, k_sel):
    N, P = sim.shape
    K = fc_w.shape[0]
    sim, fc_w, logits = (t.to(DEV).contiguous() for t in (sim, fc_w, logits))
    contrib = torch.empty((N, K, P), device=DEV)
    totals = torch.empty((N, K), device=DEV)
    order, rank = (torch.empty((N, P), dtype=torch.int32, device=DEV) for _ in range(2))
    pred = torch.empty((N,), dtype=torch.int32, device=DEV)
    sel = torch.empty((N, k_sel), dtype=torch.int32, device=DEV)
    lib = _lib.lib()
    _lib.check(lib.pasn_explain_rank(sim.data_ptr(), fc_w.data_ptr(), logits.data_ptr(), N, P, K, K_real, k_sel, contrib.data_ptr(),
                                     totals.data_ptr(), order.data_ptr(), rank.data_ptr(), pred.data_ptr(), sel.data_ptr(),
                                     _lib.current_stream()))
    torch.cuda.synchronize()
    return contrib, totals, order, rank, pred, sel


@pytest.mark.parametrize("cfg,shape", [(CFG_VIDEO_R2P1D, (2, 3, 8, 32, 32)), (CFG_VIDEO_X3D, (2, 3, 4, 64, 64)),
                                       (CFG_XPROTO, (2, 3, 224, 224))], ids=["r2p1d", "x3d_s", "xprotonet_image"])
def test_model_explain_end_to_end(cfg, shape):
    m = synth_model(cfg).to(DEV).eval()
    x = synth.echo_clips(shape).to(DEV)
    lut = np.random.default_rng(1).random((256, 3)).astype(np.float32)
    with torch.no_grad():
        _, pdist, occ, logits = m.push_forward(x)
    e = m.explain(x, select="predicted", maps="float", lut=lut)
    e_all = m.explain(x, maps="uint8")
    torch.cuda.synchronize()
    P, K = m.num_prototypes, m.num_classes
    G = P // K
    assert torch.equal(e.logits, logits) and torch.equal(e.proto_dist, pdist)
    assert torch.equal(e.similarities, 1 - pdist)
    assert torch.equal(e.probs, logits[:, :K - 1].softmax(1))
    r_contrib, _, r_order, r_rank, r_pred, r_sel = rank_ref(e.similarities.cpu(), m.last_layer.weight.detach().cpu(), logits.cpu(), K - 1, G)
    assert torch.equal(e.contributions.cpu(), r_contrib)
    assert torch.equal(e.order.cpu().long(), r_order) and torch.equal(e.pred.cpu().long(), r_pred)
    assert torch.equal(e.selected.cpu().long(), r_sel)
    video = x.dim() == 5
    out = tuple(x.shape[2:])
    N = x.shape[0]
    occ_c = occ.cpu().reshape((N * P, 1) + tuple(occ.shape[3:]))
    want_all = norm_maps(occ_c, out).reshape((N, P) + out)
    assert tuple(e_all.maps.shape) == (N, P) + out and e_all.maps.dtype == torch.uint8
    err = u8_mismatch_ok(e_all.maps.cpu(), want_all)
    assert err is None, err
    want_sel = torch.stack([want_all[n, e.selected[n].long().cpu()] for n in range(N)])
    _check_float_maps(e.maps.reshape((N * G,) + out), want_sel.reshape((N * G,) + out), "selected maps")
    ref_ov = overlays(want_sel.reshape((N * G,) + out), x.cpu().repeat_interleave(G, 0), lut).reshape(e.overlays.shape)
    assert tuple(e.overlays.shape) == (N, G) + out + (3,)
    same = (e.maps.cpu() * 255).to(torch.uint8) == (want_sel * 255).to(torch.uint8)
    assert float((e.overlays.cpu() - ref_ov).abs()[same].max()) <= 1e-4 / 255
    assert video == (e.maps.dim() == 5)


class _Loader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_load_data_and_model_products_vs_reference(golden, tmp_path):
    g = golden("g8_explain.npz")
    m = synth_model(CFG_XPROTO).to(DEV).eval()
    batches = []
    for bi, (seed, labels) in enumerate(((11, [0, 1]), (12, [2, 1]))):  # make_golden_explain.py::g2_loader
        batches.append({"cine": synth.echo_clips((2, 3, 224, 224), seed=seed), "target_AS": torch.tensor(labels),
                        "filename": [f"case{bi}_{a}" for a in range(2)]})
    cfg = dict(view="plax", frames=1, img_size=224, interval_quant=1.0, interval_unit="cycle", iterate_intervals=False,
               dataset_root=str(tmp_path / "data"))
    logs = []
    data, prod = explain.load_data_and_model_products(m, _Loader(batches), "val", cfg, True, str(tmp_path / "run"), log=logs.append)
    for tag, d in (("data", data), ("products", prod)):
        keys = sorted(d)
        assert keys == g[f"{tag}_keys"].tolist()
        assert [str(tuple(np.asarray(d[k]).shape)) for k in keys] == g[f"{tag}_shapes"].tolist()
        assert [str(np.asarray(d[k]).dtype) for k in keys] == g[f"{tag}_dtypes"].tolist()
    assert data["filenames"] == g["data__filenames"].tolist()
    assert np.array_equal(data["ys_gt"], g["data__ys_gt"])
    assert np.array_equal(prod["fc_layer_weights"], g["products__fc_layer_weights"])
    assert_close(prod["proto_dist_"], g["products__proto_dist_"], TOL_SIM, 0, "proto_dist_")
    assert_close(prod["ys_pred"], g["products__ys_pred"], TOL_LOGITS, 0, "ys_pred")
    assert_close(prod["occurrence_map_"], g["products__occurrence_map_"], 2e-3, 1e-3, "occurrence_map_")
    assert any("f1 score" in str(s) for s in logs)

    class NoModel:  # the second call reads the pickles back and runs nothing
        def __getattr__(self, name):
            raise AssertionError(f"the model was used ({name})")

    data2, prod2 = explain.load_data_and_model_products(NoModel(), None, "val", cfg, True, str(tmp_path / "run"), log=lambda *a: None)
    assert sorted(prod2) == sorted(prod) and np.array_equal(prod2["proto_dist_"], prod["proto_dist_"])
    assert data2["filenames"] == data["filenames"]


def test_kernels_are_bitwise_repeatable():
    rng = np.random.default_rng(4)
    N, P = 2, 40
    occ = torch.from_numpy(np.abs(rng.standard_normal((N, P, 8, 14, 14))).astype(np.float32)).to(DEV)
    src = torch.from_numpy(rng.standard_normal((N, 1, 32, 112, 112)).astype(np.float32)).to(DEV)
    lut = torch.from_numpy(rng.random((256, 3)).astype(np.float32)).to(DEV)
    sel = torch.from_numpy(rng.integers(0, P, (N, 3)).astype(np.int32)).to(DEV)
    sim = torch.from_numpy(rng.random((8, 2000)).astype(np.float32))
    fc_w = torch.from_numpy(rng.standard_normal((4, 2000)).astype(np.float32))
    logits = torch.from_numpy(rng.standard_normal((8, 4)).astype(np.float32))
    first = None
    for _ in range(25):
        f, _ = explain._maps_launch(occ, None, P, (32, 112, 112), "float", None, None, 0.3, 0.0, 1.0)
        q, ov = explain._maps_launch(occ, sel, 3, (32, 112, 112), "uint8", lut, src, 0.3, 0.099, 0.171)
        r = _rank(sim, fc_w, logits, 3, 5)
        now = [f, q, ov] + list(r)
        if first is None:
            first = [t.clone() for t in now]
        else:
            for a, b in zip(first, now):
                assert torch.equal(a, b)
    torch.cuda.synchronize()
