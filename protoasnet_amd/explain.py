"""Local explanations of the head-B models (``XProtoNet``, ``Video_XProtoNet``): which prototypes a clip resembles and where.

Drop-in for the arithmetic under the reference's ``explain_local`` (``src/utils/local_explainability.py:17-200``) and its helpers
(``src/utils/explainability_utils.py:11-200``): class contributions, the per-class ranking of the prototypes, the occurrence maps
upsampled to the clip and min-max normalised, and the colour-mapped overlays.  The GIF / matplotlib rendering stays with the caller.

* ``explain_batch(model, x, ...)`` (also ``model.explain(x, ...)``): one ``push_forward``, one ``pasn_explain_rank`` and one
  ``pasn_explain_maps`` call (two launches) on the current stream, no host synchronisation.
* ``prototype_maps(prototypes_info, ...)``: the same maps / overlays for the pushed prototypes (local_explainability.py:61-76), from the
  ``prototypes_info.pickle`` that ``push.push_prototypes`` writes.
* ``load_data_and_model_products(...)``: the reference's two pickles (explainability_utils.py:11-132), same paths, keys, shapes and
  dtypes, so the reference's own ``explain_local`` can sit on top.

No colour map is built in: ``lut`` is a (256, 3) table of the caller's, indexed by ``uint8(255 * map)``.  The reference's
``get_heatmap`` (cv2.COLORMAP_TURBO, BGR, divided by 255, then flipped to RGB) is ``lut = turbo_bgr[:, ::-1] / 255``.
"""
from __future__ import annotations

import ctypes
import os
import pickle
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np
import torch

from . import _lib
from .data import ECHO_MEAN, ECHO_STD

MAPS = ("float", "uint8", None)


@dataclass
class Explanation:
    """Device tensors of one batch.  P prototypes, K classes (K_real without the abstain class), G = P / K per class, k selected."""

    logits: torch.Tensor         # (N, K)
    probs: torch.Tensor          # (N, K_real): softmax over the non-abstain logits (explainability_utils.py:69-72)
    similarities: torch.Tensor   # (N, P): 1 - proto_dist, as the reference recomputes it (local_explainability.py:55)
    proto_dist: torch.Tensor     # (N, P)
    contributions: torch.Tensor  # (N, K, P): last_layer.weight[k, p] * similarities[n, p]
    totals: torch.Tensor         # (N, K): similarities @ last_layer.weight.T
    order: torch.Tensor          # (N, P) int32: per class block, prototype indices by descending similarity (ties: higher index first)
    rank: torch.Tensor           # (N, P) int32: position of each prototype in its block's order
    pred: torch.Tensor           # (N,) int32: argmax of the non-abstain logits
    selected: torch.Tensor       # (N, k) int32: the prototypes the maps belong to
    maps: Optional[torch.Tensor] = None      # (N, k, [To,] Ho, Wo) fp32 in [0, 1] or uint8
    overlays: Optional[torch.Tensor] = None  # (N, k, [To,] Ho, Wo, 3) fp32


def _is_xproto(model) -> bool:
    from .nets import _XProtoHeadMixin

    return isinstance(model, _XProtoHeadMixin)


# entry point -> the words of its messages: what it covers, why PPNet is out
_COVERS = {"explain": ("local explanations cover", "the reference has none for PPNet"),
           "faithfulness": ("faithfulness curves cover", "PPNet has no occurrence maps"),
           "saliency": ("RISE saliency covers", "PPNet has no occurrence maps to compare it with"),
           "robustness": ("robustness evaluation covers", "PPNet has no occurrence maps")}


def _check_model(model, x: torch.Tensor, what: str, maps: Optional[str] = None) -> None:
    """A head-B model, in eval mode, with its input on the GPU: the checks of ``explain_batch`` (``what`` = "explain", which also
    passes its ``maps``), ``perturbation_curves`` ("faithfulness"), ``rise`` ("saliency") and ``stability`` ("robustness"), in the order they fire."""
    covers, why = _COVERS[what]
    if not _is_xproto(model):
        raise NotImplementedError(f"{covers} XProtoNet and Video_XProtoNet; {why}")
    if maps not in MAPS:
        raise ValueError(f"maps must be one of {MAPS}, got {maps!r}")
    if model.training:
        raise RuntimeError(f"{what} runs in eval mode (call model.eval())")
    if not x.is_cuda:
        raise RuntimeError("protoasnet_amd models run on the GPU only; there is no CPU fallback")


def _int_select(select, per_clip: str) -> int:
    if isinstance(select, bool) or not isinstance(select, (int, np.integer)):
        raise TypeError(f"select must be an int ({per_clip}), got {type(select).__name__}")
    return int(select)


def _dimensions(model, abstain_class: bool):
    """(P, K, G, K_real): prototypes, classes, prototypes per class block, classes without the abstain class."""
    P, K = int(model.num_prototypes), int(model.num_classes)
    if P % K:
        raise ValueError(f"{P} prototypes do not split into {K} class blocks")
    from .prune import require_balanced

    require_balanced(model, "the explanation (it ranks within class blocks)")  # (7, 10, 10 prototypes also divide by 3)
    return P, K, P // K, K - 1 if abstain_class else K


def _check_lut(lut, device) -> Optional[torch.Tensor]:
    if lut is None:
        return None
    lut = torch.as_tensor(lut)
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"lut must be a (256, 3) colour table, got {tuple(lut.shape)}")
    return lut.to(device=device, dtype=torch.float32).contiguous()


def _select_count(select, G: int, P: int) -> Optional[int]:
    """None -> all P maps in index order; "predicted" -> the predicted class's G prototypes, ranked; int k -> the first k of those."""
    if select is None:
        return None
    if isinstance(select, str):
        if select != "predicted":
            raise ValueError(f"select must be None, 'predicted' or an int, got {select!r}")
        return G
    if isinstance(select, bool) or not isinstance(select, (int, np.integer)):
        raise TypeError(f"select must be None, 'predicted' or an int, got {type(select).__name__}")
    if not 1 <= int(select) <= G:
        raise ValueError(f"select={select} must lie in [1, {G}] (prototypes per class)")
    return int(select)


def _maps_launch(occ, sel, k, out_shape, maps, lut, src, alpha, mean, std):
    """occ (N, P, Ti, Hi, Wi) fp32 -> maps (N, k, To, Ho, Wo) and / or overlays (N, k, To, Ho, Wo, 3) (None where not asked)."""
    N, P, Ti, Hi, Wi = (int(v) for v in occ.shape)
    To, Ho, Wo = out_shape
    dev = occ.device
    lib = _lib.lib()
    m = None
    if maps is not None:
        m = torch.empty((N, k, To, Ho, Wo), dtype=torch.float32 if maps == "float" else torch.uint8, device=dev)
    ov = torch.empty((N, k, To, Ho, Wo, 3), dtype=torch.float32, device=dev) if lut is not None else None
    if m is None and ov is None:
        return None, None
    ws = torch.empty(int(lib.pasn_explain_maps_workspace_bytes(N, P, k, Ti, Hi, Wi, To, Ho, Wo)), dtype=torch.uint8, device=dev)
    src_code, src_c = 0, 1
    if ov is not None:
        src_code, src_c = _lib.dtype_code(src.dtype), int(src.shape[1])
    _lib.check(lib.pasn_explain_maps(
        occ.data_ptr(), _lib.ptr(sel), N, P, k, Ti, Hi, Wi, To, Ho, Wo, _lib.ptr(m), _lib.U8 if maps == "uint8" else _lib.F32,
        _lib.ptr(ov), _lib.ptr(src if ov is not None else None), src_code, src_c, _lib.ptr(lut), float(mean), float(std), float(alpha),
        ws.data_ptr(), _lib.current_stream()))
    return m, ov


def _clip_geometry(x: torch.Tensor):
    """(video, (To, Ho, Wo)) of a model input (N, C, [T,] H, W)."""
    if x.dim() == 5:
        return True, tuple(int(v) for v in x.shape[2:])
    if x.dim() == 4:
        return False, (1, int(x.shape[2]), int(x.shape[3]))
    raise ValueError(f"the clip must be (N, C, T, H, W) or (N, C, H, W), got {tuple(x.shape)}")


def _check_src(x: torch.Tensor) -> None:
    if x.shape[1] not in (1, 3):
        raise ValueError(f"overlays need a 1- or 3-channel clip, got {x.shape[1]} channels")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"overlays need the normalised fp32 / bf16 model input, got {x.dtype}")


def explain_batch(model, x: torch.Tensor, select: Union[None, str, int] = None, maps: Optional[str] = "float", lut=None,
                  alpha: float = 0.3, abstain_class: bool = True, mean: float = ECHO_MEAN, std: float = ECHO_STD) -> Explanation:
    """Local explanation of the clips ``x`` (the model's input, on the GPU).  ``select``: None = all P maps in index order (what the
    reference renders), "predicted" = the predicted class's prototypes by descending similarity, int k = the first k of those.
    ``maps``: "float" (normalised fp32), "uint8" (``np.uint8(255 * map)``) or None.  ``lut`` (256, 3): also the overlays
    ``(x * std + mean) + alpha * lut[uint8 map]``."""
    _check_model(model, x, "explain", maps)
    P, K, G, K_real = _dimensions(model, abstain_class)
    if K_real < 1:
        raise ValueError("abstain_class needs at least two classes")
    k_sel = _select_count(select, G, P)
    video, out_shape = _clip_geometry(x)
    lut = _check_lut(lut, x.device)
    if lut is not None:
        _check_src(x)
    with torch.no_grad():
        _, proto_dist, occ, logits = model.push_forward(x)
        sim = (1 - proto_dist).contiguous()
        probs = logits[:, :K_real].softmax(dim=1)
        N, dev = int(x.shape[0]), x.device
        fcw = model.last_layer.weight.detach().to(torch.float32).contiguous()
        contrib = torch.empty((N, K, P), dtype=torch.float32, device=dev)
        totals = torch.empty((N, K), dtype=torch.float32, device=dev)
        order = torch.empty((N, P), dtype=torch.int32, device=dev)
        rank = torch.empty((N, P), dtype=torch.int32, device=dev)
        pred = torch.empty((N,), dtype=torch.int32, device=dev)
        sel = torch.empty((N, k_sel), dtype=torch.int32, device=dev) if k_sel is not None else None
        lib = _lib.lib()
        _lib.check(lib.pasn_explain_rank(sim.data_ptr(), fcw.data_ptr(), logits.contiguous().data_ptr(), N, P, K, K_real, k_sel or 0,
                                         contrib.data_ptr(), totals.data_ptr(), order.data_ptr(), rank.data_ptr(), pred.data_ptr(),
                                         _lib.ptr(sel), _lib.current_stream()))
        occ5 = occ.reshape(N, P, *(occ.shape[3:] if video else (1,) + tuple(occ.shape[3:]))).contiguous()
        k = P if sel is None else k_sel
        m, ov = _maps_launch(occ5, sel, k, out_shape, maps, lut, x.contiguous(), alpha, mean, std)
    if not video:  # images keep the reference's (P, Ho, Wo) layout: no frame axis
        m = None if m is None else m.squeeze(2)
        ov = None if ov is None else ov.squeeze(2)
    selected = sel if sel is not None else torch.arange(P, dtype=torch.int32, device=dev).expand(N, P)
    return Explanation(logits=logits, probs=probs, similarities=sim, proto_dist=proto_dist, contributions=contrib, totals=totals,
                       order=order, rank=rank, pred=pred, selected=selected, maps=m, overlays=ov)


def prototype_maps(prototypes_info, lut=None, maps: Optional[str] = "float", alpha: float = 0.3, mean: float = ECHO_MEAN,
                   std: float = ECHO_STD, device="cuda"):
    """The pushed prototypes' normalised maps and overlays (local_explainability.py:61-76) from ``prototypes_info.pickle`` (a path or
    the loaded dict): ``{"maps": (P, [To,] Ho, Wo), "overlays": (P, [To,] Ho, Wo, 3) or None}`` on ``device``.  The P winners are run
    as P clips of one map each through the same kernel; every dimension is kept (the reference's ``.squeeze()`` drops P at P = 1)."""
    if isinstance(prototypes_info, (str, os.PathLike)):
        with open(prototypes_info, "rb") as handle:
            prototypes_info = pickle.load(handle)
    if maps not in MAPS:
        raise ValueError(f"maps must be one of {MAPS}, got {maps!r}")
    occ = torch.as_tensor(np.asarray(prototypes_info["prototypes_occurrence_maps"]), dtype=torch.float32)  # (P, 1, [T,] H, W)
    src = torch.as_tensor(np.asarray(prototypes_info["prototypes_src_imgs"]))                             # (P, 3, [To,] Ho, Wo)
    if occ.dim() not in (4, 5) or occ.shape[1] != 1 or occ.shape[0] != src.shape[0] or src.dim() != occ.dim():
        raise ValueError(f"prototypes_info: occurrence maps {tuple(occ.shape)} do not match source images {tuple(src.shape)}")
    video = occ.dim() == 5
    P = int(occ.shape[0])
    occ5 = (occ if video else occ.unsqueeze(2)).to(device).contiguous()  # (P, 1, Ti, Hi, Wi): P clips of one map
    src = src.to(device=device, dtype=torch.float32).contiguous()
    out_shape = tuple(int(v) for v in src.shape[2:]) if video else (1, int(src.shape[2]), int(src.shape[3]))
    lut = _check_lut(lut, src.device)
    if lut is not None:
        _check_src(src)
    if maps is None and lut is None:
        raise ValueError("nothing to compute: pass maps='float' / 'uint8' and / or a lut")
    with torch.no_grad():
        m, ov = _maps_launch(occ5, None, 1, out_shape, maps, lut, src, alpha, mean, std)
    m = None if m is None else m.reshape((P,) + tuple(m.shape[2:] if video else m.shape[3:]))
    ov = None if ov is None else ov.reshape((P,) + tuple(ov.shape[2:] if video else ov.shape[3:]))
    return {"maps": m, "overlays": ov}


# ------------------------------------------------------------------------------------------------- the reference's product pickles
def _products_paths(mode, data_config, root_dir_for_saving):
    filename = (
        f'{data_config["view"]}_'
        f'{data_config["frames"]}x{data_config["img_size"]}_'
        f'{data_config["interval_quant"]:.1f}x{data_config["interval_unit"]}_'
        f'{"all-Intervals" if data_config["iterate_intervals"] else ""}_'
        f"{mode}_data"
    )
    return (f'{data_config["dataset_root"]}/pickled_datasets/{filename}.pickle', f"{root_dir_for_saving}/{mode}/model_products.pickle")


def _load(path, log):
    with open(path, "rb") as handle:
        data = pickle.load(handle)
    log(f"data successfully loaded from {path}")
    return data


def _save(data, path, log):
    with open(path, "wb") as handle:
        pickle.dump(data, handle, protocol=pickle.HIGHEST_PROTOCOL)
    log(f"data successfully saved in {path}")


def load_data_and_model_products(model, dataloader, mode, data_config, abstain_class, root_dir_for_saving, log=print):
    """Reference signature (explainability_utils.py:11-132): one pass over ``dataloader`` through the HIP ``push_forward``; the data
    dict (``inputs``, ``ys_gt``, ``filenames``) and the model products (``fc_layer_weights``, ``protoL_input_``, ``proto_dist_``,
    ``occurrence_map_``, ``ys_pred``) are pickled at the reference's paths and returned.  When both pickles exist they are loaded and
    nothing runs.  The sanity log reports ``trainer.confusion_to_metrics`` (per-class F1, balanced accuracy) instead of sklearn's."""
    from .trainer import confusion_to_metrics

    data_dict_path, model_products_path = _products_paths(mode, data_config, root_dir_for_saving)
    os.makedirs(os.path.dirname(data_dict_path), exist_ok=True)
    os.makedirs(os.path.dirname(model_products_path), exist_ok=True)
    if os.path.exists(data_dict_path) and os.path.exists(model_products_path):
        data_dict = _load(data_dict_path, log)
        log(f"img  and labels and filenames of {mode}-dataset is loaded")
        model_products_dict = _load(model_products_path, log)
        log(f"model products for model {root_dir_for_saving} for {mode}-dataset is loaded")
        return data_dict, model_products_dict
    log(f"model products not saved. running the epoch on {mode}-dataset to save the results.")
    model.eval()
    device = model.prototype_vectors.device
    K_real = model.num_classes - 1 if abstain_class else model.num_classes
    protoL_input_, proto_dist_, occurrence_map_, ys_pred, inputs, ys_gt, filenames = [], [], [], [], [], [], []
    fc_layer_weights = model.last_layer.weight.detach().cpu().numpy()
    for sample in dataloader:
        batch = sample["cine"]
        inputs.extend(batch.detach().cpu().numpy())
        ys_gt.extend(torch.as_tensor(sample["target_AS"]).detach().cpu().numpy())
        filenames.extend(sample["filename"])
        with torch.no_grad():
            feats, dist, occ, logits = model.push_forward(batch.to(device))
            prob = logits[:, :K_real].softmax(dim=1)
        protoL_input_.extend(feats.cpu().numpy())
        proto_dist_.extend(dist.cpu().numpy())
        occurrence_map_.extend(occ.cpu().numpy())
        ys_pred.extend(prob.cpu().numpy())
    protoL_input_ = np.asarray(protoL_input_)      # (N, P, D)
    proto_dist_ = np.asarray(proto_dist_)          # (N, P)
    occurrence_map_ = np.asarray(occurrence_map_)  # (N, P, 1, [T,] H, W)
    inputs = np.asarray(inputs)                    # (N, 3, [To,] Ho, Wo)
    ys_gt = np.asarray(ys_gt)                      # (N,)
    ys_pred = np.asarray(ys_pred)                  # (N, K_real)

    pred_class = ys_pred.argmax(axis=1)
    n_labels = max(K_real, int(ys_gt.max()) + 1 if ys_gt.size else 0, int(pred_class.max()) + 1 if pred_class.size else 0)
    cm = torch.zeros((n_labels, n_labels), dtype=torch.int64)
    cm.index_put_((torch.as_tensor(ys_gt, dtype=torch.int64), torch.as_tensor(pred_class, dtype=torch.int64)),
                  torch.ones(len(ys_gt), dtype=torch.int64), accumulate=True)
    metrics = confusion_to_metrics(cm[:K_real, :K_real] if n_labels == K_real else cm)
    log(f"f1 score is {np.asarray(metrics['f1'])} with mean {metrics['f1_mean']}")
    log(f"balanced accuracy is {metrics['accuracy']}")
    log(f"confusion matrix [true, predicted] is \n{cm.numpy()}")

    data_dict = {"inputs": inputs, "ys_gt": ys_gt, "filenames": filenames}
    model_products_dict = {
        "fc_layer_weights": fc_layer_weights,
        "protoL_input_": protoL_input_,
        "proto_dist_": proto_dist_,
        "occurrence_map_": occurrence_map_,
        "ys_pred": ys_pred,
    }
    _save(data_dict, data_dict_path, log)
    _save(model_products_dict, model_products_path, log)
    return data_dict, model_products_dict
