"""Ordinal evaluation on the device (``csrc/ordinal.hip``): the statistics that use the ORDER of the classes.

Aortic-stenosis severity is a graded label (class index = grade: ``No AS < Early AS < Significant AS``), and everything else the package
reports treats the classes as unordered names.  Two questions need the order.  How far off are the errors, and in which direction?
``agreement``: mean absolute grade error, within-one-grade accuracy, under- and over-grading rates, linear and quadratic weighted kappa.
Can it screen?  ``screen``: for every cut ``grade >= c`` of the scale, the ROC and precision-recall areas of the score ``p[c] + ... +
p[K - 1]``, operating points (the threshold that reaches a stated specificity or sensitivity, and Youden's), the tallies at thresholds
fitted on another split (``fit_operating_points`` on ``val``, applied unchanged on ``test``) and net benefit -- for the sample and for
grouped-bootstrap replicates that are ``bootstrap.replicates``' own resamples.  The reference has no code for any of this: the
definitions in ``include/protoasnet_amd.h`` ("Ordinal evaluation") are the specification, ``tests/ordinal_cases.py``
their float64 / int64 restatement.

Everything runs on the device on the caller's stream, with no host synchronisation inside and no CPU fallback; sensitivity,
specificity, PPV, NPV and net benefit are host arithmetic on the integer tallies after the one read.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .metrics import MAX_K, MAX_REPLICATES, MAX_ROWS, _f32, _require_cuda
from .selective import check_groups

AGREEMENT_NAMES = ("mae", "within_one", "under", "over", "kappa_linear", "kappa_quadratic")  # the columns of ``Agreement.stats``
MAX_TARGETS, MAX_FIXED = 8, 32  # PASN_ORDINAL_MAX_TARGETS (per kind), PASN_ORDINAL_MAX_FIXED
KINDS = ("specificity", "sensitivity", "youden")


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def check_targets(values, name: str, limit: int = MAX_TARGETS) -> List[float]:
    """A tuple of at most ``limit`` numbers in (0, 1) (it may be empty)."""
    try:
        vs = [float(v) for v in values]
    except TypeError:
        raise ValueError(f"{name} must be a sequence of numbers in (0, 1), got {values!r}") from None
    if len(vs) > limit or any(not 0.0 < v < 1.0 for v in vs):
        raise ValueError(f"{name} must be at most {limit} numbers in (0, 1), got {values!r}")
    return vs


def _check_rows(probs, labels, what: str):
    if probs.dim() != 2 or (labels is not None and labels.shape != probs.shape[:1]):
        raise ValueError("probs must be (M, K_real), labels (M,)")
    M, K = probs.shape
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"{what} takes 1 .. {MAX_ROWS} rows, got {M}")
    if not 2 <= K <= MAX_K:
        raise ValueError(f"{what} takes 2 .. {MAX_K} classes, got {K}")
    return M, K


def _check_B_seed(B, seed) -> None:
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or not 0 <= B <= MAX_REPLICATES:
        raise ValueError(f"B must be an integer in [0, {MAX_REPLICATES}], got {B!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")


def cut_names(K: int, class_labels: Optional[Sequence[str]] = None) -> List[str]:
    """The cuts' names: ``">= <label of grade c>"`` for c = 1 .. K - 1 (``class_labels``: the reference's list, in ascending severity)."""
    if class_labels is not None and len(class_labels) < K:
        raise ValueError(f"class_labels names {len(class_labels)} classes, the cuts need {K}")
    return [f">= {class_labels[c]}" if class_labels is not None else f">= {c}" for c in range(1, K)]


# ---- agreement ---------------------------------------------------------------------------------------------------------------------------
class Agreement:
    """Device results of ``agreement`` / ``agreement_of``: ``stats`` (R, 6) fp64 in the order of ``AGREEMENT_NAMES`` and ``cm`` (R, K, K)
    int64.  From ``Replicates.cm`` row ``R - 1`` is the point estimate, the rows before it the replicates."""

    def __init__(self, stats: torch.Tensor, cm: torch.Tensor):
        self.stats, self.cm = stats, cm

    @staticmethod
    def unpack(host) -> Dict[str, float]:
        """The LAST row of a host copy of ``stats`` as ``{name: value}`` (the point estimate)."""
        v = np.asarray(host, dtype=np.float64).reshape(-1, 6)[-1]
        return {n: float(x) for n, x in zip(AGREEMENT_NAMES, v)}

    def read(self) -> Dict[str, float]:
        """``{mae, within_one, under, over, kappa_linear, kappa_quadratic}`` of the last row: ONE synchronising read."""
        return self.unpack(self.stats[-1].cpu().numpy())


def agreement_of(cm: torch.Tensor) -> Agreement:
    """The six agreement statistics of confusion matrices ``cm`` (K, K) or (R, K, K) ``[true][pred]`` (any integer type), one launch.
    ``agreement_of(bootstrap.replicates(...).cm)`` gives every replicate and the point estimate on the bootstrap's own resamples."""
    _require_cuda(cm)
    if cm.dim() not in (2, 3) or cm.shape[-1] != cm.shape[-2] or cm.dtype.is_floating_point:
        raise ValueError("cm must be (K, K) or (R, K, K) integers")
    K = cm.shape[-1]
    if not 2 <= K <= MAX_K:
        raise ValueError(f"agreement_of takes 2 .. {MAX_K} classes, got {K}")
    cm = cm.reshape(-1, K, K).to(torch.int64).contiguous()
    R = cm.shape[0]
    if not 1 <= R <= MAX_REPLICATES + 1:
        raise ValueError(f"agreement_of takes 1 .. {MAX_REPLICATES + 1} matrices, got {R}")
    with torch.cuda.device(cm.device):
        stats = torch.empty(R, 6, dtype=torch.float64, device=cm.device)
        _lib.check(_lib.lib().pasn_ordinal_agreement(_lib.ptr(cm), R, K, _lib.ptr(stats), _lib.current_stream()))
    return Agreement(stats, cm)


def agreement(probs: torch.Tensor, labels: torch.Tensor) -> Agreement:
    """The agreement statistics of ``probs`` (M, K_real) fp32 against ``labels`` (M,) (< 0 or >= K_real: a padding row): the
    confusion matrix of the first-largest predictions, then ``agreement_of``.  No host synchronisation."""
    _require_cuda(probs, labels)
    M, K = _check_rows(probs, labels, "agreement")
    dev = probs.device
    with torch.cuda.device(dev):
        probs, labels = _f32(probs), labels.to(torch.int32).contiguous()
        cm = torch.empty(1, K, K, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().pasn_ordinal_confusion(_lib.ptr(probs), _lib.ptr(labels), M, K, _lib.ptr(cm), _lib.current_stream()))
    return agreement_of(cm)


def cut_scores(probs: torch.Tensor) -> torch.Tensor:
    """``(K_real - 1, M)`` fp32: row ``c - 1`` is the score of the cut ``grade >= c``, ``p[c] + p[c + 1] + ... + p[K_real - 1]`` added in
    that order in fp32 -- the numbers ``screen`` ranks and thresholds."""
    _require_cuda(probs)
    M, K = _check_rows(probs, None, "cut_scores")
    with torch.cuda.device(probs.device):
        probs = _f32(probs)
        out = torch.empty(K - 1, M, dtype=torch.float32, device=probs.device)
        _lib.check(_lib.lib().pasn_ordinal_cut_scores(_lib.ptr(probs), M, K, _lib.ptr(out), _lib.current_stream()))
    return out


# ---- cuts --------------------------------------------------------------------------------------------------------------------------------
class OperatingFit:
    """Thresholds fitted on one split, to be applied unchanged on another: ``thresholds`` (K - 1, T) fp32 on the device, column ``t`` as
    ``kinds[t]`` / ``targets[t]`` say -- the specificities, the sensitivities, then Youden's (target ``None``).  A cut that had no
    positive or no negative row on the fitting split holds NaN, which admits nobody."""

    def __init__(self, thresholds: torch.Tensor, specificities: Sequence[float], sensitivities: Sequence[float]):
        self.specificities, self.sensitivities = check_targets(specificities, "specificities"), check_targets(sensitivities, "sensitivities")
        self.kinds = ["specificity"] * len(self.specificities) + ["sensitivity"] * len(self.sensitivities) + ["youden"]
        self.targets = self.specificities + self.sensitivities + [None]
        if thresholds.dim() != 2 or thresholds.shape[1] != len(self.kinds) or not 1 <= thresholds.shape[0] <= MAX_K - 1:
            raise ValueError(f"thresholds must be (K - 1, {len(self.kinds)}), got {tuple(thresholds.shape)}")
        self.thresholds = thresholds
        self.K = int(thresholds.shape[0]) + 1

    @property
    def kind(self) -> List[str]:
        return list(self.kinds)

    def read(self) -> Dict[str, object]:
        """``{K, kinds, targets, thresholds (per cut)}``: ONE synchronising read."""
        return {"K": self.K, "kinds": list(self.kinds), "targets": list(self.targets), "thresholds": self.thresholds.cpu().tolist()}


def _op_names(specificities, sensitivities) -> List[str]:
    return [f"spec={t:g}" for t in specificities] + [f"sens={t:g}" for t in sensitivities] + ["youden"]


class Screening:
    """Device results of ``screen``; output row ``b < B`` is replicate ``b``, row ``B`` the point estimate; C = K - 1 cuts, T operating
    points per cut (the specificities, the sensitivities, Youden), F fixed thresholds per cut (a fit's, then ``net_benefit_at``):
    ``pn`` (B + 1, C, 2) int64 = P, N; ``u2`` (B + 1, C) int64; ``stats`` (B + 1, C, 2) fp64 = auc, ap; ``op_theta`` (B + 1, C, T) fp32;
    ``op_tally`` (B + 1, C, T, 2) and ``fix_tally`` (B + 1, C, F, 2) int64 = TP, FP."""

    def __init__(self, pn, u2, stats, op_theta, op_tally, fix_tally, K, B, G, seed, specificities, sensitivities, fit, net_benefit_at):
        self.pn, self.u2, self.stats, self.op_theta, self.op_tally, self.fix_tally = pn, u2, stats, op_theta, op_tally, fix_tally
        self.K, self.B, self.G, self.seed = K, B, G, seed
        self.specificities, self.sensitivities, self.fit, self.net_benefit_at = specificities, sensitivities, fit, net_benefit_at

    def packed(self) -> torch.Tensor:
        """One fp64 device vector: pn, u2, stats, op_theta, op_tally, fix_tally flattened in that order (every count is far below 2^53
        and a fp32 threshold widens exactly: fp64 carries them all)."""
        return torch.cat([t.double().flatten() for t in (self.pn, self.u2, self.stats, self.op_theta, self.op_tally, self.fix_tally)])

    @staticmethod
    def packed_size(K: int, B: int, T: int, F: int) -> int:
        return (B + 1) * (K - 1) * (2 + 1 + 2 + T + 2 * T + 2 * F)

    @staticmethod
    def split(host, K: int, B: int, T: int, F: int) -> Dict[str, np.ndarray]:
        """The arrays of ``packed()`` back in their shapes, from its host copy (tallies as int64)."""
        v = np.asarray(host, dtype=np.float64).reshape(-1)
        R, C = B + 1, K - 1
        if v.size != Screening.packed_size(K, B, T, F):
            raise ValueError(f"a packed screening of K={K}, B={B}, T={T}, F={F} holds {Screening.packed_size(K, B, T, F)} numbers, got {v.size}")
        out, o = {}, 0
        for name, shape, integer in (("pn", (R, C, 2), True), ("u2", (R, C), True), ("stats", (R, C, 2), False), ("op_theta", (R, C, T), False),
                                     ("op_tally", (R, C, T, 2), True), ("fix_tally", (R, C, F, 2), True)):
            n = int(np.prod(shape))
            a = v[o: o + n].reshape(shape)
            out[name] = a.astype(np.int64) if integer else a
            o += n
        return out

    @staticmethod
    def unpack(host, K: int, B: int = 0, specificities=(0.9,), sensitivities=(0.9,), fit: Optional[OperatingFit] = None,
               net_benefit_at=(), confidence: Optional[float] = None) -> Dict[str, object]:
        """The host reading of ``packed()``: ``{"cuts": [...]}``, one dict per cut with ``cut`` (c), ``P``, ``N``, ``prevalence``,
        ``auc``, ``ap``, ``u2``, ``operating_points`` (one ``{kind, target, theta, tp, fp, sensitivity, specificity, ppv, npv}`` per
        target and Youden's), with a fit ``fitted`` (the same per fitted threshold, applied) and with ``net_benefit_at`` ``net_benefit``
        (``{pt, net_benefit, treat_all}``, the threshold ``pt`` on the cut's score).  ``B > 0`` and a ``confidence`` add ``"ci"``:
        ``bootstrap.intervals_of`` of the columns ``replicate_columns`` names."""
        spec, sens = check_targets(specificities, "specificities"), check_targets(sensitivities, "sensitivities")
        pts = check_targets(net_benefit_at, "net_benefit_at", MAX_FIXED)
        T, nf = len(spec) + len(sens) + 1, 0 if fit is None else len(fit.kinds)
        a = Screening.split(host, K, B, T, nf + len(pts))
        kinds, targets = ["specificity"] * len(spec) + ["sensitivity"] * len(sens) + ["youden"], spec + sens + [None]
        cuts = []
        for c in range(K - 1):
            P, N = (int(x) for x in a["pn"][B, c])
            d = {"cut": c + 1, "P": P, "N": N, "prevalence": _ratio(P, P + N), "auc": float(a["stats"][B, c, 0]),
                 "ap": float(a["stats"][B, c, 1]), "u2": int(a["u2"][B, c]),
                 "operating_points": [_reading(kinds[t], targets[t], float(a["op_theta"][B, c, t]), a["op_tally"][B, c, t], P, N)
                                      for t in range(T)]}
            if fit is not None:
                d["fitted"] = [_reading(fit.kinds[t], fit.targets[t], None, a["fix_tally"][B, c, t], P, N) for t in range(nf)]
            if pts:
                d["net_benefit"] = [_net_benefit(pt, a["fix_tally"][B, c, nf + j], P, N) for j, pt in enumerate(pts)]
            cuts.append(d)
        res: Dict[str, object] = {"cuts": cuts}
        if B > 0 and confidence is not None:
            from .bootstrap import intervals_of

            names, cols = Screening.replicate_columns(a, K, spec, sens, fit)
            res["ci"] = intervals_of(cols, confidence, names=names)
        return res

    @staticmethod
    def replicate_columns(a: Dict[str, np.ndarray], K: int, specificities, sensitivities, fit: Optional[OperatingFit] = None):
        """``(names, (B + 1, n) fp64)``: per cut ``cut<c>/auc``, ``cut<c>/ap`` and the sensitivity and specificity of every operating
        point (``cut<c>/sens@spec=0.9`` ...) and of every applied fitted threshold (``cut<c>/fitted/sens@spec=0.9`` ...)."""
        names, cols = [], []
        P, N = a["pn"][..., 0].astype(np.float64), a["pn"][..., 1].astype(np.float64)
        ops = _op_names(specificities, sensitivities)
        with np.errstate(divide="ignore", invalid="ignore"):
            for c in range(K - 1):
                names += [f"cut{c + 1}/auc", f"cut{c + 1}/ap"]
                cols += [a["stats"][:, c, 0], a["stats"][:, c, 1]]
                groups = [("", a["op_tally"], ops)]
                if fit is not None:
                    groups.append(("fitted/", a["fix_tally"], _op_names(fit.specificities, fit.sensitivities)))
                for prefix, tally, tnames in groups:
                    for t, tn in enumerate(tnames):
                        names += [f"cut{c + 1}/{prefix}sens@{tn}", f"cut{c + 1}/{prefix}spec@{tn}"]
                        cols += [tally[:, c, t, 0] / P[:, c], (N[:, c] - tally[:, c, t, 1]) / N[:, c]]
        return names, np.stack(cols, axis=1)

    def read(self, confidence: float = 0.95) -> Dict[str, object]:
        """``unpack`` of this result: ONE synchronising read."""
        return self.unpack(self.packed().cpu().numpy(), self.K, self.B, self.specificities, self.sensitivities, self.fit, self.net_benefit_at,
                           confidence if self.B else None)


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def _reading(kind, target, theta, tally, P: int, N: int) -> Dict[str, object]:
    tp, fp = int(tally[0]), int(tally[1])
    fn, tn = P - tp, N - fp
    d = {"kind": kind, "target": target, "tp": tp, "fp": fp, "sensitivity": _ratio(tp, P), "specificity": _ratio(tn, N),
         "ppv": _ratio(tp, tp + fp), "npv": _ratio(tn, tn + fn)}
    if theta is not None:
        d["theta"] = theta
    return d


def _net_benefit(pt: float, tally, P: int, N: int) -> Dict[str, float]:
    n, odds = P + N, pt / (1.0 - pt)
    return {"pt": pt, "net_benefit": _ratio(int(tally[0]), n) - _ratio(int(tally[1]), n) * odds, "treat_all": _ratio(P, n) - _ratio(N, n) * odds}


def _check_screen_args(specificities, sensitivities, B, seed, fit, net_benefit_at, K: Optional[int] = None):
    spec, sens = check_targets(specificities, "specificities"), check_targets(sensitivities, "sensitivities")
    pts = check_targets(net_benefit_at, "net_benefit_at", MAX_FIXED)
    _check_B_seed(B, seed)
    if fit is not None and not isinstance(fit, OperatingFit):
        raise ValueError(f"fit must be an OperatingFit (fit_operating_points) or None, got {fit!r}")
    if fit is not None and K is not None and fit.K != K:
        raise ValueError(f"fit was made on {fit.K} classes, the rows have {K}")
    if (0 if fit is None else len(fit.kinds)) + len(pts) > MAX_FIXED:
        raise ValueError(f"fit and net_benefit_at together give more than {MAX_FIXED} fixed thresholds per cut")
    return spec, sens, pts


def screen(probs: torch.Tensor, labels: torch.Tensor, specificities=(0.9,), sensitivities=(0.9,), groups=None, B: int = 0, seed: int = 0,
           fit: Optional[OperatingFit] = None, net_benefit_at=()) -> Screening:
    """Every cut ``grade >= c`` of ``probs`` (M, K_real) fp32 against ``labels`` (M,) as a screening test: P, N, U2 / AUC, average
    precision, the operating points at the stated ``specificities`` and ``sensitivities`` and Youden's, the tallies at the thresholds
    of ``fit`` (an ``OperatingFit`` from another split) and at ``net_benefit_at`` (threshold probabilities ``pt``, read on the cut's
    score) -- for the sample and for ``B`` grouped-bootstrap replicates (``groups``, ``seed`` as in ``bootstrap.replicates``: the same
    resamples).  A fixed number of launches whatever ``B`` is; no host synchronisation."""
    _require_cuda(probs, labels)
    M, K = _check_rows(probs, labels, "screen")
    spec, sens, pts = _check_screen_args(specificities, sensitivities, B, seed, fit, net_benefit_at, K)
    dev = probs.device
    d_off = d_rows = None
    G = M
    if groups is not None:
        offsets, rows, G = check_groups(groups, M, exclusive=True)
        d_off, d_rows = torch.from_numpy(offsets).to(dev), torch.from_numpy(rows).to(dev)
    C, T, R = K - 1, len(spec) + len(sens) + 1, int(B) + 1
    lib = _lib.lib()
    with torch.cuda.device(dev):
        probs, labels = _f32(probs), labels.to(torch.int32).contiguous()
        parts = []
        if fit is not None:
            parts.append(fit.thresholds.to(device=dev, dtype=torch.float32))
        if pts:
            parts.append(torch.tensor(pts, dtype=torch.float32).to(dev).expand(C, len(pts)))
        fixed = torch.cat(parts, dim=1).contiguous() if parts else None
        F = 0 if fixed is None else fixed.shape[1]
        pn = torch.empty(R, C, 2, dtype=torch.int64, device=dev)
        u2 = torch.empty(R, C, dtype=torch.int64, device=dev)
        stats = torch.empty(R, C, 2, dtype=torch.float64, device=dev)
        op_theta = torch.empty(R, C, T, dtype=torch.float32, device=dev)
        op_tally = torch.empty(R, C, T, 2, dtype=torch.int64, device=dev)
        fix_tally = torch.empty(R, C, F, 2, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.pasn_ordinal_workspace_bytes(M, G, K, int(B)), dev)
        a_spec, a_sens = (ctypes.c_double * MAX_TARGETS)(*spec), (ctypes.c_double * MAX_TARGETS)(*sens)
        _lib.check(lib.pasn_ordinal_screen(_lib.ptr(probs), _lib.ptr(labels), _lib.ptr(d_off), _lib.ptr(d_rows), M, G, K, int(B), int(seed), a_spec,
                                           len(spec), a_sens, len(sens), _lib.ptr(fixed), F, _lib.ptr(pn), _lib.ptr(u2), _lib.ptr(stats),
                                           _lib.ptr(op_theta), _lib.ptr(op_tally), _lib.ptr(fix_tally) if F else None, _lib.ptr(ws),
                                           _lib.current_stream()))
    return Screening(pn, u2, stats, op_theta, op_tally, fix_tally, K, int(B), G, int(seed), spec, sens, fit, pts)


def fit_operating_points(probs: torch.Tensor, labels: torch.Tensor, specificities=(0.9,), sensitivities=(0.9,)) -> OperatingFit:
    """The thresholds of ``screen``'s operating points on these rows (the sample, no replicates), kept on the device: fit on ``val``,
    hand the result to ``screen(..., fit=)`` on ``test``.  No host synchronisation."""
    s = screen(probs, labels, specificities, sensitivities)
    return OperatingFit(s.op_theta[0], s.specificities, s.sensitivities)


def intervals(res, confidence: float = 0.95) -> Dict[str, Dict[str, float]]:
    """``bootstrap.intervals_of`` with this module's column names: of an ``Agreement`` made from ``Replicates.cm`` (the six
    ``AGREEMENT_NAMES``), or of a ``Screening`` with ``B > 0`` (``Screening.replicate_columns``).  ONE synchronising read."""
    from .bootstrap import check_confidence, intervals_of

    check_confidence(confidence)
    if isinstance(res, Agreement):
        return intervals_of(res.stats.cpu().numpy(), confidence, names=AGREEMENT_NAMES)
    if not isinstance(res, Screening) or res.B < 1:
        raise ValueError("intervals takes an Agreement of replicates or a Screening with B >= 1")
    T, F = res.op_theta.shape[2], res.fix_tally.shape[2]
    a = Screening.split(res.packed().cpu().numpy(), res.K, res.B, T, F)
    names, cols = Screening.replicate_columns(a, res.K, res.specificities, res.sensitivities, res.fit)
    return intervals_of(cols, confidence, names=names)
