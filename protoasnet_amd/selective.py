"""Selective prediction: what the abstention output is for (``csrc/selective.hip``).

ProtoASNet's abstention class gives every clip a learned uncertainty ``alpha`` (``src/loss/loss.py:323-371``); the model is judged by how
much its accuracy rises as the uncertain clips are set aside.  The reference trains that output and has no code that evaluates it, so the
definitions below ("Selective prediction"; ``include/protoasnet_amd.h``) are the specification:

* ``uncertainty(logits, abstain_class, score, ab_logitpath)``: one score per row -- ``maxprob`` = 1 - the largest real-class probability,
  ``alpha`` = the abstention column of the joined softmax (``loss.py:356``) or the sigmoid of the abstention logit (``loss.py:358``).
* ``build_groups(keys)`` / ``group_predictions(probs, u, labels, groups)``: one prediction per cine from its clips' rows -- the plain mean
  ``p_mean``, the confidence-weighted mean ``p_conf`` (weights ``1 - u``) and the mean uncertainty ``u_mean``, fp64 sums in row order.
* ``risk_coverage(probs, labels, u)``: the rows ordered by ascending uncertainty (ties: the lower index; NaN last) and, for every prefix
  of that order, the accuracy, balanced accuracy and mean F1 of ``trainer.confusion_to_metrics``; ``aurc`` is the mean error over all
  prefixes (the area under the risk-coverage curve), ``error_auroc`` the AUROC of ``u`` as a detector of the wrong predictions.
* ``SelectiveEvaluator``: an ``EpochEvaluator(keep_logits=True)`` fed batch by batch together with the clips' file names; ``finish`` gives
  the curve read at a few coverages, per clip or per cine, with ONE synchronising device-to-host copy; ``finish(bootstrap=B)`` adds
  grouped-bootstrap confidence intervals (``bootstrap.py``) to the same read, ``finish(calibration=n_bins, temperature=...)`` reliability
  bins, ECE and temperature-scaled probabilities (``calibration.py``), ``finish(conformal=fit)`` conformal prediction sets
  (``conformal.py``).

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

import csv
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .metrics import MAX_ROWS, EpochEvaluator, _f32, _require_cuda, roc_auc_ovr_weighted

MAXPROB, ALPHA_JOINED, ALPHA_SEPARATE = 0, 1, 2  # the modes of pasn_uncertainty_scores
DEFAULT_COVERAGES = (1.0, 0.9, 0.8, 0.7, 0.5)


def score_mode(abstain_class: bool, score: str = "auto", ab_logitpath: str = "joined") -> int:
    """The kernel mode of a score name: ``auto`` is ``alpha`` with an abstention class and ``maxprob`` without one."""
    if score not in ("auto", "maxprob", "alpha"):
        raise ValueError(f"score must be 'auto', 'maxprob' or 'alpha', got {score!r}")
    if ab_logitpath not in ("joined", "separate"):
        raise ValueError(f"ab_logitpath must be 'joined' or 'separate', got {ab_logitpath!r}")
    if score == "auto":
        score = "alpha" if abstain_class else "maxprob"
    if score == "maxprob":
        return MAXPROB
    if not abstain_class:
        raise ValueError("score='alpha' needs a model with an abstention class")
    return ALPHA_JOINED if ab_logitpath == "joined" else ALPHA_SEPARATE


def uncertainty(logits: torch.Tensor, abstain_class: bool, score: str = "auto", ab_logitpath: str = "joined") -> torch.Tensor:
    """(M,) fp32 uncertainty of the rows of ``logits`` (M, K); the last column is the abstention logit when ``abstain_class``."""
    mode = score_mode(abstain_class, score, ab_logitpath)
    _require_cuda(logits)
    if logits.dim() != 2:
        raise ValueError("logits must be (M, K)")
    M, K = logits.shape
    u = torch.empty(M, dtype=torch.float32, device=logits.device)
    if M > 0:
        _lib.check(_lib.lib().pasn_uncertainty_scores(_lib.ptr(_f32(logits)), M, K, K - 1 if abstain_class else K, mode, _lib.ptr(u),
                                                      _lib.current_stream()))
    return u


# ---- groups: one prediction per cine ---------------------------------------------------------------------------------------------------
def build_groups(keys: Sequence) -> Tuple[np.ndarray, np.ndarray, list]:
    """CSR groups of the rows that share a key (host only): ``(offsets int64 (G + 1,), rows int32 (M,), names)``.  Groups come in order of
    first appearance, a group's rows ascending; equal keys need not be neighbours."""
    index: Dict[object, int] = {}
    members: List[List[int]] = []
    for i, k in enumerate(keys):
        g = index.setdefault(k, len(members))
        if g == len(members):
            members.append([])
        members[g].append(i)
    offsets = np.zeros(len(members) + 1, dtype=np.int64)
    np.cumsum([len(m) for m in members], out=offsets[1:])
    rows = np.fromiter((i for m in members for i in m), dtype=np.int32, count=int(offsets[-1]))
    return offsets, rows, list(index)


def check_groups(groups, M: int, exclusive: bool = False) -> Tuple[np.ndarray, np.ndarray, int]:
    """``build_groups``' tuple (or its first two arrays) checked on the host against ``M`` rows -- the kernels do not check, and these
    indices address device memory.  Returns the contiguous ``(offsets int64, rows int32, G)``.  ``exclusive=True``: the groups are
    resampling units (``bootstrap.py``, ``calibration.py``), so no more groups than rows and a row in one group only."""
    offsets = np.ascontiguousarray(groups[0], dtype=np.int64)
    rows = np.ascontiguousarray(groups[1], dtype=np.int32)
    G = offsets.size - 1
    if G < 1 or offsets[0] != 0 or offsets[-1] != rows.size or (np.diff(offsets) < 0).any():
        raise ValueError("group offsets must start at 0, not decrease and end at the number of listed rows")
    if exclusive and G > M:
        raise ValueError(f"{G} groups for {M} rows")
    if rows.size and (rows.min() < 0 or rows.max() >= M):
        raise ValueError(f"group rows must lie in [0, {M})")
    if exclusive and rows.size and np.bincount(rows, minlength=M).max() > 1:
        raise ValueError("a row may be listed in one group only")
    if exclusive and G * int(np.diff(offsets).max()) >= 1 << 31:  # the expanded rows of a replicate are counted in 32 bits
        raise ValueError("G times the largest group must stay below 2^31")
    return offsets, rows, G


class GroupPredictions:
    """Device results of ``group_predictions``: ``p_mean`` / ``p_conf`` (G, K_real) fp64, ``u_mean`` (G,) fp64, ``labels`` / ``counts``
    (G,) int32, ``status`` (2,) int32 = {groups whose rows disagree on the label, rows holding a NaN}."""

    def __init__(self, p_mean, p_conf, u_mean, labels, counts, status):
        self.p_mean, self.p_conf, self.u_mean, self.labels, self.counts, self.status = p_mean, p_conf, u_mean, labels, counts, status

    def check(self) -> "GroupPredictions":
        """Reads the status words (a host synchronisation): ``ValueError`` when a group's rows disagree on the label."""
        _raise_on_conflict(int(self.status[0].item()))
        return self


def _raise_on_conflict(n: int) -> None:
    if n > 0:
        raise ValueError(f"{n} group(s) hold rows with different labels: the rows of one cine must share its label")


def group_predictions(probs: torch.Tensor, u: torch.Tensor, labels: torch.Tensor, groups, check: bool = True) -> GroupPredictions:
    """One prediction per group of rows; ``groups`` is ``build_groups``' tuple (or its first two arrays).  ``check=True`` reads the status
    and raises ``ValueError`` on a label conflict; ``check=False`` returns without a host synchronisation (``.check()`` later)."""
    _require_cuda(probs, u, labels)
    if probs.dim() != 2 or u.shape != probs.shape[:1] or labels.shape != probs.shape[:1]:
        raise ValueError("probs must be (M, K_real), u and labels (M,)")
    M, K_real = probs.shape
    offsets, rows, G = check_groups(groups, M)
    dev = probs.device
    d_off, d_rows = torch.from_numpy(offsets).to(dev), torch.from_numpy(rows).to(dev)
    p_mean, p_conf = torch.empty(G, K_real, dtype=torch.float64, device=dev), torch.empty(G, K_real, dtype=torch.float64, device=dev)
    u_mean = torch.empty(G, dtype=torch.float64, device=dev)
    g_label, g_count = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pasn_group_predictions(
        _lib.ptr(_f32(probs)), _lib.ptr(_f32(u)), _lib.ptr(labels.to(torch.int32).contiguous()), _lib.ptr(d_off), _lib.ptr(d_rows), G, K_real,
        _lib.ptr(p_mean), _lib.ptr(p_conf), _lib.ptr(u_mean), _lib.ptr(g_label), _lib.ptr(g_count), _lib.ptr(status), _lib.current_stream()))
    res = GroupPredictions(p_mean, p_conf, u_mean, g_label, g_count, status)
    return res.check() if check else res


# ---- risk-coverage -----------------------------------------------------------------------------------------------------------------------
def coverage_rows(coverages: Sequence[float], Mv):
    """The number of rows ``m`` kept at each coverage ``c``: ``ceil(c * Mv)``, at least one row and at most ``Mv``.  ``c * Mv`` is an fp64
    product, so 1e-9 of a row is taken off before the ceiling (0.7 * 10 is 7.000000000000001, and means 7).  Works on numpy values and
    on device tensors alike (``Mv`` a 0-d tensor): the host and the device take the same IEEE steps."""
    if isinstance(Mv, torch.Tensor):
        c = torch.as_tensor(list(coverages), dtype=torch.float64, device=Mv.device)
        return torch.minimum(torch.ceil(c * Mv.double() - 1e-9).clamp(min=1.0), Mv.double().clamp(min=1.0)).to(torch.int64)
    c = np.asarray(list(coverages), dtype=np.float64)
    return np.minimum(np.maximum(np.ceil(c * np.float64(Mv) - 1e-9), 1.0), max(float(Mv), 1.0)).astype(np.int64)


def _check_coverages(coverages) -> List[float]:
    cs = [float(c) for c in coverages]
    if not cs or any(not (0.0 < c <= 1.0) for c in cs):
        raise ValueError(f"coverages must lie in (0, 1], got {list(coverages)}")
    return cs


class RiskCoverage:
    """The device curves of ``risk_coverage``: ``order`` (M,) int32, ``acc`` / ``bal_acc`` / ``f1_mean`` (M,) fp64, ``threshold`` (M,)
    fp32 -- entries at and past ``counts[0]`` (the valid rows, Mv) are unwritten --, ``aurc`` (1,) fp64, ``counts`` (2,) int64 = {Mv, rows
    whose uncertainty is NaN}, and ``error_auroc`` (0-d fp64; NaN when every row is right, every row is wrong, or a ``u`` is NaN)."""

    def __init__(self, order, acc, bal_acc, f1_mean, threshold, aurc, counts, error_auroc):
        self.order, self.acc, self.bal_acc, self.f1_mean, self.threshold = order, acc, bal_acc, f1_mean, threshold
        self.aurc, self.counts, self.error_auroc = aurc, counts, error_auroc

    def packed(self, coverages) -> torch.Tensor:
        """fp64 device vector [acc, bal_acc, f1_mean, threshold, rows kept (one each per coverage), aurc, error_auroc, Mv, NaN rows]."""
        n = coverage_rows(coverages, self.counts[0])
        i = (n - 1).clamp(min=0)
        return torch.cat([self.acc[i], self.bal_acc[i], self.f1_mean[i], self.threshold[i].double(), n.double(), self.aurc,
                          self.error_auroc.reshape(1), self.counts.double()])

    @staticmethod
    def unpack(host: torch.Tensor, coverages) -> Dict[str, object]:
        nc = len(coverages)
        v = host.tolist()
        Mv = int(v[5 * nc + 2])
        nan = float("nan")
        cut = (lambda a: a) if Mv > 0 else (lambda a: [nan] * nc)  # no valid row: the curve is empty
        return {"coverage": list(coverages), "accuracy": cut(v[:nc]), "bal_accuracy": cut(v[nc: 2 * nc]), "f1_mean": cut(v[2 * nc: 3 * nc]),
                "threshold": cut(v[3 * nc: 4 * nc]), "rows": [int(x) if Mv > 0 else 0 for x in v[4 * nc: 5 * nc]], "aurc": v[5 * nc],
                "error_auroc": v[5 * nc + 1], "valid_rows": Mv, "nan_rows": int(v[5 * nc + 3])}

    def at(self, coverages) -> Dict[str, object]:
        """The curve read at row ``m = coverage_rows(c, Mv)`` for each coverage, with ``aurc`` and ``error_auroc``: ONE device-to-host
        copy.  ``{coverage, accuracy, bal_accuracy, f1_mean, threshold, rows (lists), aurc, error_auroc, valid_rows, nan_rows}``."""
        cs = _check_coverages(coverages)
        return self.unpack(self.packed(cs).cpu(), cs)


def first_largest(probs: torch.Tensor) -> torch.Tensor:
    """The index of the first largest entry of each row (``argmax`` does not promise the first on the device)."""
    return ((probs == probs.amax(dim=1, keepdim=True)).cumsum(dim=1) == 0).sum(dim=1)


def risk_coverage(probs: torch.Tensor, labels: torch.Tensor, u: torch.Tensor) -> RiskCoverage:
    """The risk-coverage curves of ``probs`` (M, K_real) fp32, ``labels`` (M,) (< 0: a padding row, ignored) and ``u`` (M,) fp32.  No host
    synchronisation."""
    _require_cuda(probs, labels, u)
    if probs.dim() != 2 or labels.shape != probs.shape[:1] or u.shape != probs.shape[:1]:
        raise ValueError("probs must be (M, K_real), labels and u (M,)")
    M, K_real = probs.shape
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"risk_coverage takes 1 .. {MAX_ROWS} rows, got {M}")
    dev = probs.device
    probs, u, labels = _f32(probs), _f32(u), labels.to(torch.int32).contiguous()
    order = torch.empty(M, dtype=torch.int32, device=dev)
    curves = torch.empty(3, M, dtype=torch.float64, device=dev)
    threshold = torch.empty(M, dtype=torch.float32, device=dev)
    aurc = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ws = _lib.workspace(_lib.lib().pasn_risk_coverage_workspace_bytes(M, K_real), dev)
    _lib.check(_lib.lib().pasn_risk_coverage(_lib.ptr(probs), _lib.ptr(labels), _lib.ptr(u), M, K_real, _lib.ptr(order), _lib.ptr(curves[0]),
                                             _lib.ptr(curves[1]), _lib.ptr(curves[2]), _lib.ptr(threshold), _lib.ptr(aurc), _lib.ptr(counts),
                                             _lib.ptr(ws), _lib.current_stream()))
    # u as a detector of the wrong predictions: the binary AUC of the scores [1 - u, u] against the wrong (1) / right (0) flag
    valid = (labels >= 0) & (labels < K_real)
    wrong = torch.where(valid, (first_largest(probs) != labels).to(torch.int32), torch.full_like(labels, -1))
    _, per = roc_auc_ovr_weighted(torch.stack([1.0 - u, u], dim=1), wrong, 2, per_class=True)
    return RiskCoverage(order, curves[0], curves[1], curves[2], threshold, aurc, counts, per[1])


# ---- the evaluator -----------------------------------------------------------------------------------------------------------------------
class SelectiveEvaluator:
    """Selective-prediction metrics of one sweep of ``model`` (the surface ``EpochEvaluator`` reads).

    ``update(logits, sim, target, keys)``: one ``EpochEvaluator.update`` (its launch, no host synchronisation); ``keys`` are the rows'
    group names -- the clips' file names -- kept on the host.  ``finish(coverages, level)``: ``level="clip"`` scores every row with
    ``uncertainty(...)``; ``level="cine"`` first reduces the rows of each key to one prediction (``p_conf``, uncertainty ``u_mean``) and
    scores those.  Returns ``{aurc, error_auroc, accuracy@c, bal_accuracy@c, f1_mean@c, threshold@c (c as in "0.9"), rows, nan_rows}`` and
    at cine level also ``groups``, the confusion metrics ``accuracy`` / ``f1`` / ``f1_mean`` and ``auc`` / ``auc_per_class`` of the cine
    predictions, and ``cines``: one ``{filename, target_AS, n_clips, probs, uncertainty, pred}`` per cine.  One synchronising read."""

    def __init__(self, model, abstain_class: bool, score: str = "auto", ab_logitpath: str = "joined", capacity: int = 0):
        self.abstain, self.score, self.ab_logitpath = bool(abstain_class), score, ab_logitpath
        score_mode(self.abstain, score, ab_logitpath)  # a bad name fails here, not after the sweep
        self.ev = EpochEvaluator(model, keep_logits=True, abstain_class=self.abstain, capacity=capacity)
        self.keys: list = []

    def update(self, logits: torch.Tensor, sim: torch.Tensor, target: torch.Tensor, keys: Sequence) -> None:
        keys = list(keys)
        if len(keys) != logits.shape[0]:
            raise ValueError(f"{len(keys)} keys for {logits.shape[0]} rows")
        self.ev.update(logits, sim, target)
        self.keys += keys

    def finish(self, coverages=DEFAULT_COVERAGES, level: str = "clip", bootstrap: int = 0, seed: int = 0, confidence: float = 0.95,
               unit: str = "cine", calibration: int = 0, temperature=None, ordinal=None, ordinal_net_benefit_at=(), conformal=None,
               conformal_mondrian: bool = False) -> Dict[str, object]:
        """``bootstrap=B > 0`` adds ``res["ci"]``: ``bootstrap.intervals`` of ``B`` grouped replicates (``seed``, ``confidence``) of the
        rows the level scores -- at cine level the cine predictions, the unit the cine; at clip level the clips, the unit the cine
        (``build_groups`` of the keys) or, with ``unit="clip"``, the clip.  Still one synchronising read; ``bootstrap=0`` is the call
        without it, launch for launch.

        ``temperature`` (a ``calibration.TemperatureFit`` or a float ``T > 0``): the class probabilities scored everywhere in the call
        are ``calibration.scaled_probs`` of the kept logits, and the ``maxprob`` uncertainty follows them (it is 1 - the largest scored
        probability by definition); the ``alpha`` modes keep reading the raw logits.  ``calibration=n_bins > 0`` adds
        ``res["calibration"]``: ``calibration.reliability(...).summary()`` of the level's rows (the clips; at cine level ``p_conf`` with
        the cine's label), and under ``["selective"]`` the same with ``conf = 1 - u`` -- is the uncertainty an honest probability of
        error? -- (``ece``, ``mce``, ``conf_gap``, ``bins``); with ``bootstrap=B`` ``res["ci"]`` gains the six calibration statistics, from
        the same seed and units and therefore the same resamples.  Still one read; the defaults are the call without either.

        ``conformal`` (a ``conformal.ConformalFit``) adds ``res["conformal"]``: ``{kind, mondrian, alphas, qhat, qhat_per_class,
        levels}``, ``levels`` one ``ConformalSets.summary()`` dict per alpha of ``conformal.predict_sets`` on the rows the level scores
        (the clips; at cine level ``p_conf.float()`` with the cine's label and ``u_mean``), after ``temperature`` if one is given;
        ``conformal_mondrian`` takes each class's own threshold.  At cine level every entry of ``res["cines"]`` gains
        ``"set@<alpha>"``, the list of class indices.  The same single read; ``conformal=None`` is the call without it.

        ``ordinal`` (``True``, or an ``ordinal.OperatingFit`` from another split) adds ``res["ordinal"]``: ``{"agreement": {mae,
        within_one, under, over, kappa_linear, kappa_quadratic}, "cuts": [...]}``, ``cuts`` being ``ordinal.Screening.unpack``'s list
        (per cut ``grade >= c``: ``P``, ``N``, ``prevalence``, ``auc``, ``ap`` and the operating points with their sensitivity,
        specificity, PPV, NPV and threshold) of the rows the level scores (the clips; at cine level ``p_conf.float()`` with the cine's
        label), after ``temperature`` if one is given.  ``True`` reports the operating points at specificity 0.9, sensitivity 0.9 and
        Youden's; a fit reports those of its own targets and, under ``"fitted"``, its thresholds applied unchanged;
        ``ordinal_net_benefit_at`` (threshold probabilities) adds ``"net_benefit"``.  With ``bootstrap=B`` the six agreement
        statistics and each cut's ``auc``, ``ap`` and every reported sensitivity / specificity join ``res["ci"]``, on the same
        resamples.  The same single read; ``ordinal=None`` is the call without it."""
        if level not in ("clip", "cine"):
            raise ValueError(f"level must be 'clip' or 'cine', got {level!r}")
        if unit not in ("clip", "cine"):
            raise ValueError(f"unit must be 'clip' or 'cine', got {unit!r}")
        if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) or bootstrap < 0:
            raise ValueError(f"bootstrap must be a non-negative integer, got {bootstrap!r}")
        boot = None
        if bootstrap:
            from . import bootstrap as boot

            boot.check_confidence(confidence)
            boot._check_B_seed(bootstrap, seed)
        if isinstance(calibration, bool) or not isinstance(calibration, (int, np.integer)) or calibration < 0:
            raise ValueError(f"calibration must be a non-negative integer (the number of bins), got {calibration!r}")
        cal = None
        if calibration or temperature is not None:
            from . import calibration as cal

            if calibration:
                cal.check_bins(calibration)
            if temperature is not None:
                cal._check_temperature(temperature)
        n_bins = int(calibration)
        conf = None
        if conformal is not None:
            from . import conformal as conf

            if not isinstance(conformal, conf.ConformalFit):
                raise ValueError(f"conformal must be a ConformalFit (conformal.calibrate) or None, got {conformal!r}")
            if not isinstance(conformal_mondrian, (bool, np.bool_)):
                raise ValueError(f"conformal_mondrian must be a bool, got {conformal_mondrian!r}")
        ordm = None
        if ordinal is not None:
            from . import ordinal as ordm

            if ordinal is not True and not isinstance(ordinal, ordm.OperatingFit):
                raise ValueError(f"ordinal must be True, an OperatingFit (ordinal.fit_operating_points) or None, got {ordinal!r}")
            ord_fit = None if ordinal is True else ordinal
            ord_spec, ord_sens = ((0.9,), (0.9,)) if ord_fit is None else (ord_fit.specificities, ord_fit.sensitivities)
            ord_spec, ord_sens, ord_pts = ordm._check_screen_args(ord_spec, ord_sens, int(bootstrap), 0, ord_fit, ordinal_net_benefit_at)
        cs = _check_coverages(coverages)
        ev, K = self.ev, self.ev.K_real
        if ev.rows == 0:
            raise ValueError("no rows: call update() first")
        if conf is not None and conformal.K != K:
            raise ValueError(f"the conformal fit was calibrated on {conformal.K} classes, the evaluator scores {K}")
        if ordm is not None and ord_fit is not None and ord_fit.K != K:
            raise ValueError(f"the operating points were fitted on {ord_fit.K} classes, the evaluator scores {K}")
        probs, labels = ev.probs[: ev.rows], ev.labels[: ev.rows]
        if temperature is None:
            u = uncertainty(ev.logits[: ev.rows], self.abstain, self.score, self.ab_logitpath)
        elif score_mode(self.abstain, self.score, self.ab_logitpath) == MAXPROB:
            probs, u = cal.scaled_probs(ev.logits[: ev.rows], K, temperature, with_u=True)
        else:
            probs = cal.scaled_probs(ev.logits[: ev.rows], K, temperature)
            u = uncertainty(ev.logits[: ev.rows], self.abstain, self.score, self.ab_logitpath)
        if level == "clip":
            packed = risk_coverage(probs, labels, u).packed(cs)
            if boot is None and not n_bins and conf is None and ordm is None:
                return self._result(RiskCoverage.unpack(packed.cpu(), cs))
            groups = build_groups(self.keys)[:2] if bootstrap and unit == "cine" else None
            parts = [packed]
            rep = None
            if boot is not None:
                rep = boot.replicates(probs, labels, u, groups, bootstrap, seed)
                parts.append(rep.stats.flatten())
            if n_bins:
                parts += self._calibration_parts(cal, probs, labels, u, groups, n_bins, bootstrap, seed)
            if conf is not None:
                parts += self._conformal_parts(conf, conformal, probs, labels, u, conformal_mondrian, masks=False)
            if ordm is not None:
                parts += self._ordinal_parts(ordm, rep, probs, labels, groups, bootstrap, seed, ord_spec, ord_sens, ord_fit, ord_pts)
            host = torch.cat(parts).cpu()  # the one read
            res = self._result(RiskCoverage.unpack(host[: packed.numel()], cs))
            ord_ci = None
            if ordm is not None:
                host, ord_ci = self._add_ordinal(res, host, ordm, K, bootstrap, ord_spec, ord_sens, ord_fit, ord_pts, confidence)
            if conf is not None:
                host = self._add_conformal(res, host, conf, conformal, conformal_mondrian, None)
            self._add_intervals(res, host[packed.numel():], boot, cal, n_bins, bootstrap, confidence)
            if ord_ci:
                res["ci"].update(ord_ci)
            return res
        offsets, rows, names = build_groups(self.keys)
        G = len(names)
        gp = group_predictions(probs, u, labels, (offsets, rows), check=False)
        p, gl = gp.p_conf.float(), gp.labels
        pred = first_largest(p)
        cm = torch.bincount(gl.long().clamp(0, K - 1) * K + pred.clamp(max=K - 1), minlength=K * K)
        auc, auc_k = roc_auc_ovr_weighted(p, gl, K, per_class=True)
        rc = risk_coverage(p, gl, gp.u_mean.float())
        tail = [gp.status.double(), cm.double(), auc.reshape(1), auc_k, gp.p_conf.flatten(), gp.u_mean, gl.double(), gp.counts.double(), pred.double()]
        rep = None
        if boot is not None:  # the rows are the cine predictions: every row is its own unit
            rep = boot.replicates(p, gl, gp.u_mean.float(), None, bootstrap, seed)
            tail.append(rep.stats.flatten())
        if n_bins:
            tail += self._calibration_parts(cal, p, gl, gp.u_mean.float(), None, n_bins, bootstrap, seed)
        if conf is not None:
            tail += self._conformal_parts(conf, conformal, p, gl, gp.u_mean.float(), conformal_mondrian, masks=True)
        if ordm is not None:
            tail += self._ordinal_parts(ordm, rep, p, gl, None, bootstrap, seed, ord_spec, ord_sens, ord_fit, ord_pts)
        host = torch.cat([rc.packed(cs)] + tail).cpu()  # the one read
        n_rc = 5 * len(cs) + 4
        res = self._result(RiskCoverage.unpack(host[:n_rc], cs))
        ord_ci = None
        if ordm is not None:
            host, ord_ci = self._add_ordinal(res, host, ordm, K, bootstrap, ord_spec, ord_sens, ord_fit, ord_pts, confidence)
        masks = None
        if conf is not None:
            masks = host[host.numel() - len(conformal.alphas) * G:].view(len(conformal.alphas), G).long().tolist()
            host = self._add_conformal(res, host, conf, conformal, conformal_mondrian, G)
        t = host[n_rc:]
        _raise_on_conflict(int(t[0]))
        from .trainer import confusion_to_metrics

        res.update(confusion_to_metrics(t[2: 2 + K * K].view(K, K)))
        o = 2 + K * K
        res.update({"groups": G, "nan_clip_rows": int(t[1]), "auc": float(t[o]), "auc_per_class": t[o + 1: o + 1 + K].tolist()})
        o += 1 + K
        pc = t[o: o + G * K].view(G, K).tolist()  # whole columns at once: per-element reads of a tensor would dominate the call
        um, lab, cnt, prd = (t[o + G * K + j * G: o + G * K + (j + 1) * G] for j in range(4))
        res["cines"] = [{"filename": n, "target_AS": l, "n_clips": c, "probs": p, "uncertainty": x, "pred": d}
                        for n, l, c, p, x, d in zip(names, lab.long().tolist(), cnt.long().tolist(), pc, um.tolist(), prd.long().tolist())]
        if masks is not None:
            for alpha, row in zip(conformal.alphas, masks):
                for c, m in zip(res["cines"], row):
                    c[f"set@{alpha:g}"] = conf.mask_classes(m, K)
        self._add_intervals(res, t[o + G * K + 4 * G:], boot, cal, n_bins, bootstrap, confidence)
        if ord_ci:
            res["ci"].update(ord_ci)
        return res

    @staticmethod
    def _ordinal_parts(ordm, rep, probs, labels, groups, B: int, seed: int, spec, sens, fit, pts) -> List[torch.Tensor]:
        """The device vectors ``ordinal=`` adds at the very END of the one read: the agreement statistics (of every replicate's
        confusion matrix when the bootstrap ran: ``rep`` is its ``Replicates``) and the packed screening, on the same resamples."""
        agr = ordm.agreement_of(rep.cm) if rep is not None else ordm.agreement(probs, labels)
        scr = ordm.screen(probs, labels, spec, sens, groups, int(B), int(seed), fit, pts)
        return [agr.stats.flatten(), scr.packed()]

    @staticmethod
    def _add_ordinal(res, host, ordm, K: int, B: int, spec, sens, fit, pts, confidence: float):
        """Reads ``_ordinal_parts`` off the end of ``host``, adds ``res["ordinal"]`` and returns ``host`` without them and the
        intervals that join ``res["ci"]`` (None without a bootstrap)."""
        T, F = len(spec) + len(sens) + 1, (0 if fit is None else len(fit.kinds)) + len(pts)
        n_s, n_a = ordm.Screening.packed_size(K, B, T, F), (B + 1 if B else 1) * 6
        cut = host.numel() - n_s - n_a
        agr = host[cut: cut + n_a].numpy().reshape(-1, 6)
        scr = ordm.Screening.unpack(host[cut + n_a:].numpy(), K, B, spec, sens, fit, pts, confidence if B else None)
        res["ordinal"] = {"agreement": ordm.Agreement.unpack(agr), "cuts": scr["cuts"]}
        ci = None
        if B:
            from .bootstrap import intervals_of

            ci = intervals_of(agr, confidence, names=ordm.AGREEMENT_NAMES)
            ci.update(scr["ci"])
        return host[:cut], ci

    @staticmethod
    def _conformal_parts(conf, fit, probs, labels, u, mondrian: bool, masks: bool) -> List[torch.Tensor]:
        """The device vectors ``conformal=fit`` adds at the END of the one read: the tallies, the thresholds and, at cine level, the
        masks (every count is far below 2^53: fp64 carries it exactly)."""
        sets = conf.predict_sets(probs, fit, labels, u, bool(mondrian))
        parts = [sets.packed().double(), fit.qhat.double().flatten()]
        if masks:  # (uint16 words through their int16 view: K_real = 16 may set bit 15)
            parts.append((sets.masks.view(torch.int16).to(torch.int32) & 0xFFFF).double().flatten())
        return parts

    @staticmethod
    def _add_conformal(res, host, conf, fit, mondrian: bool, G):
        """Reads ``_conformal_parts`` off the end of ``host``, adds ``res["conformal"]`` and returns ``host`` without them."""
        K, A = fit.K, len(fit.alphas)
        n_t, n_q, n_m = A * conf.tally_words(K), (K + 1) * A, A * G if G is not None else 0
        cut = host.numel() - n_t - n_q - n_m
        q = host[cut + n_t: cut + n_t + n_q].view(K + 1, A)
        res["conformal"] = {"kind": fit.kind, "mondrian": bool(mondrian), "alphas": list(fit.alphas), "qhat": q[0].tolist(),
                            "qhat_per_class": q[1:].tolist(),
                            "levels": conf.ConformalSets.unpack(host[cut: cut + n_t].numpy(), fit.alphas, K)}
        return host[:cut]

    @staticmethod
    def _calibration_parts(cal, probs, labels, u, groups, n_bins: int, B: int, seed: int) -> List[torch.Tensor]:
        """The device vectors ``calibration=n_bins`` adds to the one read: the summary of the class probabilities, the summary of
        ``1 - u`` as a claimed probability of being right, and with ``B`` replicates their statistics."""
        rel = cal.reliability(probs, labels, n_bins, None, groups, B, seed)
        parts = [rel.packed(), cal.reliability(probs, labels, n_bins, 1.0 - u).packed()]
        return parts + [rel.stats.flatten()] if B else parts

    @staticmethod
    def _add_intervals(res, host, boot, cal, n_bins: int, B: int, confidence: float) -> None:
        """``host``: what followed the level's own numbers in the read -- the bootstrap's replicates, then ``_calibration_parts``."""
        if boot is not None:
            res["ci"] = boot.intervals_of(host[: (B + 1) * 6].view(B + 1, 6).numpy(), confidence)
            host = host[(B + 1) * 6:]
        if n_bins:
            w = 7 + 3 * n_bins
            res["calibration"] = cal.Reliability.unpack(host[:w], n_bins)
            sel = cal.Reliability.unpack(host[w: 2 * w], n_bins)
            res["calibration"]["selective"] = {k: sel[k] for k in ("ece", "mce", "conf_gap", "bins")}
            if boot is not None:
                res["ci"].update(boot.intervals_of(host[2 * w:].view(B + 1, 6).numpy(), confidence, names=cal.STAT_NAMES))

    @staticmethod
    def _result(at: Dict[str, object]) -> Dict[str, object]:
        res = {"aurc": at["aurc"], "error_auroc": at["error_auroc"], "rows": at["valid_rows"], "nan_rows": at["nan_rows"]}
        for j, c in enumerate(at["coverage"]):
            for name in ("accuracy", "bal_accuracy", "f1_mean", "threshold"):
                res[f"{name}@{c:g}"] = at[name][j]
        return res


def write_cine_log(path: str, cines: Sequence[dict], class_names: Sequence[str]) -> None:
    """One CSV row per cine: ``filename, target_AS, n_clips, prob_<label>..., uncertainty, pred`` (``cines`` as ``finish`` returns them)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        w.writerow(["filename", "target_AS", "n_clips"] + [f"prob_{n}" for n in class_names] + ["uncertainty", "pred"])
        for c in cines:
            if len(c["probs"]) != len(class_names):
                raise ValueError(f"{len(c['probs'])} probabilities for {len(class_names)} class names")
            w.writerow([c["filename"], c["target_AS"], c["n_clips"]] + [repr(float(p)) for p in c["probs"]] + [repr(float(c["uncertainty"])), c["pred"]])
