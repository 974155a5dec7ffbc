"""Out-of-distribution detection: does a clip look like anything the model was trained on?  (``csrc/ood.hip``)

``selective.py`` and ``calibration.py`` ask how sure the model is about a grade, ``conformal.py`` which grades it can not rule out,
``robustness.py`` how it moves under a known corruption; none of them says whether the INPUT is of the kind the model was trained on (a
wrong view, another vendor's scanner, an unusable acquisition), and the abstention output was trained on label ambiguity, not on that.
The detectors here do.  A HIGHER score means MORE out-of-distribution.  The reference has no code for any of it: the definitions in
``include/protoasnet_amd.h`` ("Out-of-distribution detection") are the specification, ``tests/ood_cases.py`` their numpy
restatement.

* ``head_scores(sim, logits, K_real)``: ``maxsim`` = 1 - the largest prototype similarity and ``energy`` = -logsumexp of the real logits;
  no fit.  ``"abstain"`` is ``selective.uncertainty``: the sweep can state whether the abstention output detects shift.
* ``knn(q, bank, k, self_base)``: the k nearest bank rows of every query in exact, order-defined fp32 arithmetic (bitwise reproducible,
  no query x bank matrix); the detector's score is the k-th distance.  ``rows_normalize`` puts rows on the unit sphere first.
* ``moments`` / ``gaussian_fit`` / ``mahalanobis``: class-conditional Gaussians with a pooled covariance.
* ``calibrate(scores_id, tprs)``: per detector and level the ``ceil((n + 1) tpr)``-th smallest in-distribution score (the exact order
  statistic of ``pasn_conformal_quantiles``): an exchangeable in-distribution row is flagged with probability at most ``1 - tpr``.
* ``evaluate(scores, kind, thresholds, correct)``: flags, integer tallies and the AUROC (``pasn_roc_auc_ovr``), read once.
* ``OODDetector``: the bank, the moments and the scores of a model's embeddings behind one object.

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .metrics import _f32, _require_cuda

DETECTORS = ("knn", "mahalanobis", "maxsim", "energy", "abstain")
BANK_DETECTORS = ("knn", "mahalanobis")
EMBEDDINGS = ("sim", "features")
MAX_E, MAX_K, MAX_MAHALANOBIS_E, MAX_CLASSES, MAX_LEVELS = 1024, 64, 256, 16, 8
MAX_QUERIES, MAX_BANK = 1 << 20, 1 << 24
TALLY_WORDS = 8
TALLY_NAMES = ("id_rows", "id_flagged", "ood_rows", "ood_flagged", "nan_rows", "id_correct_kept", "id_kept", "id_correct_flagged")


def _rows(x: torch.Tensor, what: str, max_rows: int, max_e: int = MAX_E):
    if x.dim() != 2:
        raise ValueError(f"{what} must be (M, E), got {tuple(x.shape)}")
    M, E = x.shape
    if not 1 <= M <= max_rows:
        raise ValueError(f"{what} takes 1 .. {max_rows} rows, got {M}")
    if not 1 <= E <= max_e:
        raise ValueError(f"{what} takes 1 .. {max_e} columns, got {E}")
    return M, E


def check_tprs(tprs) -> List[float]:
    try:
        tp = [float(t) for t in tprs]
    except TypeError:
        raise ValueError(f"tprs must be a sequence of numbers in (0, 1), got {tprs!r}") from None
    if not 1 <= len(tp) <= MAX_LEVELS or any(not 0.0 < t < 1.0 for t in tp):
        raise ValueError(f"tprs must hold 1 .. {MAX_LEVELS} numbers strictly between 0 and 1, got {tprs!r}")
    return tp


# ---- scores that need no fit -------------------------------------------------------------------------------------------------------------
def head_scores(sim: Optional[torch.Tensor], logits: Optional[torch.Tensor], num_real_classes: Optional[int] = None):
    """``(maxsim, energy)``, each (M,) fp32 (None where its input is None): ``1 - max_p sim`` and ``-logsumexp`` of the first
    ``num_real_classes`` logits (fp64, rounded once).  One launch; no host synchronisation."""
    _require_cuda(sim, logits)
    if sim is None and logits is None:
        raise ValueError("head_scores needs sim, logits or both")
    for t, what in ((sim, "sim"), (logits, "logits")):
        if t is not None:
            _rows(t, what, MAX_QUERIES, 4096)
    if sim is not None and logits is not None and sim.shape[0] != logits.shape[0]:
        raise ValueError("sim and logits must have the same rows")
    ref = sim if sim is not None else logits
    M, dev = ref.shape[0], ref.device
    P = sim.shape[1] if sim is not None else 1
    K = logits.shape[1] if logits is not None else 1
    K_real = K if num_real_classes is None else int(num_real_classes)
    if logits is not None and not 1 <= K_real <= K:
        raise ValueError(f"num_real_classes must lie in [1, {K}], got {num_real_classes}")
    with torch.cuda.device(dev):
        sim = None if sim is None else _f32(sim)
        logits = None if logits is None else _f32(logits)
        maxsim = None if sim is None else torch.empty(M, dtype=torch.float32, device=dev)
        energy = None if logits is None else torch.empty(M, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().pasn_ood_head_scores(_lib.ptr(sim), _lib.ptr(logits), M, P, K, K_real, _lib.ptr(maxsim), _lib.ptr(energy),
                                                   _lib.current_stream()))
    return maxsim, energy


def rows_normalize(x: torch.Tensor) -> torch.Tensor:
    """The rows of ``x`` (M, E) over their fp32 norm (a zero row is copied); bit for bit ``pasn_ood_rows_normalize``."""
    _require_cuda(x)
    M, E = _rows(x, "x", MAX_BANK)
    with torch.cuda.device(x.device):
        x = _f32(x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().pasn_ood_rows_normalize(_lib.ptr(x), M, E, _lib.ptr(y), _lib.current_stream()))
    return y


# ---- k nearest bank rows -----------------------------------------------------------------------------------------------------------------
class KNN:
    """Device result of ``knn``: ``dist`` (Mq, k) fp32 ascending, ``index`` (Mq, k) int32 (-1: fewer eligible rows than k), ``status``
    (2,) int64 = {bank rows holding a NaN, query rows holding a NaN}.  ``score`` is the k-th distance."""

    def __init__(self, dist, index, status):
        self.dist, self.index, self.status = dist, index, status

    @property
    def score(self) -> torch.Tensor:
        return self.dist[:, -1].contiguous()


def knn(q: torch.Tensor, bank: torch.Tensor, k: int = 10, self_base: int = -1) -> KNN:
    """The ``k`` nearest rows of ``bank`` (Mb, E) for every row of ``q`` (Mq, E): squared Euclidean distance accumulated in fp32 in
    coordinate order without FMA, ties to the lower bank index, rows holding a NaN never neighbours.  ``self_base >= 0``: query i IS bank
    row ``self_base + i`` and is left out of its own neighbours.  A memset and two launches; no host synchronisation."""
    _require_cuda(q, bank)
    Mq, E = _rows(q, "q", MAX_QUERIES)
    Mb, Eb = _rows(bank, "bank", MAX_BANK)
    if E != Eb:
        raise ValueError(f"q has {E} columns, the bank {Eb}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
    if isinstance(self_base, bool) or not isinstance(self_base, (int, np.integer)) or not -1 <= self_base <= Mb:
        raise ValueError(f"self_base must be -1 or a bank row, got {self_base!r}")
    dev, lib = q.device, _lib.lib()
    with torch.cuda.device(dev):
        q, bank = _f32(q), _f32(bank)
        dist = torch.empty(Mq, k, dtype=torch.float32, device=dev)
        index = torch.empty(Mq, k, dtype=torch.int32, device=dev)
        status = torch.empty(2, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.pasn_ood_knn_workspace_bytes(Mq, Mb, E, int(k)), dev)
        _lib.check(lib.pasn_ood_knn(_lib.ptr(q), _lib.ptr(bank), Mq, Mb, E, int(k), int(self_base), _lib.ptr(dist), _lib.ptr(index),
                                    _lib.ptr(status), _lib.ptr(ws), _lib.current_stream()))
    return KNN(dist, index, status)


# ---- class-conditional Gaussians -----------------------------------------------------------------------------------------------------------
def moment_chunk() -> int:
    return int(_lib.lib().pasn_ood_moment_chunk())


class Moments:
    """Device sums of ``moments``: ``n`` (K,) int64, ``sum`` (K, E) fp64, ``scatter`` (E, E) fp64, ``skipped`` (2,) int64 = {rows with a
    label out of range, labelled rows holding a NaN}."""

    def __init__(self, n, sum, scatter, skipped):
        self.n, self.sum, self.scatter, self.skipped = n, sum, scatter, skipped


def moments(x: torch.Tensor, labels: torch.Tensor, num_classes: int, into: Optional[Moments] = None) -> Moments:
    """The exact fp64 moments of the valid rows of ``x`` (M, E <= 256) under ``labels`` (M,), in the fixed order of
    ``pasn_ood_moments``; ``into``: added onto an earlier call's result (which is returned).  No host synchronisation."""
    _require_cuda(x, labels)
    M, E = _rows(x, "x", MAX_BANK, MAX_MAHALANOBIS_E)
    K = int(num_classes)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"num_classes must lie in [1, {MAX_CLASSES}], got {num_classes}")
    if labels.shape != (M,):
        raise ValueError("labels must be (M,)")
    dev, lib = x.device, _lib.lib()
    with torch.cuda.device(dev):
        if into is None:
            out = Moments(torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, E, dtype=torch.float64, device=dev),
                          torch.empty(E, E, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.int64, device=dev))
        else:
            out = into
            if out.sum.shape != (K, E):
                raise ValueError(f"the earlier moments are {tuple(out.sum.shape)}, these rows give ({K}, {E})")
        ws = _lib.workspace(lib.pasn_ood_moments_workspace_bytes(M, E, K), dev)
        _lib.check(lib.pasn_ood_moments(_lib.ptr(_f32(x)), _lib.ptr(labels.to(torch.int32).contiguous()), M, E, K, int(into is not None),
                                        _lib.ptr(out.n), _lib.ptr(out.sum), _lib.ptr(out.scatter), _lib.ptr(out.skipped), _lib.ptr(ws),
                                        _lib.current_stream()))
    return out


def gaussian_fit(n, sum, scatter, shrink: float = 1e-6):
    """The host finish of a fit, float64 numpy: ``(mu (K, E), W (E, E))`` with ``mu_c = sum_c / n_c`` (NaN for a class without rows), the
    pooled within-class covariance ``S = (scatter - sum_c n_c mu_c mu_c^T) / (N - C)`` (C: the classes with rows),
    ``S += shrink (tr S / E) I`` and ``W = L^-1`` for ``S = L L^T``.  Fewer than ``E + C`` valid rows is a ``ValueError``."""
    n = np.asarray(n, dtype=np.int64)
    s, sc = np.asarray(sum, dtype=np.float64), np.asarray(scatter, dtype=np.float64)
    K, E = s.shape
    if not (float(shrink) >= 0.0 and np.isfinite(float(shrink))):
        raise ValueError(f"shrink must be a finite number >= 0, got {shrink!r}")
    N, C = int(n.sum()), int((n > 0).sum())
    if N < E + C:
        raise ValueError(f"a Mahalanobis fit of {E} dimensions and {C} classes needs at least {E + C} valid rows, got {N}")
    mu = np.full((K, E), np.nan)
    within = sc.copy()
    for c in range(K):
        if n[c] > 0:
            mu[c] = s[c] / float(n[c])
            within = within - float(n[c]) * np.outer(mu[c], mu[c])
    cov = within / float(N - C)
    cov = cov + float(shrink) * (np.trace(cov) / E) * np.eye(E)
    W = np.linalg.inv(np.linalg.cholesky(cov))
    return mu, np.tril(W)


def mahalanobis(x: torch.Tensor, mu: torch.Tensor, W: torch.Tensor):
    """``(m (M, K) fp64, score (M,) fp32, argclass (M,) int32)``: ``m_c = ||W (x - mu_c)||^2`` and its minimum over the classes with a
    finite mean.  One launch; no host synchronisation."""
    _require_cuda(x, mu, W)
    M, E = _rows(x, "x", MAX_QUERIES, MAX_MAHALANOBIS_E)
    if mu.dim() != 2 or mu.shape[1] != E or not 1 <= mu.shape[0] <= MAX_CLASSES or W.shape != (E, E):
        raise ValueError(f"mu must be (K <= {MAX_CLASSES}, {E}) and W ({E}, {E})")
    K, dev = mu.shape[0], x.device
    with torch.cuda.device(dev):
        m = torch.empty(M, K, dtype=torch.float64, device=dev)
        score = torch.empty(M, dtype=torch.float32, device=dev)
        arg = torch.empty(M, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().pasn_ood_mahalanobis(_lib.ptr(_f32(x)), _lib.ptr(mu.double().contiguous()), _lib.ptr(W.double().contiguous()),
                                                   M, E, K, _lib.ptr(m), _lib.ptr(score), _lib.ptr(arg), _lib.current_stream()))
    return m, score, arg


# ---- thresholds, flags, tallies ------------------------------------------------------------------------------------------------------------
class OODThresholds:
    """Device result of ``calibrate``: per detector ``tau`` (A,) fp32, ``n`` (1,) int64 the scores that entered, ``nan`` 0-d int64 the
    NaN scores left out; ``tprs`` the levels."""

    def __init__(self, tau: Dict[str, torch.Tensor], n: Dict[str, torch.Tensor], nan: Dict[str, torch.Tensor], tprs: Sequence[float]):
        self.tau, self.n, self.nan, self.tprs = tau, n, nan, [float(t) for t in tprs]

    def read(self) -> Dict[str, object]:
        """ONE synchronising copy: ``{tprs, detectors: {name: {tau, n, nan_rows}}}``."""
        names, A = list(self.tau), len(self.tprs)
        v = torch.cat([torch.cat([self.tau[d].double(), self.n[d].double().reshape(1), self.nan[d].double().reshape(1)]) for d in names]).cpu()
        v = v.view(len(names), A + 2)
        return {"tprs": list(self.tprs),
                "detectors": {d: {"tau": v[i, :A].tolist(), "n": int(v[i, A]), "nan_rows": int(v[i, A + 1])} for i, d in enumerate(names)}}


def _threshold(score: torch.Tensor, tprs: Sequence[float]):
    M, dev, A, lib = score.shape[0], score.device, len(tprs), _lib.lib()
    with torch.cuda.device(dev):
        own = _f32(score)
        bad = torch.isnan(own)
        stratum = torch.where(bad, -2, 0).to(torch.int32)  # (pasn_conformal_scores' codes: 0 a valid row of label 0, -2 a NaN row)
        qhat = torch.empty(3, A, dtype=torch.float32, device=dev)
        n = torch.empty(3, dtype=torch.int64, device=dev)
        r = torch.empty(3, A, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.pasn_conformal_workspace_bytes(M, 2, A), dev)
        alphas = (ctypes.c_double * A)(*[1.0 - t for t in tprs])
        _lib.check(lib.pasn_conformal_quantiles(_lib.ptr(own), _lib.ptr(stratum), M, 2, A, alphas, _lib.ptr(qhat), _lib.ptr(n), _lib.ptr(r),
                                                _lib.ptr(ws), _lib.current_stream()))
    return qhat[0].contiguous(), n[:1], bad.sum()


def calibrate(scores_id, tprs=(0.95,)) -> OODThresholds:
    """The thresholds of in-distribution scores -- a dict ``{detector: (M,) fp32}`` or one tensor (detector ``"score"``) -- at the levels
    ``tprs``: per level the ``r``-th smallest score, ``r = ceil((n + 1) tpr)``, ``+inf`` when ``r > n``; NaN scores are left out and
    counted.  The exact selection of ``pasn_conformal_quantiles`` with ``alpha = 1 - tpr``; no host synchronisation."""
    tp = check_tprs(tprs)
    if isinstance(scores_id, torch.Tensor):
        scores_id = {"score": scores_id}
    if not scores_id:
        raise ValueError("calibrate needs at least one detector's scores")
    tau, n, nan = {}, {}, {}
    for name, s in scores_id.items():
        _require_cuda(s)
        if s.dim() != 1 or not 1 <= s.shape[0] <= MAX_QUERIES:
            raise ValueError(f"the scores of {name!r} must be (M,), 1 <= M <= {MAX_QUERIES}, got {tuple(s.shape)}")
        tau[name], n[name], nan[name] = _threshold(s, tp)
    return OODThresholds(tau, n, nan, tp)


def tally(scores: torch.Tensor, kind: torch.Tensor, tau: torch.Tensor, correct: Optional[torch.Tensor] = None):
    """``(flags (A, M) uint8, tallies (A, 8) int64)`` of ``pasn_ood_tally``: a row is flagged iff ``score > tau`` or the score is NaN;
    ``kind`` 0 in-distribution, 1 shifted, anything else padding; ``TALLY_NAMES`` names the columns."""
    _require_cuda(scores, kind, tau, correct)
    if scores.dim() != 1 or kind.shape != scores.shape or (correct is not None and correct.shape != scores.shape):
        raise ValueError("scores, kind and correct must be (M,)")
    if tau.dim() != 1 or not 1 <= tau.shape[0] <= MAX_LEVELS:
        raise ValueError(f"tau must be (A,), 1 <= A <= {MAX_LEVELS}")
    M, A, dev = scores.shape[0], tau.shape[0], scores.device
    if not 1 <= M <= MAX_QUERIES:
        raise ValueError(f"tally takes 1 .. {MAX_QUERIES} rows, got {M}")
    with torch.cuda.device(dev):
        flags = torch.empty(A, M, dtype=torch.uint8, device=dev)
        tallies = torch.empty(A, TALLY_WORDS, dtype=torch.int64, device=dev)
        correct = None if correct is None else correct.to(torch.int32).contiguous()
        _lib.check(_lib.lib().pasn_ood_tally(_lib.ptr(_f32(scores)), _lib.ptr(kind.to(torch.int32).contiguous()), _lib.ptr(correct),
                                             _lib.ptr(_f32(tau)), M, A, _lib.ptr(flags), _lib.ptr(tallies), _lib.current_stream()))
    return flags, tallies


def auroc(scores: torch.Tensor, kind: torch.Tensor) -> torch.Tensor:
    """The AUROC of ``scores`` with the shifted rows (``kind == 1``) as positives against the in-distribution ones (``kind == 0``): a 0-d
    fp64 device tensor, NaN when either side is empty.  ``pasn_roc_auc_ovr`` on the two-column table ``(-score, score)`` -- an exact
    Mann-Whitney count; rows of another kind and rows with a NaN score do not enter."""
    from .metrics import roc_auc_ovr_weighted

    _require_cuda(scores, kind)
    s = _f32(scores)
    labels = torch.where((kind == 0) | (kind == 1), kind.to(torch.int32), -1)
    labels = torch.where(torch.isnan(s), -1, labels).to(torch.int32)
    s = torch.nan_to_num(s, nan=0.0, posinf=float("inf"), neginf=float("-inf"))  # (only rows that do not enter change)
    _, per_class = roc_auc_ovr_weighted(torch.stack([-s, s], dim=1), labels, 2, per_class=True)
    return per_class[1]


class OODEvaluation:
    """Device results of ``evaluate``: per detector ``flags`` (A, M) uint8, ``tallies`` (A, 8) int64 and ``auroc`` 0-d fp64."""

    def __init__(self, flags, tallies, auroc, tprs):
        self.flags, self.tallies, self.auroc, self.tprs = flags, tallies, auroc, list(tprs)

    def packed(self) -> torch.Tensor:
        """The fp64 device vector ``read`` copies: per detector the tallies (below 2^53: exact) and the AUROC."""
        return torch.cat([torch.cat([self.tallies[d].double().flatten(), self.auroc[d].reshape(1)]) for d in self.tallies])

    @staticmethod
    def unpack(host, names: Sequence[str], tprs: Sequence[float]) -> Dict[str, object]:
        A = len(tprs)
        v = np.asarray(host, dtype=np.float64).reshape(len(names), A * TALLY_WORDS + 1)
        nan = float("nan")

        def div(a, b):
            return float(a) / float(b) if b else nan

        out = {}
        for i, d in enumerate(names):
            t = v[i, :-1].reshape(A, TALLY_WORDS)
            out[d] = {"auroc": float(v[i, -1]), "levels": [{
                "tpr": float(tpr), **{k: int(x) for k, x in zip(TALLY_NAMES, w)},
                "id_flagged_rate": div(w[1], w[0]), "ood_flagged_rate": div(w[3], w[2]),
                "accuracy_kept": div(w[5], w[6]), "accuracy_flagged": div(w[7], w[1])} for tpr, w in zip(tprs, t)]}
        return out

    def read(self) -> Dict[str, object]:
        """ONE synchronising copy: per detector ``{auroc, levels: [{tpr, <TALLY_NAMES>, id_flagged_rate, ood_flagged_rate, accuracy_kept,
        accuracy_flagged}]}`` (a rate with a zero denominator is NaN; the accuracies need ``correct``)."""
        return self.unpack(self.packed().cpu().numpy(), list(self.tallies), self.tprs)


def evaluate(scores: Dict[str, torch.Tensor], kind: torch.Tensor, thresholds: OODThresholds,
             correct: Optional[torch.Tensor] = None) -> OODEvaluation:
    """Every detector of ``scores`` against its thresholds on rows of ``kind`` (0 in-distribution, 1 shifted): flags, tallies and the
    AUROC on the device; ``.read()`` gives plain numbers.  No host synchronisation."""
    if not isinstance(thresholds, OODThresholds):
        raise ValueError(f"thresholds must be an OODThresholds (ood.calibrate), got {thresholds!r}")
    flags, tallies, auc = {}, {}, {}
    for name, s in scores.items():
        if name not in thresholds.tau:
            raise ValueError(f"no threshold was calibrated for {name!r}")
        flags[name], tallies[name] = tally(s, kind, thresholds.tau[name], correct)
        auc[name] = auroc(s, kind)
    return OODEvaluation(flags, tallies, auc, thresholds.tprs)


# ---- the detector ------------------------------------------------------------------------------------------------------------------------
class OODFit:
    """What ``OODDetector.fit_finish`` leaves: ``bank`` (Mb, E) fp32 on the device (normalised when the detector normalises), ``mu`` (K, E)
    and ``W`` (E, E) fp64 on the device (None without ``"mahalanobis"``), ``n`` the valid rows per class (host), ``skipped`` (host) and,
    once calibrated, ``thresholds``."""

    def __init__(self, bank, mu, W, n, skipped):
        self.bank, self.mu, self.W, self.n, self.skipped = bank, mu, W, n, skipped
        self.thresholds: Optional[OODThresholds] = None


def check_detectors(detectors) -> tuple:
    d = tuple(detectors)
    if not d or any(x not in DETECTORS for x in d) or len(set(d)) != len(d):
        raise ValueError(f"detectors must be distinct names of {DETECTORS}, got {detectors!r}")
    return d


def embedding_of(feats: torch.Tensor, proto_dist: torch.Tensor, embedding: str = "sim") -> torch.Tensor:
    """The (M, E) fp32 embedding of ``push_forward``'s outputs: ``"sim"`` = 1 - proto_dist, the P similarities the last layer sees (its
    penultimate feature); ``"features"`` = the mean over the prototypes of the pooled features."""
    if embedding == "sim":
        return (1 - proto_dist).float().contiguous()
    if embedding == "features":
        return feats.float().mean(1).contiguous()
    raise ValueError(f"embedding must be one of {EMBEDDINGS}, got {embedding!r}")


class OODDetector:
    """``fit_update(emb, labels)`` per batch of the training split, ``fit_finish()``, then ``scores(emb, sim, logits)`` for any rows.

    ``detectors``: which of ``DETECTORS``; ``embedding``: what ``embed`` makes of ``push_forward``'s outputs (a caller may hand
    ``fit_update`` / ``scores`` any (M, E) fp32 tensor instead); ``k``: the neighbour whose distance is the kNN score; ``normalize``: kNN
    on the unit sphere (queries and bank through ``rows_normalize``), as in deep-nearest-neighbour detection -- the Mahalanobis moments
    take the rows as they are; ``shrink``: the ridge of ``gaussian_fit``; ``num_classes``: the label range of the Mahalanobis fit (None:
    one read of the first batch's largest label); ``abstain_class``: the last logit is the abstention output (needed by ``"abstain"``)."""

    def __init__(self, detectors=DETECTORS, embedding="sim", k: int = 10, normalize: bool = True, shrink: float = 1e-6,
                 num_classes: Optional[int] = None, abstain_class: bool = True):
        self.detectors = check_detectors(detectors)
        if embedding not in EMBEDDINGS:
            raise ValueError(f"embedding must be one of {EMBEDDINGS}, got {embedding!r}")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
            raise ValueError(f"k must be an integer in [1, {MAX_K}], got {k!r}")
        if not isinstance(normalize, (bool, np.bool_)):
            raise ValueError(f"normalize must be a bool, got {normalize!r}")
        if isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating)) or not (shrink >= 0 and np.isfinite(shrink)):
            raise ValueError(f"shrink must be a finite number >= 0, got {shrink!r}")
        if "abstain" in self.detectors and not abstain_class:
            raise ValueError("the detector 'abstain' needs a model with an abstention class")
        self.embedding, self.k, self.normalize, self.shrink = embedding, int(k), bool(normalize), float(shrink)
        self.num_classes, self.abstain_class = num_classes, bool(abstain_class)
        self._bank: List[torch.Tensor] = []
        self._moments: Optional[Moments] = None
        self.fit: Optional[OODFit] = None
        self.thresholds: Optional[OODThresholds] = None

    def embed(self, feats, proto_dist) -> torch.Tensor:
        return embedding_of(feats, proto_dist, self.embedding)

    def _check_emb(self, emb):
        _require_cuda(emb)
        M, E = _rows(emb, "emb", MAX_QUERIES)
        if "mahalanobis" in self.detectors and E > MAX_MAHALANOBIS_E:
            raise ValueError(f"'mahalanobis' takes embeddings of at most {MAX_MAHALANOBIS_E} dimensions, got {E}: use 'knn' for wider ones")
        return M, E

    def fit_update(self, emb: torch.Tensor, labels: Optional[torch.Tensor] = None) -> None:
        """Appends the rows to the device bank and (with ``"mahalanobis"``) accumulates their moments under ``labels`` (M,)."""
        self._check_emb(emb)
        emb = _f32(emb)
        if "knn" in self.detectors:
            self._bank.append(rows_normalize(emb) if self.normalize else emb.clone())
        if "mahalanobis" in self.detectors:
            if labels is None:
                raise ValueError("'mahalanobis' needs the labels of the bank rows")
            _require_cuda(labels)
            if self.num_classes is None:
                self.num_classes = int(labels.max().item()) + 1
            self._moments = moments(emb, labels, self.num_classes, into=self._moments)
        self.fit = None

    def fit_finish(self) -> OODFit:
        """The fit: the bank in one tensor and, after ONE read of the moments, ``mu`` and ``W`` back on the device."""
        bank = mu = W = n = skipped = None
        if "knn" in self.detectors:
            if not self._bank:
                raise ValueError("no rows: fit_update() was never called")
            bank = torch.cat(self._bank) if len(self._bank) > 1 else self._bank[0]
            self._bank = [bank]
            if bank.shape[0] > MAX_BANK:
                raise ValueError(f"the bank holds {bank.shape[0]} rows, at most {MAX_BANK}")
        if "mahalanobis" in self.detectors:
            mo = self._moments
            if mo is None:
                raise ValueError("no rows: fit_update() was never called")
            K, E = mo.sum.shape
            host = torch.cat([mo.n.double(), mo.skipped.double(), mo.sum.flatten(), mo.scatter.flatten()]).cpu().numpy()  # the one read
            n, skipped = host[:K].astype(np.int64), host[K: K + 2].astype(np.int64)
            mu_h, W_h = gaussian_fit(n, host[K + 2: K + 2 + K * E].reshape(K, E), host[K + 2 + K * E:].reshape(E, E), self.shrink)
            dev = mo.sum.device
            mu, W = torch.from_numpy(mu_h).to(dev), torch.from_numpy(np.ascontiguousarray(W_h)).to(dev)
        self.fit = OODFit(bank, mu, W, n, skipped)
        return self.fit

    def scores(self, emb: Optional[torch.Tensor] = None, sim: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None,
               self_base: int = -1) -> Dict[str, torch.Tensor]:
        """``{detector: (M,) fp32}`` on the device for rows given by their embedding (the bank detectors), similarities (``maxsim``) and
        logits (``energy``, ``abstain``).  ``self_base >= 0``: the rows ARE bank rows ``self_base ..``, and the kNN scan leaves each out
        of its own neighbours (the Mahalanobis fit is not leave-one-out).  No host synchronisation."""
        out: Dict[str, torch.Tensor] = {}
        need_fit = [d for d in self.detectors if d in BANK_DETECTORS]
        if need_fit:
            if self.fit is None:
                raise ValueError("fit_finish() first: 'knn' and 'mahalanobis' score against a fit")
            if emb is None:
                raise ValueError("'knn' and 'mahalanobis' need the embedding")
            self._check_emb(emb)
        K_real = None if logits is None else logits.shape[1] - (1 if self.abstain_class else 0)
        for d in self.detectors:
            if d == "knn":
                q = rows_normalize(emb) if self.normalize else emb
                out[d] = knn(q, self.fit.bank, self.k, self_base).score
            elif d == "mahalanobis":
                out[d] = mahalanobis(emb, self.fit.mu, self.fit.W)[1]
            elif d == "maxsim":
                if sim is None:
                    raise ValueError("'maxsim' needs sim")
                out[d] = head_scores(sim, None)[0]
            elif d == "energy":
                if logits is None:
                    raise ValueError("'energy' needs logits")
                out[d] = head_scores(None, logits, K_real)[1]
            else:
                if logits is None:
                    raise ValueError("'abstain' needs logits")
                from . import selective

                out[d] = selective.uncertainty(logits, True, "alpha")
        return out

    def calibrate(self, scores: Dict[str, torch.Tensor], tprs=(0.95,)) -> OODThresholds:
        """``ood.calibrate`` on in-distribution scores; the thresholds are kept in the fit."""
        th = calibrate(scores, tprs)
        if self.fit is not None:
            self.fit.thresholds = th
        self.thresholds = th
        return th

    def evaluate(self, scores: Dict[str, torch.Tensor], kind: torch.Tensor, correct: Optional[torch.Tensor] = None,
                 thresholds: Optional[OODThresholds] = None) -> OODEvaluation:
        """``ood.evaluate`` under the calibrated thresholds."""
        th = thresholds if thresholds is not None else self.thresholds
        if th is None:
            raise ValueError("calibrate() first")
        return evaluate(scores, kind, th, correct)
