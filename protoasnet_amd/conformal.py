"""Conformal prediction sets: which classes can not be ruled out for a study, at a stated error rate?  (``csrc/conformal.hip``)

``selective.py`` evaluates the abstention output, ``bootstrap.py`` puts intervals on the metrics, ``calibration.py`` asks whether the
probabilities are honest; none of them gives a guarantee for a single study.  Split conformal prediction does: thresholds calibrated on
one split (``val``), and for every row of another a set of classes that holds the true one with probability >= 1 - alpha -- for
EXCHANGEABLE rows: the clips of one cine are not exchangeable with another patient's, so the guarantee is a cine-level one
(``DPTrainer.fit_conformal(level="cine")``).  The reference has no code for this: the definitions in ``include/protoasnet_amd.h``
("Conformal prediction") are the specification, ``tests/conformal_cases.py`` their float64 / int64 restatement.

* ``scores(probs, labels, kind, randomized, seed, lam, k_reg, salt)``: the (M, K) score table -- ``lac`` = 1 - p, ``aps`` = the
  probability mass ranked before the class plus ``U`` times its own (one Philox uniform per row when ``randomized``), ``raps`` = ``aps``
  plus ``lam * max(0, rank - k_reg)`` -- and with labels the own-label scores and strata.
* ``calibrate(probs, labels, alphas, kind, ...) -> ConformalFit``: per stratum (all valid rows; the valid rows of each label) and alpha
  the ``ceil((n + 1)(1 - alpha))``-th smallest own-label score, ``+inf`` when there are too few rows.  An exact selection.
* ``predict_sets(probs, fit, labels, u, mondrian) -> ConformalSets``: the (A, M) uint16 class masks and the integer tallies behind
  coverage, set sizes, per-class and size-stratified coverage and the mean uncertainty per set size; ``summary()`` is ONE read.

Everything runs on the device on the caller's stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .metrics import MAX_K, MAX_ROWS, _f32, _require_cuda

KINDS = ("lac", "aps", "raps")  # PASN_CONFORMAL_LAC / _APS / _RAPS
MAX_ALPHAS = 8
SALT_CALIBRATE, SALT_PREDICT = 0, 1  # the uniforms of the two splits must not be the same numbers


def tally_words(K: int) -> int:
    """The int64 words of one level's tallies: rows, covered, nan_rows; four arrays by set size; two by label."""
    return 3 + 4 * (K + 1) + 2 * K


def check_alphas(alphas) -> List[float]:
    try:
        al = [float(a) for a in alphas]
    except TypeError:
        raise ValueError(f"alphas must be a sequence of numbers in (0, 1), got {alphas!r}") from None
    if not 1 <= len(al) <= MAX_ALPHAS or any(not 0.0 < a < 1.0 for a in al):
        raise ValueError(f"alphas must hold 1 .. {MAX_ALPHAS} numbers strictly between 0 and 1, got {alphas!r}")
    return al


def check_settings(kind="aps", randomized=True, seed=0, lam=0.0, k_reg=1, salt=0) -> Dict[str, object]:
    """The score settings, checked on the host: ``{kind, randomized, seed, lam, k_reg}`` (and the salt's range)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if not isinstance(randomized, (bool, np.bool_)):
        raise ValueError(f"randomized must be a bool, got {randomized!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not (lam >= 0 and np.isfinite(lam)):
        raise ValueError(f"lam must be a finite number >= 0, got {lam!r}")
    if isinstance(k_reg, bool) or not isinstance(k_reg, (int, np.integer)) or k_reg < 0:
        raise ValueError(f"k_reg must be an integer >= 0, got {k_reg!r}")
    if isinstance(salt, bool) or not isinstance(salt, (int, np.integer)) or not 0 <= salt < 1 << 32:
        raise ValueError(f"salt must be an integer in [0, 2^32), got {salt!r}")
    return {"kind": kind, "randomized": bool(randomized), "seed": int(seed), "lam": float(lam), "k_reg": int(k_reg)}


def _check_rows(probs: torch.Tensor, labels: Optional[torch.Tensor], u: Optional[torch.Tensor] = None):
    if probs.dim() != 2 or (labels is not None and labels.shape != probs.shape[:1]) or (u is not None and u.shape != probs.shape[:1]):
        raise ValueError("probs must be (M, K_real), labels and u (M,)")
    M, K = probs.shape
    if not 1 <= M <= MAX_ROWS:
        raise ValueError(f"conformal prediction takes 1 .. {MAX_ROWS} rows, got {M}")
    if not 2 <= K <= MAX_K:
        raise ValueError(f"conformal prediction takes 2 .. {MAX_K} classes, got {K}")
    return M, K


def _scores(probs, labels, settings, salt):
    """(scores, own, stratum) on the device; own and stratum are None without labels."""
    M, K = probs.shape
    dev = probs.device
    with torch.cuda.device(dev):
        probs = _f32(probs)
        labels = None if labels is None else labels.to(torch.int32).contiguous()
        table = torch.empty(M, K, dtype=torch.float32, device=dev)
        own = None if labels is None else torch.empty(M, dtype=torch.float32, device=dev)
        stratum = None if labels is None else torch.empty(M, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().pasn_conformal_scores(_lib.ptr(probs), _lib.ptr(labels), M, K, KINDS.index(settings["kind"]),
                                                    int(settings["randomized"]), settings["seed"], int(salt), settings["lam"],
                                                    settings["k_reg"], _lib.ptr(table), _lib.ptr(own), _lib.ptr(stratum), _lib.current_stream()))
    return table, own, stratum


def scores(probs: torch.Tensor, labels: Optional[torch.Tensor] = None, kind: str = "aps", randomized: bool = True, seed: int = 0,
           lam: float = 0.0, k_reg: int = 1, salt: int = 0):
    """The (M, K_real) fp32 conformal scores of ``probs``; with ``labels`` (M,) returns ``(scores, own, stratum)``: the own-label score
    (NaN where the row is not valid) and the label of a valid row, -1 for a padding row, -2 for a row holding a NaN.  No host
    synchronisation."""
    settings = check_settings(kind, randomized, seed, lam, k_reg, salt)
    _require_cuda(probs, labels)
    _check_rows(probs, labels)
    table, own, stratum = _scores(probs, labels, settings, salt)
    return table if labels is None else (table, own, stratum)


class ConformalFit:
    """Device result of ``calibrate``: ``qhat`` (1 + K, A) fp32 -- row 0 the marginal thresholds, row 1 + c class c's --, ``n`` (1 + K,)
    int64 the rows of each stratum, ``r`` (1 + K, A) int64 the ranks that were selected; and the score settings (``kind``,
    ``randomized``, ``seed``, ``lam``, ``k_reg``), ``alphas`` and ``K``, so that prediction can not be run with other ones."""

    def __init__(self, qhat: torch.Tensor, n: torch.Tensor, r: torch.Tensor, alphas: Sequence[float], settings: Dict[str, object]):
        self.qhat, self.n, self.r = qhat, n, r
        self.alphas = [float(a) for a in alphas]
        self.settings = dict(settings)
        self.K = qhat.shape[0] - 1

    @property
    def kind(self) -> str:
        return self.settings["kind"]

    def read(self) -> Dict[str, object]:
        """ONE synchronising copy: ``{kind, alphas, qhat, qhat_per_class, n, n_per_class, r}`` (``qhat`` one number per alpha)."""
        A, S = len(self.alphas), self.K + 1
        v = torch.cat([self.qhat.double().flatten(), self.n.double(), self.r.double().flatten()]).cpu()
        q, n, r = v[: S * A].view(S, A), v[S * A: S * A + S].long(), v[S * A + S:].view(S, A).long()
        return {"kind": self.kind, "alphas": list(self.alphas), "qhat": q[0].tolist(), "qhat_per_class": q[1:].tolist(), "n": int(n[0]),
                "n_per_class": n[1:].tolist(), "r": r[0].tolist()}

    def state_dict(self) -> Dict[str, object]:
        """Host tensors and plain values (a synchronising copy): what ``torch.save`` can put next to a checkpoint."""
        return {"qhat": self.qhat.cpu(), "n": self.n.cpu(), "r": self.r.cpu(), "alphas": list(self.alphas), **self.settings}

    @classmethod
    def from_state_dict(cls, sd: Dict[str, object], device="cuda") -> "ConformalFit":
        settings = check_settings(sd["kind"], sd["randomized"], sd["seed"], sd["lam"], sd["k_reg"])
        alphas = check_alphas(sd["alphas"])
        qhat, n, r = (torch.as_tensor(sd[k]).to(device=device, dtype=d).contiguous()
                      for k, d in (("qhat", torch.float32), ("n", torch.int64), ("r", torch.int64)))
        if qhat.dim() != 2 or qhat.shape[1] != len(alphas) or not 2 <= qhat.shape[0] - 1 <= MAX_K or n.shape != qhat.shape[:1] or r.shape != qhat.shape:
            raise ValueError("qhat and r must be (1 + K, A), n (1 + K,), with one column per alpha")
        return cls(qhat, n, r, alphas, settings)


def calibrate(probs: torch.Tensor, labels: torch.Tensor, alphas=(0.1,), kind: str = "aps", randomized: bool = True, seed: int = 0,
              lam: float = 0.0, k_reg: int = 1) -> ConformalFit:
    """The thresholds of ``probs`` (M, K_real) fp32 against ``labels`` (M,) (< 0 or >= K_real: a padding row) at the miscoverage levels
    ``alphas``.  A fixed number of launches whatever M is; no host synchronisation."""
    al = check_alphas(alphas)
    settings = check_settings(kind, randomized, seed, lam, k_reg)
    if labels is None:
        raise ValueError("calibrate needs labels")
    _require_cuda(probs, labels)
    M, K = _check_rows(probs, labels)
    _, own, stratum = _scores(probs, labels, settings, SALT_CALIBRATE)
    dev, A, lib = probs.device, len(al), _lib.lib()
    with torch.cuda.device(dev):
        qhat = torch.empty(K + 1, A, dtype=torch.float32, device=dev)
        n = torch.empty(K + 1, dtype=torch.int64, device=dev)
        r = torch.empty(K + 1, A, dtype=torch.int64, device=dev)
        ws = _lib.workspace(lib.pasn_conformal_workspace_bytes(M, K, A), dev)
        _lib.check(lib.pasn_conformal_quantiles(_lib.ptr(own), _lib.ptr(stratum), M, K, A, (ctypes.c_double * A)(*al), _lib.ptr(qhat),
                                                _lib.ptr(n), _lib.ptr(r), _lib.ptr(ws), _lib.current_stream()))
    return ConformalFit(qhat, n, r, al, settings)


class ConformalSets:
    """Device results of ``predict_sets``: ``masks`` (A, M) uint16 -- bit k: class k is in the row's set -- and ``tallies`` (A, T) int64,
    ``T = tally_words(K)``, per level ``[rows, covered, nan_rows, size_hist, covered_by_size, u_by_size, u_rows_by_size (K + 1 each),
    class_n, class_covered (K each)]``; ``u_by_size`` holds the uint64 sums of ``q = u * 2^32`` (below 2^63: the bits are the same)."""

    def __init__(self, masks, tallies, alphas, K, kind, mondrian, has_labels, has_u):
        self.masks, self.tallies = masks, tallies
        self.alphas, self.K, self.kind, self.mondrian, self.has_labels, self.has_u = list(alphas), K, kind, bool(mondrian), has_labels, has_u

    def packed(self) -> torch.Tensor:
        """The int64 device vector ``summary`` reads: the tallies, flattened."""
        return self.tallies.flatten()

    @staticmethod
    def unpack(host, alphas, K: int, has_labels: bool = True, has_u: bool = True) -> List[Dict[str, object]]:
        """One dict per alpha from the tallies on the host (int64, or the fp64 copy a joined read carries: every count is below 2^53
        but ``u_by_size``, which is read in fp64 anyway).  A reading with a zero denominator is NaN; the label readings are NaN
        without labels, the ``u`` readings without ``u``."""
        nan = float("nan")
        T = tally_words(K)
        t = np.asarray(host).reshape(len(alphas), T)
        out = []

        def div(a, b):
            return float(a) / float(b) if b else nan

        for alpha, w in zip(alphas, t):
            rows, covered, nan_rows = int(w[0]), int(w[1]), int(w[2])
            o = 3
            size, cov_size, uq, un = (w[o + j * (K + 1): o + (j + 1) * (K + 1)] for j in range(4))
            o += 4 * (K + 1)
            cn, cc = w[o: o + K], w[o + K: o + 2 * K]
            by_size = [div(c, s) if has_labels else nan for c, s in zip(cov_size, size)]
            seen = [x for x, s in zip(by_size, size) if s]
            out.append({
                "alpha": float(alpha), "rows": rows, "nan_rows": nan_rows,
                "coverage": div(covered, rows) if has_labels else nan,
                "mean_size": div(sum(k * int(s) for k, s in enumerate(size)), rows),
                "empty": div(size[0], rows), "singleton": div(size[1], rows),
                "singleton_accuracy": div(cov_size[1], size[1]) if has_labels else nan,
                "size_hist": [int(s) for s in size],
                "class_n": [int(c) for c in cn],
                "class_coverage": [div(c, m) if has_labels else nan for c, m in zip(cc, cn)],
                "coverage_by_size": by_size,
                "min_coverage_by_size": min(seen) if has_labels and seen else nan,
                "u_by_size": [div(float(q) * 2.0 ** -32, m) if has_u else nan for q, m in zip(uq, un)],
            })
        return out

    def summary(self) -> List[Dict[str, object]]:
        """ONE read: per alpha ``{alpha, rows, nan_rows, coverage, mean_size, empty, singleton, singleton_accuracy, size_hist, class_n,
        class_coverage, coverage_by_size, min_coverage_by_size, u_by_size}``."""
        return self.unpack(self.packed().cpu().numpy(), self.alphas, self.K, self.has_labels, self.has_u)


def predict_sets(probs: torch.Tensor, fit: ConformalFit, labels: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                 mondrian: bool = False) -> ConformalSets:
    """The prediction sets of ``probs`` (M, K_real) fp32 under ``fit`` -- its score settings, its thresholds: the marginal ones, or with
    ``mondrian`` each class its own --, and their tallies against ``labels`` (M,) and the uncertainty ``u`` (M,) fp32 when given.  No
    host synchronisation."""
    if not isinstance(fit, ConformalFit):
        raise ValueError(f"fit must be a ConformalFit (conformal.calibrate), got {fit!r}")
    if not isinstance(mondrian, (bool, np.bool_)):
        raise ValueError(f"mondrian must be a bool, got {mondrian!r}")
    _require_cuda(probs, labels, u, fit.qhat)
    M, K = _check_rows(probs, labels, u)
    if K != fit.K:
        raise ValueError(f"the fit was calibrated on {fit.K} classes, probs has {K}")
    table, _, _ = _scores(probs, None, fit.settings, SALT_PREDICT)
    dev, A = probs.device, len(fit.alphas)
    with torch.cuda.device(dev):
        labels = None if labels is None else labels.to(torch.int32).contiguous()
        u = None if u is None else _f32(u)
        masks = torch.empty(A, M, dtype=torch.uint16, device=dev)
        tallies = torch.empty(A, tally_words(K), dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().pasn_conformal_sets(_lib.ptr(table), _lib.ptr(fit.qhat), _lib.ptr(labels), _lib.ptr(u), M, K, A, int(mondrian),
                                                  _lib.ptr(masks), _lib.ptr(tallies), _lib.current_stream()))
    return ConformalSets(masks, tallies, fit.alphas, K, fit.kind, mondrian, labels is not None, u is not None)


def mask_classes(mask: int, K: int) -> List[int]:
    """The class indices of one mask word."""
    return [k for k in range(K) if (int(mask) >> k) & 1]
