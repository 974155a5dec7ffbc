"""CPU: conformal prediction -- the numpy restatement of tests/conformal_cases.py (what the GPU tests hold the kernels to) against cases
worked out by hand, the statistical validity of the definition itself, and the C-ABI / Python surface with its argument checks."""
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import calibration_cases as cc
import conformal_cases as cf
import protoasnet_amd
from protoasnet_amd import _lib, conformal, selective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_conformal_scores", "pasn_conformal_workspace_bytes", "pasn_conformal_quantiles", "pasn_conformal_tally_words",
               "pasn_conformal_sets")

# eighths: exact in fp32, and every sum and product below is exact in fp64
HAND_PROBS = np.array([[0.75, 0.125, 0.125], [0.125, 0.75, 0.125], [0.375, 0.375, 0.25], [0.25, 0.375, 0.375]], dtype=np.float32)
HAND_LABELS = np.array([0, 0, 0, 2])
INF = float("inf")


# ---- the restatement by hand ---------------------------------------------------------------------------------------------------------------
def test_four_rows_three_classes_by_hand():
    """Deterministic APS: row 0 ranks 0, 1, 2 (the tie of classes 1 and 2 goes to the lower class), row 1 ranks 1, 0, 2, row 2 ranks
    0, 1, 2 (a tie for the top), row 3 ranks 1, 2, 0.  Own-label scores 0.75, 0.875, 0.375 and (label 2) 0.75."""
    s = cf.scores_ref(HAND_PROBS, "aps", randomized=False)
    assert s.dtype == np.float32 and s.tolist() == [[0.75, 0.875, 1.0], [0.875, 0.75, 1.0], [0.375, 0.75, 1.0], [1.0, 0.375, 0.75]]
    assert cf.ranking(HAND_PROBS).tolist() == [[0, 1, 2], [1, 0, 2], [0, 1, 2], [1, 2, 0]]
    assert cf.scores_ref(HAND_PROBS, "lac").tolist() == (1.0 - HAND_PROBS.astype(np.float64)).tolist()
    # RAPS: + lam * max(0, rank - k_reg): with k_reg = 1 the second rank pays lam, the third 2 lam
    assert cf.scores_ref(HAND_PROBS, "raps", randomized=False, lam=0.25, k_reg=1)[0].tolist() == [0.75, 1.125, 1.5]
    assert cf.scores_ref(HAND_PROBS, "raps", randomized=False, lam=0.25, k_reg=2)[3].tolist() == [1.25, 0.375, 0.75]
    assert np.array_equal(cf.scores_ref(HAND_PROBS, "raps", randomized=False, lam=0.0, k_reg=0), s)
    st = cf.strata_ref(HAND_PROBS, HAND_LABELS)
    assert st.tolist() == [0, 0, 0, 2] and cf.own_ref(s, st).tolist() == [0.75, 0.875, 0.375, 0.75]
    # stratum 0 holds 0.375 0.75 0.75 0.875: r = ceil(5 * 0.5) = 3, ceil(5 * 0.75) = 4, ceil(5 * 0.9) = 5 > 4
    fit = cf.calibrate_ref(HAND_PROBS, HAND_LABELS, [0.5, 0.25, 0.1], "aps", randomized=False)
    assert fit["n"].tolist() == [4, 3, 0, 1]
    assert fit["r"].tolist() == [[3, 4, 5], [2, 3, 4], [1, 1, 1], [1, 2, 2]]
    # class 0 holds 0.375 0.75 0.875, class 1 nothing (+inf whatever alpha), class 2 the one 0.75 (r = 2 > 1 at alpha 0.25)
    assert fit["qhat"].tolist() == [[0.75, 0.875, INF], [0.75, 0.875, INF], [INF, INF, INF], [0.75, INF, INF]]
    # the sets of the same rows under the marginal thresholds: {0}, {1}, {0, 1}, {1, 2} at 0.75
    masks, t = cf.sets_ref(s, fit["qhat"], HAND_LABELS)
    assert masks.dtype == np.uint16 and masks.tolist() == [[1, 2, 3, 6], [3, 3, 3, 6], [7, 7, 7, 7]]
    K = 3
    assert t.shape == (3, cf.tally_words(K)) and cf.tally_words(K) == 3 + 16 + 6
    rows, covered, nan_rows = t[0, :3]
    assert (rows, covered, nan_rows) == (4, 3, 0)
    assert t[0, 3:7].tolist() == [0, 2, 2, 0] and t[0, 7:11].tolist() == [0, 1, 2, 0]  # size_hist, covered_by_size
    assert t[0, 11:19].tolist() == [0] * 8  # no u
    assert t[0, 19:22].tolist() == [3, 0, 1] and t[0, 22:25].tolist() == [2, 0, 1]  # class_n, class_covered
    assert t[2, :3].tolist() == [4, 4, 0] and t[2, 3:7].tolist() == [0, 0, 0, 4]  # +inf: the full label set
    sm = cf.summary_ref(t, [0.5, 0.25, 0.1], K, has_u=False)
    assert sm[0]["coverage"] == 0.75 and sm[0]["mean_size"] == 1.5 and sm[0]["empty"] == 0.0 and sm[0]["singleton"] == 0.5
    assert sm[0]["singleton_accuracy"] == 0.5 and sm[0]["class_coverage"][0] == 2 / 3 and np.isnan(sm[0]["class_coverage"][1])
    assert sm[0]["coverage_by_size"][1:3] == [0.5, 1.0] and sm[0]["min_coverage_by_size"] == 0.5 and np.isnan(sm[0]["coverage_by_size"][0])
    assert np.isnan(sm[0]["u_by_size"]).all()
    # Mondrian: class 1's threshold is +inf (an empty stratum): class 1 is in every set; class 2's is 0.75 at alpha 0.5
    masks, t = cf.sets_ref(s, fit["qhat"], HAND_LABELS, mondrian=True)
    assert masks[0].tolist() == [1 | 2, 2, 1 | 2, 2 | 4] and t[0, :2].tolist() == [4, 3]
    # the uncertainty by set size: q = u 2^32, summed as integers
    masks, t = cf.sets_ref(s, fit["qhat"], HAND_LABELS, u=np.array([0.5, 0.25, 1.0, np.nan], np.float32))
    assert t[0, 11:15].tolist() == [0, 3 << 30, 1 << 32, 0] and t[0, 15:19].tolist() == [0, 2, 1, 0]
    assert cf.summary_ref(t, [0.5, 0.25, 0.1], K)[0]["u_by_size"][1:3] == [0.375, 1.0]
    # without labels: masks and the size histogram only
    masks2, t = cf.sets_ref(s, fit["qhat"], None)
    assert np.array_equal(masks2, masks) and t[0, :3].tolist() == [4, 0, 0] and t[0, 3:7].tolist() == [0, 2, 2, 0] and t[0, 7:11].sum() == 0
    assert t[0, 19:].sum() == 0 and np.isnan(cf.summary_ref(t, [0.5, 0.25, 0.1], K, has_labels=False)[0]["coverage"])


def test_nan_and_padding_rows_enter_nothing():
    probs = np.concatenate([HAND_PROBS, [[np.nan, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25], [0.25, np.nan, 0.5]]]).astype(np.float32)
    labels = np.concatenate([HAND_LABELS, [0, -1, 3, -1]])
    st = cf.strata_ref(probs, labels)
    assert st.tolist() == [0, 0, 0, 2, cf.NAN, cf.PAD, cf.PAD, cf.NAN]
    for kind in cf.KINDS:
        s = cf.scores_ref(probs, kind, randomized=False)
        assert np.isnan(s[4]).all() and np.isnan(s[7]).all() and not np.isnan(s[[0, 1, 2, 3, 5, 6]]).any()
    fit = cf.calibrate_ref(probs, labels, [0.5], "aps", randomized=False)
    want = cf.calibrate_ref(HAND_PROBS, HAND_LABELS, [0.5], "aps", randomized=False)
    assert all(np.array_equal(fit[k], want[k]) for k in fit)
    s = cf.scores_ref(probs, "aps", randomized=False)
    masks, t = cf.sets_ref(s, np.full((4, 1), np.inf, np.float32), labels)
    assert masks[0].tolist() == [7, 7, 7, 7, 0, 7, 7, 0]  # +inf admits every class, but a NaN row keeps the empty mask
    assert t[0, :3].tolist() == [4, 4, 2] and t[0, 3:7].tolist() == [0, 0, 0, 4]
    assert np.isnan(cf.own_ref(s, st)[4:]).all()


def test_the_rank_rule_and_too_few_rows():
    v = np.array([0.5, 0.25, 0.75, 0.25], np.float32)
    assert cf.quantile_ref(v, 0.5) == (np.float32(0.5), 4, 3)  # ceil(5 * 0.5) = 3: the third smallest of 0.25 0.25 0.5 0.75
    assert cf.quantile_ref(v, 0.75) == (np.float32(0.25), 4, 2)  # ties: a value, whichever of the two rows it comes from
    assert cf.quantile_ref(v, 0.2) == (np.float32(0.75), 4, 4) and cf.quantile_ref(v, 0.19) == (np.float32(np.inf), 4, 5)
    assert cf.quantile_ref(v[:0], 0.9) == (np.float32(np.inf), 0, 1)
    # n + 1 = 10 at alpha 0.1: (double)10 * (1.0 - 0.1) is exactly 9.0, r = 9 = n; at n = 8 r = ceil(8.1) = 9 > 8
    assert cf.quantile_ref(np.arange(9, dtype=np.float32), 0.1) == (np.float32(8.0), 9, 9)
    assert cf.quantile_ref(np.arange(8, dtype=np.float32), 0.1)[0] == np.inf
    # the uniforms: one per row, other numbers under another salt or seed, always in [0, 1)
    u0, u1 = cf.uniforms(1000, 7, 0), cf.uniforms(1000, 7, 1)
    assert (u0 != u1).mean() > 0.99 and (cf.uniforms(1000, 8, 0) != u0).mean() > 0.99 and 0 <= u0.min() and u0.max() < 1
    assert abs(u0.mean() - 0.5) < 0.05 and np.array_equal(cf.uniforms(10, 7, 0), u0[:10])
    assert np.array_equal(cf.uniforms(5, 7 + (3 << 32), 0) != cf.uniforms(5, 7, 0), np.ones(5, bool))  # the high seed word is read


def test_the_vectorised_scores_are_the_row_by_row_ones():
    probs, labels = cf.conf_case(300, 5, seed=2)
    probs[7, 1] = probs[7, 3]  # a tie inside a random row
    U = cf.uniforms(300, 9, 1)
    for kind, rnd in (("aps", True), ("aps", False), ("raps", True)):
        got = cf.scores_ref(probs, kind, rnd, 9, 0.02, 2, salt=1)
        for i in range(300):
            p = probs[i].astype(np.float64)
            if np.isnan(p).any():
                assert np.isnan(got[i]).all()
                continue
            order = sorted(range(5), key=lambda k: (-p[k], k))
            acc = 0.0
            for rank, k in enumerate(order, 1):
                s = acc + (U[i] if rnd else 1.0) * p[k]
                if kind == "raps":
                    s = s + 0.02 * max(0, rank - 2)
                assert got[i, k] == np.float32(s), (kind, i, k)
                acc = acc + p[k]
    assert np.array_equal(cf.scores_ref(probs, "aps", False)[5], np.array([1, 1, 1, 1, 1], np.float32))  # top probability exactly 1.0f


def test_what_a_fused_product_would_change_at_5000_rows():
    """The contraction rule: ``acc + U p`` rounded ONCE (an FMA) is another fp64 number than the definition's two roundings in a good part
    of the scores of the 5000-row cases -- by one fp64 ulp.  MEASURED here, and asserted so that nobody relies on the opposite: after the
    one rounding to fp32 NO score of these cases differs (an fp64 ulp moves an fp32 rounding only when the sum lies within 2^-29 of a
    rounding boundary), so the bitwise GPU comparison of fp32 scores does not by itself prove the absence of contraction at these
    shapes.  The rule is pinned in the source instead (``#pragma clang fp contract(off)`` in every scoring function, checked with the
    symbols below)."""
    for K in (4, 16):
        probs, _ = cf.conf_case(5000, K, seed=K)
        kw = dict(kind="aps", randomized=True, seed=3, salt=0)
        plain, fused = cf.scores_ref(probs, rounded=False, **kw), cf.scores_ref(probs, rounded=False, fused=True, **kw)
        ok = ~np.isnan(plain)
        differ = (plain != fused) & ok
        print(f"K={K}: {differ.sum()} of {ok.sum()} fp64 scores differ under a fused product")
        assert 0 < differ.sum() < ok.sum() // 2, (K, differ.sum())  # (a 56-bit product: its own rounding shows in a few scores in 100)
        assert (np.abs(plain[differ] - fused[differ]) <= np.spacing(np.maximum(plain[differ], fused[differ]))).all()  # the last bit
        with np.errstate(invalid="ignore"):
            assert np.array_equal(plain.astype(np.float32), fused.astype(np.float32), equal_nan=True)
        assert np.array_equal(plain.astype(np.float32), cf.scores_ref(probs, **kw), equal_nan=True)
    # without the uniform the product is exact, and the fused sum is the plain one
    probs, _ = cf.conf_case(500, 4, seed=1)
    assert np.array_equal(cf.scores_ref(probs, "aps", False), cf.scores_ref(probs, "aps", False, fused=True), equal_nan=True)


# ---- the definition is valid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 4])
def test_marginal_coverage_is_what_the_definition_promises(K):
    """Calibrated on 2000 rows and predicted on 4000 others (seed 7, lam 0.01, k_reg 2): the marginal coverage of lac, randomised aps and
    randomised raps lies within 3 sqrt(alpha (1 - alpha) (1 / n_test + 1 / n_cal)) of 1 - alpha.  Deterministic aps is only required to
    cover at least 1 - alpha minus the band: on these over-confident rows the cumulative mass of the last ranks rounds to exactly 1.0
    in fp32, so at K = 4, alpha = 0.05 and at K = 3, alpha = 0.05 and 0.1 the threshold IS 1.0 and the sets are the full label set --
    coverage 1, which is correct behaviour of a deterministic score (it over-covers), not an error."""
    alphas = [0.05, 0.1, 0.2]
    pc, lc = cc.prob_case(2000, K, seed=11, pad=True)
    pt, lt = cc.prob_case(4000, K, seed=12, pad=True)
    n_cal, n_test = int(((lc >= 0) & (lc < K)).sum()), int(((lt >= 0) & (lt < K)).sum())
    for kind, rnd in (("lac", False), ("aps", True), ("raps", True), ("aps", False)):
        kw = dict(kind=kind, randomized=rnd, seed=7, lam=0.01, k_reg=2)
        fit = cf.calibrate_ref(pc, lc, alphas, **kw)
        assert fit["n"][0] == n_cal
        masks, t = cf.predict_ref(pt, fit, alphas, lt, **kw)
        for a, alpha in enumerate(alphas):
            assert t[a, 0] == n_test
            cov = t[a, 1] / t[a, 0]
            band = 3 * math.sqrt(alpha * (1 - alpha) * (1 / n_test + 1 / n_cal))
            print(f"K={K} {kind} randomized={rnd} alpha={alpha}: qhat={fit['qhat'][0, a]:.6f} coverage={cov:.4f} "
                  f"deviation={cov - (1 - alpha):+.4f} band={band:.4f}")
            if kind == "aps" and not rnd:
                assert cov >= 1 - alpha - band, (K, alpha, cov)
                if (K, alpha) in ((4, 0.05), (3, 0.05), (3, 0.1)):
                    assert fit["qhat"][0, a] == 1.0 and cov == 1.0 and t[a, 3 + K] == n_test  # the full label set
            else:
                assert abs(cov - (1 - alpha)) <= band, (K, kind, alpha, cov, band)


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "protoasnet_amd.h")) as f:
        raw = f.read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", protoasnet_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pasn_\w+)", nm))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
        assert getattr(lib, name) is not None
    assert "conformal" in protoasnet_amd.__all__ and protoasnet_amd.conformal is conformal  # exported lazily, like its neighbours
    assert int(re.search(r"#define PASN_CONFORMAL_MAX_ALPHAS (\d+)", header).group(1)) == conformal.MAX_ALPHAS == 8
    assert [int(re.search(rf"#define PASN_CONFORMAL_{k.upper()} (\d+)", header).group(1)) for k in conformal.KINDS] == [0, 1, 2]
    assert conformal.KINDS == cf.KINDS
    for K in (2, 4, 16):
        assert lib.pasn_conformal_tally_words(K) == conformal.tally_words(K) == cf.tally_words(K)
    assert lib.pasn_conformal_tally_words(1) == 0 and lib.pasn_conformal_tally_words(17) == 0
    with open(os.path.join(REPO, "protoasnet_amd", "build.py")) as f:
        assert '"conformal.hip"' in f.read()
    with open(os.path.join(REPO, "protoasnet_amd", "csrc", "conformal.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "asm" not in src  # plain C++: no inline assembly at all


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first
    half = (ctypes.c_double * 8)(*([0.5] * 8))

    def scores(M=100, K_real=3, kind=1, randomized=1, lam=0.0, k_reg=1, **null):
        p = dict(probs=fake, labels=fake, scores=fake, own=fake, stratum=fake)
        p.update(null)
        return lib.pasn_conformal_scores(p["probs"], p["labels"], M, K_real, kind, randomized, 7, 0, lam, k_reg, p["scores"], p["own"],
                                         p["stratum"], 0)

    def quant(M=100, K_real=3, A=3, alphas=half, **null):
        p = dict(own=fake, stratum=fake, qhat=fake, n=fake, r=fake, workspace=fake)
        p.update(null)
        return lib.pasn_conformal_quantiles(p["own"], p["stratum"], M, K_real, A, alphas, p["qhat"], p["n"], p["r"], p["workspace"], 0)

    def sets(M=100, K_real=3, A=3, mondrian=0, **null):
        p = dict(scores=fake, qhat=fake, labels=0, u=0, masks=fake, tallies=fake)
        p.update(null)
        return lib.pasn_conformal_sets(p["scores"], p["qhat"], p["labels"], p["u"], M, K_real, A, mondrian, p["masks"], p["tallies"], 0)

    size = lib.pasn_conformal_workspace_bytes
    assert size(100, 3, 3) > 0 and size(100, 3, 3) == size(1 << 20, 3, 3) and size(100, 3, 3) % 16 == 0  # it does not grow with M
    assert size(100, 3, 3) == 4 * 4 * 3 * 256 * 4 + 2 * 4 * 3 * 8  # four passes of (1 + K) x A x 256 counters, two target states
    for call in (scores, quant, sets):
        for bad in (dict(K_real=1), dict(K_real=17), dict(M=0), dict(M=(1 << 20) + 1)):
            assert call(**bad) == 1, (call.__name__, bad)
    with pytest.raises(ValueError, match="K_real"):
        _lib.check(sets(K_real=17))
    for call in (quant, sets):
        for A in (0, 9):
            assert call(A=A) == 1, (call.__name__, A)
    assert size(100, 1, 3) == 0 and size(100, 17, 3) == 0 and size(0, 3, 3) == 0 and size((1 << 20) + 1, 3, 3) == 0
    assert size(100, 3, 0) == 0 and size(100, 3, 9) == 0
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert quant(alphas=(ctypes.c_double * 3)(0.1, bad, 0.2)) == 1, bad
    with pytest.raises(ValueError, match="alpha"):
        _lib.check(quant(alphas=(ctypes.c_double * 3)(0.1, 1.0, 0.2)))
    assert quant(alphas=None) == 1
    for bad in (dict(kind=-1), dict(kind=3), dict(randomized=2), dict(lam=-0.5), dict(lam=float("nan")), dict(lam=INF), dict(k_reg=-1)):
        assert scores(**bad) == 1, bad
    with pytest.raises(ValueError, match="lam"):
        _lib.check(scores(lam=-0.5))
    with pytest.raises(ValueError, match="kind"):
        _lib.check(scores(kind=3))
    for k in ("probs", "scores"):
        assert scores(**{k: 0}) == 1, k
    for k in ("labels", "own", "stratum"):  # together or not at all
        assert scores(**{k: 0}) == 1, k
    for k in ("own", "stratum", "qhat", "n", "r", "workspace"):
        assert quant(**{k: 0}) == 1, k
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(quant(workspace=0))
    assert quant(workspace=264) == 1  # misaligned
    with pytest.raises(ValueError, match="misaligned"):
        _lib.check(quant(workspace=264))
    for k in ("scores", "qhat", "masks", "tallies"):
        assert sets(**{k: 0}) == 1, k
    assert sets(mondrian=2) == 1 and sets(mondrian=-1) == 1


def test_python_surface_checks_its_arguments():
    probs, labels = torch.rand(4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        conformal.scores(probs)
    with pytest.raises(RuntimeError, match="GPU only"):
        conformal.calibrate(probs, labels)
    for bad in (dict(kind="APS"), dict(kind=1), dict(randomized=1), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(lam=-1.0),
                dict(lam=float("nan")), dict(lam="0"), dict(k_reg=-1), dict(k_reg=1.5), dict(k_reg=True)):
        with pytest.raises(ValueError):
            conformal.scores(probs, **bad)
        with pytest.raises(ValueError):
            conformal.calibrate(probs, labels, **bad)
    for bad in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="salt"):
            conformal.scores(probs, salt=bad)
    for bad in ((), (0.0,), (1.0,), (0.1, 1.5), (float("nan"),), [0.1] * 9, 0.1, None):
        with pytest.raises(ValueError, match="alphas"):
            conformal.calibrate(probs, labels, alphas=bad)
    with pytest.raises(ValueError, match="labels"):
        conformal.calibrate(probs, None)
    with pytest.raises(ValueError, match="ConformalFit"):
        conformal.predict_sets(probs, {"qhat": 1.0})
    fit = conformal.ConformalFit(torch.full((4, 2), 0.5), torch.zeros(4, dtype=torch.int64), torch.ones(4, 2, dtype=torch.int64), (0.1, 0.2),
                                 conformal.check_settings("raps", True, 5, 0.01, 2))
    assert fit.K == 3 and fit.kind == "raps" and fit.alphas == [0.1, 0.2]
    with pytest.raises(RuntimeError, match="GPU only"):
        conformal.predict_sets(probs, fit)
    with pytest.raises(ValueError, match="mondrian"):
        conformal.predict_sets(probs, fit, mondrian=1)
    # a fit travels through its state dict with its settings: prediction can not be run with other ones
    sd = fit.state_dict()
    assert {k: sd[k] for k in ("kind", "randomized", "seed", "lam", "k_reg", "alphas")} == {
        "kind": "raps", "randomized": True, "seed": 5, "lam": 0.01, "k_reg": 2, "alphas": [0.1, 0.2]}
    back = conformal.ConformalFit.from_state_dict(sd, device="cpu")
    assert back.settings == fit.settings and back.alphas == fit.alphas and torch.equal(back.qhat, fit.qhat) and torch.equal(back.r, fit.r)
    assert back.read() == {"kind": "raps", "alphas": [0.1, 0.2], "qhat": [0.5, 0.5], "qhat_per_class": [[0.5, 0.5]] * 3, "n": 0,
                           "n_per_class": [0, 0, 0], "r": [1, 1]}
    for bad in (dict(sd, kind="x"), dict(sd, alphas=[0.1]), dict(sd, n=torch.zeros(3, dtype=torch.int64)), dict(sd, lam=-1.0)):
        with pytest.raises(ValueError):
            conformal.ConformalFit.from_state_dict(bad, device="cpu")
    # shapes and sizes are checked on the host, after the device check
    assert conformal._check_rows(probs, labels) == (4, 3)
    for p, l, u in ((torch.rand(4), None, None), (probs, labels[:3], None), (probs, labels, torch.rand(3)), (torch.rand(4, 1), None, None),
                    (torch.rand(4, 17), None, None), (torch.rand(0, 3), None, None)):
        with pytest.raises(ValueError):
            conformal._check_rows(p, l, u)
    assert conformal.mask_classes(0b1011, 4) == [0, 1, 3] and conformal.mask_classes(1 << 15, 16) == [15] and conformal.mask_classes(0, 4) == []
    # a summary is host arithmetic on the one vector that was read, and it is the restatement's
    probs_c, labels_c = cf.conf_case(200, 4, seed=3)
    fit_c = cf.calibrate_ref(probs_c, labels_c, [0.1, 0.3], "lac")
    _, t = cf.predict_ref(probs_c, fit_c, [0.1, 0.3], labels_c, cf.u_case(200, 4), kind="lac")
    got, want = conformal.ConformalSets.unpack(t, [0.1, 0.3], 4), cf.summary_ref(t, [0.1, 0.3], 4)
    assert repr(got) == repr(want) and got[0]["rows"] > 100 and got[0]["nan_rows"] == 2
    assert repr(conformal.ConformalSets.unpack(t.astype(np.float64), [0.1, 0.3], 4)) == repr(want)  # the fp64 copy of a joined read
    # finish and the trainer check their own arguments before they look at the rows
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    for bad in (dict(conformal="fitted"), dict(conformal=0.1), dict(conformal=fit, conformal_mondrian=1)):
        with pytest.raises(ValueError, match="conformal"):
            sel.finish(**bad)
    from protoasnet_amd.trainer import DPTrainer

    t = DPTrainer.__new__(DPTrainer)
    t.conformal_fit = t.temperature_fit = None
    with pytest.raises(ValueError, match="fit_conformal"):
        t.evaluate_selective("test", conformal="fitted")
    with pytest.raises(ValueError, match="conformal"):
        t.evaluate_selective("test", conformal="fit")
    for bad in (dict(level="study"), dict(alphas=(1.0,)), dict(kind="top"), dict(temperature="fitted"), dict(temperature="x"), dict(lam=-1)):
        with pytest.raises(ValueError):
            t.fit_conformal("val", **bad)


def test_the_default_call_is_unchanged(monkeypatch):
    """``conformal=None`` (the default) adds no key and reaches nothing of the new module: ``finish`` on stubbed device functions, each of
    which is reached exactly as often as before; the trainer passes the keyword on only when it is given."""
    sig = inspect.signature(selective.SelectiveEvaluator.finish)
    assert [sig.parameters[k].default for k in ("conformal", "conformal_mondrian")] == [None, False]
    assert list(sig.parameters)[-2:] == ["conformal", "conformal_mondrian"]  # behind every keyword the call had
    from protoasnet_amd.trainer import DPTrainer

    sig = inspect.signature(DPTrainer.evaluate_selective)
    assert [sig.parameters[k].default for k in ("conformal", "conformal_mondrian")] == [None, False]
    sig = inspect.signature(DPTrainer.fit_conformal)
    assert [sig.parameters[k].default for k in ("mode", "alphas", "kind", "level", "temperature")] == ["val", (0.1,), "aps", "cine", None]
    cs = [1.0, 0.5]
    calls = []

    class RC:
        def packed(self, coverages):
            return torch.tensor([0.5, 1.0, 0.4, 0.9, 0.3, 0.8, 0.75, 0.25, 6, 3, 0.25, 0.7, 6, 1], dtype=torch.float64)

    class Ev:
        K_real, rows = 2, 6
        probs, labels, logits = torch.zeros(6, 2), torch.zeros(6, dtype=torch.int32), torch.zeros(6, 3)

    def counted(name, result):
        def f(*a, **k):
            calls.append(name)
            return result
        return f

    def not_reached(*a, **k):
        raise AssertionError("the defaults must not reach the conformal module")

    monkeypatch.setattr(selective, "uncertainty", counted("uncertainty", torch.zeros(6)))
    monkeypatch.setattr(selective, "risk_coverage", counted("risk_coverage", RC()))
    monkeypatch.setattr(_lib, "lib", counted("lib", None))  # any library call of finish itself would go through here
    for name in ("scores", "_scores", "calibrate", "predict_sets"):
        monkeypatch.setattr(conformal, name, not_reached)
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    sel.ev, sel.keys, sel.abstain, sel.score, sel.ab_logitpath = Ev(), list("aabbcc"), True, "auto", "joined"
    res = sel.finish(cs, level="clip")
    assert calls == ["uncertainty", "risk_coverage"]  # the two device steps of the call as it was, once each, and no other library call
    assert "conformal" not in res and sorted(res) == sorted(
        ["aurc", "error_auroc", "rows", "nan_rows"] + [f"{n}@{c}" for n in ("accuracy", "bal_accuracy", "f1_mean", "threshold") for c in ("1", "0.5")])
    assert res == sel.finish(cs, level="clip", conformal=None, conformal_mondrian=False)
    fit = conformal.ConformalFit(torch.full((3, 1), 0.5), torch.zeros(3, dtype=torch.int64), torch.ones(3, 1, dtype=torch.int64), (0.1,),
                                 conformal.check_settings())
    with pytest.raises(AssertionError, match="must not reach"):
        sel.finish(cs, level="clip", conformal=fit)
    with pytest.raises(ValueError, match="calibrated on 3 classes"):
        sel.finish(cs, level="clip", conformal=conformal.ConformalFit(torch.zeros(4, 1), torch.zeros(4, dtype=torch.int64),
                                                                      torch.ones(4, 1, dtype=torch.int64), (0.1,), conformal.check_settings()))
    # the trainer hands finish exactly the keywords it handed it before
    seen = []

    class Sweep:
        def finish(self, *a, **k):
            seen.append(sorted(k))
            return {"aurc": 0.0, "error_auroc": 0.0}

    t = DPTrainer.__new__(DPTrainer)
    t.conformal_fit = t.temperature_fit = None
    t.config, t.current_epoch, t.log = {}, 0, lambda *a, **k: None
    t._selective_sweep = lambda mode, score="auto": Sweep()
    t.evaluate_selective("test", level="clip")
    assert seen == [["bootstrap", "calibration", "confidence", "seed", "temperature", "unit"]]
