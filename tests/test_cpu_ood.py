"""CPU: out-of-distribution detection -- the numpy restatement of tests/ood_cases.py (what the GPU tests hold the kernels to) against
cases worked out by hand, the validity of the threshold rule itself, and the C-ABI / Python surface with its argument checks."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ood_cases as oc
import protoasnet_amd
from protoasnet_amd import _lib, build, ood

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_ood_head_scores", "pasn_ood_knn_workspace_bytes", "pasn_ood_knn", "pasn_ood_rows_normalize", "pasn_ood_moment_chunk",
               "pasn_ood_moments_workspace_bytes", "pasn_ood_moments", "pasn_ood_mahalanobis", "pasn_ood_tally")
INF, NAN = float("inf"), float("nan")


# ---- the restatement by hand ---------------------------------------------------------------------------------------------------------------
def test_knn_by_hand():
    """One query at the origin against (3, 4), (1, 0), (0, 1) and a NaN row: d = 25, 1, 1, not eligible."""
    q = np.array([[0.0, 0.0]], np.float32)
    bank = np.array([[3.0, 4.0], [1.0, 0.0], [0.0, 1.0], [NAN, 0.0]], np.float32)
    assert oc.dist_ref(q, bank[:3]).tolist() == [[25.0, 1.0, 1.0]]
    d, i, st = oc.knn_ref(q, bank, 3)
    assert d.tolist() == [[1.0, 1.0, 25.0]] and i.tolist() == [[1, 2, 0]] and st.tolist() == [1, 0]  # the tie goes to the lower index
    d, i, _ = oc.knn_ref(q, bank, 5)
    assert d.tolist() == [[1.0, 1.0, 25.0, INF, INF]] and i.tolist() == [[1, 2, 0, -1, -1]]  # three eligible rows: the rest is fill
    # the bank against itself, leave-one-out: row 0 sees rows 1 and 2 at 4 + 16 = 20 and 9 + 9 = 18
    d, i, st = oc.knn_ref(bank, bank, 2, self_base=0)
    assert d[0].tolist() == [18.0, 20.0] and i[0].tolist() == [2, 1] and d[1].tolist() == [2.0, 20.0] and i[1].tolist() == [2, 0]
    assert np.isnan(d[3]).all() and i[3].tolist() == [-1, -1] and st.tolist() == [1, 1]  # a NaN query
    # without leave-one-out a row is its own nearest neighbour at 0; a slice of the bank with self_base = 1
    assert oc.knn_ref(bank[:3], bank[:3], 1)[1][:, 0].tolist() == [0, 1, 2]
    assert oc.knn_ref(bank[1:3], bank[:3], 1, self_base=1)[1][:, 0].tolist() == [2, 1]
    # inf: every finite row is at +inf from an inf query (ties to the lower index), inf - inf is NaN and not eligible
    qi = np.array([[INF, 0.0]], np.float32)
    bi = np.array([[1.0, 0.0], [INF, 0.0], [2.0, 0.0]], np.float32)
    d, i, st = oc.knn_ref(qi, bi, 3)
    assert d.tolist() == [[INF, INF, INF]] and i.tolist() == [[0, 2, -1]] and st.tolist() == [0, 0]


def test_head_scores_and_normalize_by_hand():
    sim = np.array([[0.25, 0.75, 0.5], [NAN, 0.5, 0.25], [-1.0, -2.0, -0.5]], np.float32)
    m = oc.maxsim_ref(sim)
    assert m[0] == 0.25 and np.isnan(m[1]) and m[2] == 1.5
    lg = np.array([[0.0, 0.0, 9.0], [1.0, 1.0, 1.0], [NAN, 0.0, 0.0]], np.float32)
    e = oc.energy_ref(lg, 2)
    assert e[0] == np.float32(-np.log(2.0)) and e[1] == np.float32(-(1.0 + np.log(2.0))) and np.isnan(e[2])  # the third logit is not read
    assert oc.energy_ref(lg, 3)[1] == np.float32(-(1.0 + np.log(3.0)))
    x = np.array([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]], np.float32)
    assert oc.normalize_ref(x).tolist() == [[np.float32(0.6), np.float32(0.8)], [0.0, 0.0], [0.0, -1.0]]


def test_moments_by_hand():
    """Quarters are exact.  Rows 0 and 2 are class 0, row 1 class 1, row 3 is padding, row 4 holds a NaN."""
    x = np.array([[0.5, 0.25], [1.0, -1.0], [0.25, 0.25], [7.0, 7.0], [NAN, 1.0]], np.float32)
    labels = np.array([0, 1, 0, -1, 1])
    mo = oc.moments_ref(x, labels, 3)
    assert mo["n"].tolist() == [2, 1, 0] and mo["skipped"].tolist() == [1, 1]
    assert mo["sum"].tolist() == [[0.75, 0.5], [1.0, -1.0], [0.0, 0.0]]
    assert mo["scatter"].tolist() == [[0.25 + 1.0 + 0.0625, 0.125 - 1.0 + 0.0625], [0.125 - 1.0 + 0.0625, 0.0625 + 1.0 + 0.0625]]
    twice = oc.moments_ref(x, labels, 3, prev=mo)
    assert twice["n"].tolist() == [4, 2, 0] and np.array_equal(twice["scatter"], 2 * mo["scatter"])
    # the chunk cut shows in the order of the additions only: the same numbers here, where every sum is exact
    assert all(np.array_equal(oc.moments_ref(x, labels, 3, chunk=2)[k], mo[k]) for k in mo)
    # two well separated classes in one dimension: mu = 0 and 10, pooled variance ((1 + 1) + (1 + 1)) / (4 - 2) = 2, W = 1 / sqrt(2)
    x1 = np.array([[-1.0], [1.0], [9.0], [11.0]], np.float32)
    m1 = oc.moments_ref(x1, np.array([0, 0, 2, 2]), 3)
    mu, W = oc.gaussian_fit_ref(m1["n"], m1["sum"], m1["scatter"], shrink=0.0)
    assert mu[0, 0] == 0.0 and np.isnan(mu[1, 0]) and mu[2, 0] == 10.0 and abs(W[0, 0] - 2 ** -0.5) < 1e-15
    m, bound, score, arg = oc.mahalanobis_ref(np.array([[2.0], [9.0], [NAN]], np.float32), mu, W)
    assert abs(m[0, 0] - 2.0) < 1e-12 and abs(m[0, 2] - 32.0) < 1e-12 and arg.tolist() == [0, 2, -1]  # class 1 has no rows and never wins
    assert abs(score[1] - 0.5) < 1e-6 and np.isnan(score[2]) and (bound[:2, [0, 2]] < 1e-12).all()
    with pytest.raises(ValueError, match="at least 3"):
        oc.gaussian_fit_ref(np.array([1, 0, 1]), m1["sum"], m1["scatter"])
    mu2, W2 = ood.gaussian_fit(m1["n"], m1["sum"], m1["scatter"], shrink=0.0)  # the host finish of the package is the same arithmetic
    assert np.array_equal(mu2, mu, equal_nan=True) and np.array_equal(W2, W)
    with pytest.raises(ValueError, match="at least 3 valid rows"):
        ood.gaussian_fit(np.array([1, 0, 1]), m1["sum"], m1["scatter"])


def test_thresholds_and_tallies_by_hand():
    s = np.array([0.5, 0.25, 0.75, NAN], np.float32)
    assert oc.threshold_ref(s, 0.5) == (np.float32(0.5), 3, 2, 1)  # r = ceil(4 * 0.5) = 2: the second smallest of 0.25 0.5 0.75
    assert oc.threshold_ref(s, 0.75) == (np.float32(0.75), 3, 3, 1) and oc.threshold_ref(s, 0.9) == (np.float32(INF), 3, 4, 1)
    assert oc.threshold_ref(s[3:], 0.5) == (np.float32(INF), 0, 1, 1)
    # r = ceil((n + 1) tpr) through the routine's arithmetic, 1.0 - (1.0 - tpr): 999 rows at 0.9 select the 900th
    assert oc.threshold_ref(np.arange(999, dtype=np.float32), 0.9)[:3] == (np.float32(899.0), 999, 900)
    scores = np.array([0.25, 0.5, 0.75, NAN, 0.75, 0.25, 9.0], np.float32)
    kind = np.array([0, 0, 0, 0, 1, 1, 2])
    correct = np.array([1, 0, 1, 1, 0, 0, 1])
    flags, t = oc.tally_ref(scores, kind, np.array([0.5, INF], np.float32), correct)
    assert flags.tolist() == [[0, 0, 1, 1, 1, 0, 1], [0, 0, 0, 1, 0, 0, 0]]  # strictly above; a NaN is always flagged; padding gets a flag
    assert dict(zip(oc.TALLY_NAMES, t[0].tolist())) == {"id_rows": 4, "id_flagged": 2, "ood_rows": 2, "ood_flagged": 1, "nan_rows": 1,
                                                        "id_correct_kept": 1, "id_kept": 2, "id_correct_flagged": 2}
    assert t[1].tolist() == [4, 1, 2, 0, 1, 2, 3, 1]
    assert oc.tally_ref(scores, kind, np.array([0.5], np.float32))[1][0].tolist() == [4, 2, 2, 1, 1, 0, 0, 0]
    # AUROC: positives 0.75 and 0.25 against negatives 0.25, 0.5, 0.75 (the NaN row does not enter): (2 + 2 + 1) + (1) = 6 of 12
    assert oc.auroc_ref(scores, kind) == 0.5 and np.isnan(oc.auroc_ref(scores[:4], kind[:4]))
    assert oc.cine_mean_ref(np.array([0.5, 0.25, 1.0], np.float32), np.array([0, 2, 3]), np.array([2, 0, 1])).tolist() == [0.75, 0.25]


def test_a_fused_product_changes_distances_of_the_33_by_1000_case():
    """The contraction rule shows in the numbers: with the product kept exact and ONE rounding per step, some distances of the
    (33, 1000, 40, 10) case of the GPU tests are other floats than the definition's, and so are some of the k-th distances."""
    q, bank = oc.emb_case(33, 40, seed=33), oc.emb_case(1000, 40, seed=1000)
    plain, fused = oc.dist_ref(q, bank), oc.dist_ref(q, bank, fma=True)
    differ = int((plain != fused).sum())
    print(f"{differ} of {plain.size} distances differ under a fused product")
    assert differ > 0
    d0, d1 = oc.knn_ref(q, bank, 10)[0], oc.knn_ref(q, bank, 10, fma=True)[0]
    assert (d0 != d1).any()


# ---- the threshold rule is valid, and the scores point the right way -----------------------------------------------------------------------
def _bank_scores(bank, labels, rows, K, k=5):
    """{knn, mahalanobis}: restatement scores of `rows` against a fit on (bank, labels)."""
    mo = oc.moments_ref(bank, labels, K)
    mu, W = oc.gaussian_fit_ref(mo["n"], mo["sum"], mo["scatter"])
    nb = oc.normalize_ref(bank)
    return {"knn": oc.knn_ref(oc.normalize_ref(rows), nb, k)[0][:, -1], "mahalanobis": oc.mahalanobis_ref(rows, mu, W)[2]}


def test_flag_rate_of_fresh_in_distribution_rows_lies_in_the_band():
    """999 calibration rows at tpr = 0.9: r = 900, and conditional on the calibration draw the flag rate of fresh exchangeable rows is
    Beta(100, 900) distributed: mean 0.1, sd about 0.0095.  20 000 fresh rows of the same mixture must be flagged at 0.1 +- 0.04."""
    E, K = 4, 3
    bank, labels = oc.mixture_case(400, E, K, seed=1)
    cal, _ = oc.mixture_case(999, E, K, seed=2)
    fresh, _ = oc.mixture_case(20000, E, K, seed=3)
    s_cal, s_new = _bank_scores(bank, labels, cal, K), _bank_scores(bank, labels, fresh, K)
    for d in ("knn", "mahalanobis"):
        tau, n, r, nan = oc.threshold_ref(s_cal[d], 0.9)
        assert (n, r, nan) == (999, 900, 0)
        rate = oc.tally_ref(s_new[d], np.zeros(20000), np.array([tau]))[1][0, 1] / 20000
        print(f"{d}: tau {tau:.6f} flag rate {rate:.4f}")
        assert abs(rate - 0.1) <= 0.04, (d, rate)


def test_a_mean_shifted_sample_scores_higher():
    """The sign convention: a sample shifted by two standard deviations on every coordinate gets AUROC > 0.5 from both bank detectors."""
    E, K = 4, 3
    bank, labels = oc.mixture_case(400, E, K, seed=1)
    idr, _ = oc.mixture_case(300, E, K, seed=4)
    far, _ = oc.mixture_case(300, E, K, seed=5, shift=2.0)
    kind = np.concatenate([np.zeros(300), np.ones(300)])
    scores = _bank_scores(bank, labels, np.concatenate([idr, far]), K)
    for d, s in scores.items():
        a = oc.auroc_ref(s, kind)
        print(f"{d}: AUROC {a:.4f}")
        assert a > 0.5, (d, a)
    # energy and maxsim point the same way on their own inputs: a flat logit row / a row far from every prototype is more out-of-distribution
    assert oc.energy_ref(np.array([[0, 0, 0]], np.float32), 3)[0] > oc.energy_ref(np.array([[5, 0, 0]], np.float32), 3)[0]
    assert oc.maxsim_ref(np.array([[0.1, 0.2]], np.float32))[0] > oc.maxsim_ref(np.array([[0.1, 0.9]], np.float32))[0]


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
    assert "ood.hip" in build.SOURCES
    assert "ood" in protoasnet_amd.__all__ and protoasnet_amd.ood is ood  # exported lazily, like its neighbours
    assert lib.pasn_ood_moment_chunk() == ood.moment_chunk() == oc.DEFAULT_CHUNK
    assert ood.TALLY_NAMES == oc.TALLY_NAMES and len(ood.TALLY_NAMES) == ood.TALLY_WORDS == 8
    with open(os.path.join(REPO, "protoasnet_amd", "csrc", "ood.hip")) as f:
        src = f.read()
    assert "#pragma clang fp contract(off)" in src and "asm" not in src and "atomicAdd(float" not in src  # plain C++, no inline assembly


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def head(M=10, P=4, K=4, K_real=3, **null):
        p = dict(sim=fake, logits=fake, maxsim=fake, energy=fake)
        p.update(null)
        return lib.pasn_ood_head_scores(p["sim"], p["logits"], M, P, K, K_real, p["maxsim"], p["energy"], 0)

    def knn(Mq=10, Mb=100, E=8, k=5, self_base=-1, **null):
        p = dict(q=fake, bank=fake, dist=fake, index=fake, status=fake, workspace=fake)
        p.update(null)
        return lib.pasn_ood_knn(p["q"], p["bank"], Mq, Mb, E, k, self_base, p["dist"], p["index"], p["status"], p["workspace"], 0)

    def norm(M=10, E=8, **null):
        p = dict(x=fake, y=fake)
        p.update(null)
        return lib.pasn_ood_rows_normalize(p["x"], M, E, p["y"], 0)

    def mom(M=10, E=8, K=3, accumulate=0, **null):
        p = dict(x=fake, labels=fake, n=fake, sum=fake, scatter=fake, skipped=fake, workspace=fake)
        p.update(null)
        return lib.pasn_ood_moments(p["x"], p["labels"], M, E, K, accumulate, p["n"], p["sum"], p["scatter"], p["skipped"], p["workspace"], 0)

    def maha(M=10, E=8, K=3, **null):
        p = dict(x=fake, mu=fake, W=fake, m=fake, score=fake, argclass=fake)
        p.update(null)
        return lib.pasn_ood_mahalanobis(p["x"], p["mu"], p["W"], M, E, K, p["m"], p["score"], p["argclass"], 0)

    def tally(M=10, A=2, **null):
        p = dict(scores=fake, kind=fake, correct=0, tau=fake, flags=fake, tallies=fake)
        p.update(null)
        return lib.pasn_ood_tally(p["scores"], p["kind"], p["correct"], p["tau"], M, A, p["flags"], p["tallies"], 0)

    for call, bads in (
            (head, (dict(M=0), dict(M=(1 << 20) + 1), dict(P=0), dict(P=4097), dict(K_real=0), dict(K_real=5), dict(maxsim=0, energy=0),
                    dict(sim=0), dict(logits=0))),
            (knn, (dict(Mq=0), dict(Mq=(1 << 20) + 1), dict(Mb=0), dict(Mb=(1 << 24) + 1), dict(E=0), dict(E=1025), dict(k=0), dict(k=65),
                   dict(self_base=-2), dict(self_base=101), dict(q=0), dict(bank=0), dict(dist=0), dict(index=0), dict(status=0),
                   dict(workspace=0), dict(workspace=264))),
            (norm, (dict(M=0), dict(M=(1 << 24) + 1), dict(E=0), dict(E=1025), dict(x=0), dict(y=0))),
            (mom, (dict(M=0), dict(M=(1 << 24) + 1), dict(E=0), dict(E=257), dict(K=0), dict(K=17), dict(accumulate=2), dict(x=0), dict(labels=0),
                   dict(n=0), dict(sum=0), dict(scatter=0), dict(skipped=0), dict(workspace=0), dict(workspace=264))),
            (maha, (dict(M=0), dict(M=(1 << 20) + 1), dict(E=0), dict(E=257), dict(K=0), dict(K=17), dict(x=0), dict(mu=0), dict(W=0), dict(m=0),
                    dict(score=0), dict(argclass=0))),
            (tally, (dict(M=0), dict(M=(1 << 20) + 1), dict(A=0), dict(A=9), dict(scores=0), dict(kind=0), dict(tau=0), dict(flags=0),
                     dict(tallies=0)))):
        for bad in bads:
            assert call(**bad) == 1, (call.__name__, bad)
    with pytest.raises(ValueError, match="k must lie"):
        _lib.check(knn(k=65))
    with pytest.raises(ValueError, match="misaligned"):
        _lib.check(mom(workspace=264))
    with pytest.raises(ValueError, match="E must lie in \\[1, 256\\]"):
        _lib.check(maha(E=257))
    # the size queries: 0 for anything out of range; the kNN workspace holds one (distance, index) list per query and bank chunk
    size = lib.pasn_ood_knn_workspace_bytes
    assert size(10, 100, 8, 5) == 10 * 5 * 8 and size(10, 1000, 8, 5) == 8 * 10 * 5 * 8 and size(10, 1000, 8, 5) % 16 == 0
    assert size(10, 1000, 1024, 5) == size(10, 1000, 8, 5)  # it does not grow with E
    for bad in ((0, 100, 8, 5), ((1 << 20) + 1, 100, 8, 5), (10, 0, 8, 5), (10, (1 << 24) + 1, 8, 5), (10, 100, 0, 5), (10, 100, 1025, 5),
                (10, 100, 8, 0), (10, 100, 8, 65)):
        assert size(*bad) == 0, bad
    msize = lib.pasn_ood_moments_workspace_bytes
    assert msize(1000, 8, 3) >= 1000 * 4 + 5 * 8 and msize(1000, 8, 3) % 16 == 0 and msize(1000, 256, 3) == msize(1000, 8, 3)
    for bad in ((0, 8, 3), ((1 << 24) + 1, 8, 3), (10, 0, 3), (10, 257, 3), (10, 8, 0), (10, 8, 17)):
        assert msize(*bad) == 0, bad


def test_python_surface_checks_its_arguments():
    x, labels = torch.rand(6, 4), torch.zeros(6, dtype=torch.int64)
    for call in (lambda: ood.knn(x, x, 2), lambda: ood.rows_normalize(x), lambda: ood.moments(x, labels, 2),
                 lambda: ood.head_scores(x, x), lambda: ood.calibrate(x[:, 0]), lambda: ood.tally(x[:, 0], labels, x[0]),
                 lambda: ood.mahalanobis(x, x.double(), torch.eye(4).double()), lambda: ood.auroc(x[:, 0], labels)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for bad in (dict(detectors=()), dict(detectors=("knn", "nearest")), dict(detectors=("knn", "knn")), dict(embedding="logits"), dict(k=0),
                dict(k=65), dict(k=2.0), dict(normalize=1), dict(shrink=-1.0), dict(shrink=NAN), dict(detectors=("abstain",), abstain_class=False)):
        with pytest.raises(ValueError):
            ood.OODDetector(**bad)
    det = ood.OODDetector()
    assert det.detectors == ood.DETECTORS == ("knn", "mahalanobis", "maxsim", "energy", "abstain")
    assert (det.embedding, det.k, det.normalize, det.shrink) == ("sim", 10, True, 1e-6)
    sig = inspect.signature(ood.OODDetector.__init__)
    assert [sig.parameters[k].default for k in ("detectors", "embedding", "k", "normalize", "shrink")] == [ood.DETECTORS, "sim", 10, True, 1e-6]
    with pytest.raises(ValueError, match="fit_finish"):
        det.scores(x, x, x)
    with pytest.raises(RuntimeError, match="GPU only"):
        det.fit_update(x, labels)
    with pytest.raises(ValueError, match="never called"):
        det.fit_finish()
    wide = ood.OODDetector(detectors=("knn", "mahalanobis"))
    with pytest.raises(ValueError, match="use 'knn'"):
        wide._check_emb(_Cuda(3, 257))
    for bad in ((), (0.0,), (1.0,), (0.5, 1.5), [0.5] * 9, 0.9, None):
        with pytest.raises(ValueError, match="tprs"):
            ood.check_tprs(bad)
    assert ood.check_tprs((0.95,)) == [0.95]
    with pytest.raises(ValueError, match="embedding"):
        ood.embedding_of(x, x, "logits")
    assert torch.equal(ood.embedding_of(None, torch.tensor([[0.25, 1.0]])), torch.tensor([[0.75, 0.0]]))
    assert torch.equal(ood.embedding_of(torch.tensor([[[1.0, 3.0], [3.0, 5.0]]]), None, "features"), torch.tensor([[2.0, 4.0]]))
    # a read is host arithmetic on the one vector that was copied
    t = np.array([[4, 2, 2, 1, 1, 1, 2, 2], [4, 1, 2, 0, 1, 2, 3, 1]], dtype=np.float64)
    got = ood.OODEvaluation.unpack(np.concatenate([t.flatten(), [0.5]]), ["knn"], [0.5, 0.9])
    lv = got["knn"]["levels"]
    assert got["knn"]["auroc"] == 0.5 and lv[0]["id_flagged_rate"] == 0.5 and lv[0]["ood_flagged_rate"] == 0.5
    assert lv[0]["accuracy_kept"] == 0.5 and lv[0]["accuracy_flagged"] == 1.0 and lv[1]["accuracy_kept"] == 2 / 3 and lv[1]["tpr"] == 0.9
    assert lv[1]["id_rows"] == 4 and isinstance(lv[1]["id_rows"], int) and lv[1]["ood_flagged_rate"] == 0.0
    assert np.isnan(ood.OODEvaluation.unpack(np.zeros(9), ["knn"], [0.5])["knn"]["levels"][0]["id_flagged_rate"])  # a zero denominator
    from protoasnet_amd.trainer import DPTrainer

    sig = inspect.signature(DPTrainer.fit_ood)
    assert [sig.parameters[k].default for k in ("bank", "calibrate", "level", "tprs", "max_bank")] == ["train", "val", "cine", (0.95,), None]
    sig = inspect.signature(DPTrainer.evaluate_ood)
    assert [sig.parameters[k].default for k in ("mode", "shift", "corruptions", "severities", "level", "max_clips", "seed")] == [
        "test", "corruptions", None, (1, 3, 5), "cine", None, 0]
    t = DPTrainer.__new__(DPTrainer)
    t.ood_fit = None
    with pytest.raises(ValueError, match="fit_ood"):
        t.evaluate_ood("test")
    for bad in (dict(level="study"), dict(tprs=(1.0,)), dict(detectors=("nearest",)), dict(k=0)):
        with pytest.raises(ValueError):
            t.fit_ood(**bad)


class _Cuda:
    """A stand-in with the attributes the host-side shape checks read (no device is needed to refuse a shape)."""

    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)
