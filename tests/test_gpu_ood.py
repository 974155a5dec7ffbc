"""GPU: out-of-distribution detection (csrc/ood.hip through protoasnet_amd.ood) against the numpy restatement of tests/ood_cases.py --
kNN distances and indices, moments, maxsim and normalised rows bitwise, flags and tallies as integers, energy and Mahalanobis to their
derived bounds --, and through OODDetector and DPTrainer.fit_ood / evaluate_ood."""
import os

import numpy as np
import pytest
import torch

import ood_cases as oc
from protoasnet_amd import _lib, ood, selective, synth
from test_cpu_trainer import TRAIN_CFG
from util import CFG_PPNET, CFG_VIDEO_X3D, CFG_XPROTO, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
# (Mq, Mb, E, k): one of everything; k equal to the bank; more neighbours than rows (fill); two query tiles and eight bank chunks of one
# ragged tile; three query tiles, 17 chunks, E at the edge of the resident queries; E past it (queries slab by slab), two chunks, k = 64.
# The last case is not the issue's: 157 bank tiles in 53 chunks of three tiles -- a block that walks several tiles and a ragged last chunk.
KNN_CASES = [(1, 1, 1, 1), (3, 7, 5, 7), (3, 5, 4, 8), (33, 1000, 40, 10), (65, 2049, 256, 32), (2, 130, 1024, 64), (5, 20000, 8, 5)]


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _log(name, err, gate):
    """The largest observed error next to its gate; never changes the verdict."""
    if os.environ.get("PASN_PARITY_LOG"):
        with open(os.environ["PASN_PARITY_LOG"], "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{name}\tmax_err={err:.3g}\tgate={gate:.3g}\n")


def _same_bits(got, want, what):
    """Arrays of one float type bitwise equal, any NaN in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    view = np.uint32 if want.dtype == np.float32 else np.uint64
    bad = np.argwhere((np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)) & ~nan)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def _check_knn(q, bank, k, self_base=-1, what=""):
    got = ood.knn(*_dev(q, bank), k=k, self_base=self_base)
    d, i, st = oc.knn_ref(q, bank, k, self_base)
    _same_bits(got.dist.cpu().numpy(), d, what + " dist")
    gi = got.index.cpu().numpy()
    assert gi.dtype == np.int32 and np.array_equal(gi, i), (what, np.argwhere(gi != i)[:4].tolist())
    assert got.status.dtype == torch.int64 and got.status.tolist() == st.tolist(), (what, got.status.tolist(), st.tolist())
    assert torch.equal(got.score.view(torch.int32), got.dist[:, k - 1].contiguous().view(torch.int32))
    return got


# ---- k nearest bank rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mq,Mb,E,k", KNN_CASES)
def test_knn_matches_the_restatement_bitwise(Mq, Mb, E, k):
    q, bank = oc.emb_case(Mq, E, seed=Mq), oc.emb_case(Mb, E, seed=Mb)
    got = _check_knn(q, bank, k, what=f"({Mq}, {Mb}, {E}, {k})")
    if k > Mb:
        assert got.dist[:, Mb:].eq(INF).all() and got.index[:, Mb:].eq(-1).all()
    if (Mq, Mb, E, k) == (33, 1000, 40, 10):
        # the kernel does not contract: a fused product gives other floats in this case (test_cpu_ood shows it on the CPU)
        fused = oc.knn_ref(q, bank, k, fma=True)[0]
        assert (got.dist.cpu().numpy() != fused).any()
        # the same call again, and on buffers at another offset (4 bytes off any 16-byte boundary): bitwise equal
        again = ood.knn(*_dev(q, bank), k=k)
        assert torch.equal(again.dist.view(torch.int32), got.dist.view(torch.int32)) and torch.equal(again.index, got.index)
        big_q, big_b = torch.zeros(Mq * E + 8, device=DEV), torch.zeros(Mb * E + 8, device=DEV)
        q2, b2 = big_q[1: 1 + Mq * E].view(Mq, E), big_b[3: 3 + Mb * E].view(Mb, E)
        q2.copy_(_dev(q)[0])
        b2.copy_(_dev(bank)[0])
        assert q2.data_ptr() % 16 != 0 and q2.is_contiguous()
        off = ood.knn(q2, b2, k=k)
        assert torch.equal(off.dist.view(torch.int32), got.dist.view(torch.int32)) and torch.equal(off.index, got.index)


def test_knn_ties_leave_one_out_nan_and_inf():
    # four values per coordinate: exact ties are the rule, and the lower bank index wins each
    q, bank = oc.emb_case(40, 6, seed=1, levels=4), oc.emb_case(700, 6, seed=2, levels=4)
    want = oc.knn_ref(q, bank, 16)
    assert (want[0][:, 1:] == want[0][:, :-1]).mean() > 0.3  # (ties are common in the answer itself)
    _check_knn(q, bank, 16, what="quantised")
    # the bank as its own queries, every row left out of its own list; and a slice of it
    bank = oc.emb_case(300, 12, seed=3)
    got = _check_knn(bank, bank, 5, self_base=0, what="self_base 0")
    assert (got.index != torch.arange(300, device=DEV)[:, None]).all() and (got.dist[:, 0] > 0).all()
    assert (ood.knn(*_dev(bank, bank), k=1).index[:, 0] == torch.arange(300, device=DEV)).all()  # without it a row finds itself
    _check_knn(bank[17:67], bank, 5, self_base=17, what="self_base 17")
    _check_knn(bank[:3], bank[:3], 4, self_base=0, what="two eligible rows, k = 4")
    # a NaN query row, two NaN bank rows (one of them in another tile), a row holding +-inf on either side
    q, bank = oc.emb_case(9, 7, seed=4), oc.emb_case(400, 7, seed=5)
    q[2, 3] = NAN
    bank[5, 0] = NAN
    bank[390, 6] = NAN
    q[4, 1] = INF
    bank[7, 1] = INF
    bank[8, 2] = -INF
    got = _check_knn(q, bank, 6, what="NaN and inf")
    assert got.status.tolist() == [2, 1] and torch.isnan(got.dist[2]).all() and got.index[2].eq(-1).all()
    assert not torch.isin(got.index, torch.tensor([5, 390], device=DEV, dtype=torch.int32)).any()
    assert got.dist[4].eq(INF).all() and got.index[4].tolist() == [0, 1, 2, 3, 4, 6]  # every finite row at +inf; inf - inf is not eligible


# ---- scores that need no fit, normalised rows --------------------------------------------------------------------------------------------
def test_maxsim_and_rows_normalize_bitwise_energy_within_two_ulp():
    rng = np.random.default_rng(8)
    M, P, K, K_real = 517, 30, 4, 3  # crosses two 256-thread blocks
    sim = rng.uniform(-1, 1, (M, P)).astype(np.float32)
    sim[3, 7] = NAN
    sim[4] = 1.0
    logits = rng.uniform(-12, 12, (M, K)).astype(np.float32)
    logits[5, 1] = NAN
    logits[6, :3] = [80.0, -80.0, 0.0]
    logits[7, 3] = NAN  # the abstention logit is not read
    maxsim, energy = ood.head_scores(*_dev(sim, logits), K_real)
    _same_bits(maxsim.cpu().numpy(), oc.maxsim_ref(sim), "maxsim")
    assert float(maxsim[4]) == 0.0 and bool(torch.isnan(maxsim[3]))
    want = oc.energy_ref(logits, K_real)
    got = energy.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[5]) and not np.isnan(got[7])
    ok = ~np.isnan(want)
    ulps = np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64))  # (no value straddles zero by luck:
    ulps = np.where(np.sign(got[ok]) == np.sign(want[ok]), ulps, 1 << 30)                                 # a sign flip is a failure)
    _log("energy ulp", float(ulps.max()), 2)
    print(f"energy: {int((ulps > 0).sum())} of {ulps.size} values differ from the float64 restatement, at most {int(ulps.max())} ulp")
    assert ulps.max() <= 2
    # either output alone
    assert torch.equal(ood.head_scores(_dev(sim)[0], None)[0].view(torch.int32), maxsim.view(torch.int32))
    assert ood.head_scores(None, _dev(logits)[0], K_real)[0] is None
    for E in (1, 5, 40, 256, 1000):
        x = oc.emb_case(259, E, seed=E)
        x[1] = 0.0
        x[2] *= np.float32(1e-20)  # squares underflow to denormals or zero: a zero n2 copies the row
        y = ood.rows_normalize(_dev(x)[0]).cpu().numpy()
        want = oc.normalize_ref(x)
        differ = int((y.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"rows_normalize E={E}: {differ} of {y.size} values differ")
        _same_bits(y, want, f"rows_normalize E={E}")


# ---- class-conditional Gaussians -----------------------------------------------------------------------------------------------------------
def _moments_case(M, E, K, seed):
    rng = np.random.default_rng(seed + 1)
    # magnitudes over 2^-12 .. 2^12: products 48 bits wide at exponents 48 apart do not add exactly in fp64, so the ORDER of the sums shows
    x = (oc.emb_case(M, E, seed) * np.exp2(rng.integers(-12, 13, (M, E))).astype(np.float32)).astype(np.float32)
    labels = rng.integers(0, K, M).astype(np.int32)
    if M >= 7:
        labels[1], labels[4] = -1, K  # padding rows
        x[2, E - 1] = NAN             # a labelled NaN row
        x[4, 0] = NAN                 # a NaN row that is padding anyway
    return x, labels


def _check_moments(got, want, what):
    for k in ("sum", "scatter"):
        _same_bits(getattr(got, k).cpu().numpy(), want[k], f"{what} {k}")
    assert got.n.dtype == torch.int64 and got.n.tolist() == want["n"].tolist() and got.skipped.tolist() == want["skipped"].tolist(), what


def test_moments_match_the_restatement_bitwise():
    chunk = ood.moment_chunk()
    for M, E, K in ((1, 1, 2), (7, 3, 2), (chunk + 1, 40, 4), (3 * chunk + 5, 256, 4)):
        x, labels = _moments_case(M, E, K, seed=M + E)
        want = oc.moments_ref(x, labels, K, chunk)
        got = ood.moments(*_dev(x, labels), K)
        _check_moments(got, want, f"({M}, {E}, {K})")
        if M >= 7:
            assert want["skipped"].tolist() == [2, 1]
        _check_moments(ood.moments(*_dev(x, labels), K), want, "repeat")
    # two accumulated calls against the restatement of that sequence (not of the concatenation: the second call's sum is added as one)
    xa, la = _moments_case(chunk + 9, 17, 3, seed=5)
    xb, lb = _moments_case(40, 17, 3, seed=6)
    first = ood.moments(*_dev(xa, la), 3)
    both = ood.moments(*_dev(xb, lb), 3, into=first)
    assert both is first
    _check_moments(both, oc.moments_ref(xb, lb, 3, chunk, prev=oc.moments_ref(xa, la, 3, chunk)), "accumulated")
    # the defined order is visible: another chunk length gives other bits somewhere in this case
    other = oc.moments_ref(xa, la, 3, chunk=64)
    assert (other["scatter"] != oc.moments_ref(xa, la, 3, chunk)["scatter"]).any()


def test_mahalanobis_within_its_summation_bound():
    for M, E, K, seed in ((1, 1, 2, 1), (37, 5, 3, 2), (130, 40, 4, 3), (21, 256, 4, 4)):
        xb, lb = oc.mixture_case(max(3 * E, 40), E, K, seed)
        if K > 2:
            lb[lb == 1] = 0  # class 1 has no rows: a NaN mean that never wins
        mo = oc.moments_ref(xb, lb, K)
        mu, W = oc.gaussian_fit_ref(mo["n"], mo["sum"], mo["scatter"])
        x, _ = oc.mixture_case(M, E, K, seed + 10, shift=0.5)
        if M > 4:
            x[3, 0] = NAN
        m, score, arg = ood.mahalanobis(*_dev(x, mu, W))
        wm, bound, wscore, warg = oc.mahalanobis_ref(x, mu, W)
        gm = m.cpu().numpy()
        assert gm.dtype == np.float64 and np.array_equal(np.isnan(gm), np.isnan(wm))
        ok = ~np.isnan(wm)
        ratio = float((np.abs(gm[ok] - wm[ok]) / bound[ok]).max())
        _log(f"mahalanobis ({M}, {E}, {K}) error / bound", ratio, 1.0)
        print(f"mahalanobis ({M}, {E}, {K}): largest error / bound {ratio:.3g}")
        assert ratio <= 1.0
        # the score is the rounded minimum; the class is the restatement's wherever the two smallest differ by more than the bound
        gs, ga = score.cpu().numpy(), arg.cpu().numpy()
        assert np.array_equal(np.isnan(gs), np.isnan(wscore)) and np.array_equal(ga < 0, warg < 0)
        rows = np.flatnonzero(warg >= 0)
        assert (np.abs(gs[rows].view(np.int32).astype(np.int64) - wscore[rows].view(np.int32).astype(np.int64)) <= 1).all()
        assert np.array_equal(gs[rows], gm[rows, ga[rows]].astype(np.float32))
        two = np.sort(np.where(np.isnan(wm[rows]), np.inf, wm[rows]), axis=1)[:, :2]
        clear = rows[(two[:, 1] - two[:, 0]) > 2 * np.nanmax(bound[rows], axis=1)]
        assert len(clear) > 0 and np.array_equal(ga[clear], warg[clear])
        if K > 2:
            assert (ga[rows] != 1).all()
        if M > 4:
            assert np.isnan(gs[3]) and ga[3] == -1


# ---- thresholds, flags, tallies ------------------------------------------------------------------------------------------------------------
def test_thresholds_flags_tallies_and_auroc_are_exact():
    rng = np.random.default_rng(12)
    M = 3000
    scores = rng.normal(0, 1, M).astype(np.float32)
    scores[::97] = NAN
    scores[5], scores[6] = INF, scores[7]  # an infinite score and an exact tie
    tprs = (0.5, 0.9, 0.95, 0.9999)  # the last needs more rows than there are: +inf
    th = ood.calibrate({"a": _dev(scores)[0], "b": _dev(-scores[:10])[0]}, tprs)
    for name, s in (("a", scores), ("b", -scores[:10])):
        want = [oc.threshold_ref(s, t) for t in tprs]
        assert th.tau[name].dtype == torch.float32 and th.tau[name].tolist() == [float(w[0]) for w in want], name
        assert int(th.n[name]) == want[0][1] and int(th.nan[name]) == want[0][3]
    assert th.tau["a"][3] == INF and th.read()["detectors"]["b"] == {"tau": th.tau["b"].tolist(), "n": 9, "nan_rows": 1}
    kind = rng.integers(0, 3, M).astype(np.int32)  # 2: padding rows
    kind[:4] = [-1, 7, 0, 1]
    correct = rng.integers(0, 2, M).astype(np.int32)
    tau = th.tau["a"]
    for c in (correct, None):
        flags, tallies = ood.tally(*_dev(scores, kind), tau, None if c is None else _dev(c)[0])
        wf, wt = oc.tally_ref(scores, kind, tau.cpu().numpy(), c)
        assert flags.dtype == torch.uint8 and np.array_equal(flags.cpu().numpy(), wf)
        assert tallies.dtype == torch.int64 and np.array_equal(tallies.cpu().numpy(), wt), (tallies.tolist(), wt.tolist())
    assert wt[3, 1] + wt[3, 3] == wt[3, 4] > 0  # at +inf only the NaN rows are flagged
    got = float(ood.auroc(*_dev(scores, kind)))
    assert got == oc.auroc_ref(scores, kind)
    ev = ood.evaluate({"a": _dev(scores)[0]}, _dev(kind)[0], th, _dev(correct)[0])
    rd = ev.read()["a"]
    wt = oc.tally_ref(scores, kind, tau.cpu().numpy(), correct)[1]
    assert rd["auroc"] == got and [[lv[k] for k in oc.TALLY_NAMES] for lv in rd["levels"]] == wt.tolist()
    assert rd["levels"][1]["id_flagged_rate"] == wt[1, 1] / wt[1, 0] and rd["levels"][1]["accuracy_kept"] == wt[1, 5] / wt[1, 6]
    with pytest.raises(ValueError, match="no threshold"):
        ood.evaluate({"c": _dev(scores)[0]}, _dev(kind)[0], th)


# ---- the detector on a model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,shape", [(CFG_VIDEO_X3D, (6, 3, 4, 64, 64)), (CFG_XPROTO, (6, 3, 224, 224))], ids=["x3d_s", "xprotonet_image"])
def test_detector_fed_from_push_forward_equals_the_restatement(cfg, shape):
    m = synth_model(cfg).to(DEV).eval()
    K_real = cfg["num_classes"] - 1
    det = ood.OODDetector(detectors=("knn", "maxsim", "energy", "abstain"), k=3)
    outs = []
    with torch.no_grad():
        for b in range(2):  # 12 clips in two batches
            feats, dist, _, logits = m.push_forward(synth.echo_clips(shape, seed=40 + b).to(DEV))
            emb = det.embed(feats, dist)
            det.fit_update(emb)
            outs.append((emb, (1 - dist).float(), logits.float()))
    fit = det.fit_finish()
    emb, sim, logits = (torch.cat(t) for t in zip(*outs))
    assert torch.equal(emb, sim) and fit.bank.shape == (12, emb.shape[1]) and fit.mu is None
    scores = det.scores(emb, sim, logits, self_base=0)
    h_emb, h_sim, h_logits = (t.cpu().numpy() for t in (emb, sim, logits))
    nb = oc.normalize_ref(h_emb)
    _same_bits(fit.bank.cpu().numpy(), nb, "bank")
    wd, wi, _ = oc.knn_ref(nb, nb, 3, self_base=0)
    got = ood.knn(fit.bank, fit.bank, 3, self_base=0)
    assert np.array_equal(got.index.cpu().numpy(), wi)
    _same_bits(scores["knn"].cpu().numpy(), wd[:, -1], "knn score")
    _same_bits(scores["maxsim"].cpu().numpy(), oc.maxsim_ref(h_sim), "maxsim")
    assert torch.equal(scores["abstain"], selective.uncertainty(logits, True))
    we = oc.energy_ref(h_logits, K_real)
    assert (np.abs(scores["energy"].cpu().numpy().view(np.int32).astype(np.int64) - we.view(np.int32).astype(np.int64)) <= 2).all()
    # thresholds, flags and tallies: the restatement fed the downloaded scores, with the second batch playing the shifted rows
    host = {d: s.cpu().numpy() for d, s in scores.items()}
    th = det.calibrate({d: s[:6] for d, s in scores.items()}, (0.5, 0.8))
    kind = np.array([0] * 6 + [1] * 6, np.int32)
    correct = (selective.first_largest(logits[:, :K_real]) == 0).to(torch.int32)
    on_device = det.evaluate(scores, _dev(kind)[0], correct)
    ev = on_device.read()
    for d in det.detectors:
        tau = [oc.threshold_ref(host[d][:6], t)[0] for t in (0.5, 0.8)]
        assert th.tau[d].tolist() == [float(t) for t in tau], d
        wf, wt = oc.tally_ref(host[d], kind, np.array(tau, np.float32), correct.cpu().numpy())
        assert np.array_equal(on_device.flags[d].cpu().numpy(), wf), d
        assert [[lv[k] for k in oc.TALLY_NAMES] for lv in ev[d]["levels"]] == wt.tolist(), d
        want_auc = oc.auroc_ref(host[d], kind)
        assert ev[d]["auroc"] == want_auc, d
    # Mahalanobis on a hand-made embedding (12 rows can not fit the model's 30 or 40 similarities: that is refused)
    full = ood.OODDetector(detectors=("mahalanobis",), num_classes=2)
    full.fit_update(emb, _dev(np.arange(12) % 2)[0])
    with pytest.raises(ValueError, match="needs at least"):
        full.fit_finish()
    small = ood.OODDetector(detectors=("mahalanobis",), num_classes=2, shrink=1e-3)
    small.fit_update(emb[:, :3], _dev(np.arange(12) % 2)[0])
    f = small.fit_finish()
    mo = oc.moments_ref(h_emb[:, :3], np.arange(12) % 2, 2)
    mu, W = oc.gaussian_fit_ref(mo["n"], mo["sum"], mo["scatter"], 1e-3)
    assert np.array_equal(f.mu.cpu().numpy(), mu) and np.array_equal(f.W.cpu().numpy(), W) and f.n.tolist() == [6, 6]
    wm, bound, _, _ = oc.mahalanobis_ref(h_emb[:, :3], mu, W)
    gm = ood.mahalanobis(emb[:, :3].contiguous(), f.mu, f.W)[0].cpu().numpy()
    assert (np.abs(gm - wm) <= bound).all()
    assert small.scores(emb[:, :3].contiguous())["mahalanobis"].shape == (12,)


class _Counting:
    """The library with every call's symbol recorded."""

    def __init__(self, handle, calls):
        self._handle, self._calls = handle, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._handle, name)


@pytest.mark.timeout(900)
def test_trainer_fit_ood_and_evaluate_ood(monkeypatch):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(CFG_VIDEO_X3D).to(DEV)
    K_real = 2

    def loader(seed, tag):  # three batches of two clips; cines of two clips that straddle batches
        return [{"cine": synth.echo_clips((2, 3, 4, 64, 64), seed=seed + b), "target_AS": torch.tensor([b % 2, ((b + 1) % 3) % 2]),
                 "filename": [f"{tag}{b}", f"{tag}{(b + 1) % 3}"]} for b in range(3)]

    loaders = {"train": loader(60, "t"), "val": loader(70, "v"), "test": loader(80, "s"), "other": loader(90, "o")}
    logs = []
    t = DPTrainer(m, {"abstain_class": True, "train": TRAIN_CFG}, loaders, log=lambda s, *_: logs.append(str(s)))
    # what the existing evaluation entries call in the library, before anything of this module ran
    calls = []
    real = _lib.lib()

    def record():
        del calls[:]
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "lib", lambda: _Counting(real, calls))
            t.evaluate_selective("test", level="cine")
            t.evaluate_robustness("val", corruptions=("noise",), severities=(1,))
        return list(calls)

    record()  # (the first pass also compiles plans and probes routes: those calls are not the entries' own)
    before = record()
    assert before and not any(c.startswith("pasn_ood") for c in before)
    with pytest.raises(ValueError, match="fit_ood"):
        t.evaluate_ood("test")
    m.train()
    state = (t.current_epoch, t.current_iteration)
    dets = ("knn", "maxsim", "energy", "abstain")
    with pytest.raises(ValueError, match="needs at least"):  # six clips can not fit 30 similarities
        t.fit_ood("train", "val", detectors=("mahalanobis",))
    res = t.fit_ood("train", "val", tprs=(0.5, 0.75), detectors=dets, k=2)
    assert m.training and (t.current_epoch, t.current_iteration) == state
    assert res["level"] == "cine" and res["bank_rows"] == 6 and res["rows"] == 3 and res["tprs"] == [0.5, 0.75] and list(res["detectors"]) == list(dets)
    assert all(r["n"] == 3 and len(r["tau"]) == 2 for r in res["detectors"].values()) and any("ood knn (cine)" in s and "tau" in s for s in logs)
    # the same by hand: the detector over the train loader, the val scores averaged per cine in fp64
    det = ood.OODDetector(detectors=dets, k=2)
    m.eval()

    def sweep(name):
        outs, keys = [], []
        with torch.no_grad():
            for b in loaders[name]:
                feats, dist, _, logits = m.push_forward(t.prepare_input(b["cine"]))
                outs.append((det.embed(feats, dist), (1 - dist).float(), logits.float()))
                keys += b["filename"]
        return [torch.cat(x) for x in zip(*outs)], keys

    (emb, sim, logits), _ = sweep("train")
    det.fit_update(emb)
    det.fit_finish()
    (emb, sim, logits), keys = sweep("val")
    offsets, rows, _ = selective.build_groups(keys)
    val_scores = {d: oc.cine_mean_ref(s.cpu().numpy(), offsets, rows) for d, s in det.scores(emb, sim, logits).items()}
    for d in dets:
        assert res["detectors"][d]["tau"] == [float(oc.threshold_ref(val_scores[d], tp)[0]) for tp in (0.5, 0.75)], d
    m.train()
    # two corruptions x two severities
    ev = t.evaluate_ood("test", corruptions=("noise", "blur"), severities=(1, 5), seed=3)
    assert m.training and ev["level"] == "cine" and ev["rows"] == 3 and ev["tprs"] == [0.5, 0.75] and list(ev["detectors"]) == list(dets)
    for d in dets:
        e = ev["detectors"][d]
        assert e["tau"] == res["detectors"][d]["tau"] and list(e["cells"]) == ["noise", "blur"] and list(e["cells"]["blur"]) == [1, 5]
        assert all(len(e[k]) == 2 for k in ("id_flagged_rate", "accuracy_kept", "accuracy_flagged"))
        for by_sev in e["cells"].values():
            for c in by_sev.values():
                assert c["rows"] == 3 and len(c["flagged_rate"]) == 2 and (np.isnan(c["auroc"]) or 0.0 <= c["auroc"] <= 1.0)
    # ... the integers against the restatement, for the clean rows and one cell
    from protoasnet_amd import robustness

    m.eval()
    (emb, sim, logits), keys = sweep("test")
    offsets, rows, _ = selective.build_groups(keys)
    clean = {d: oc.cine_mean_ref(s.cpu().numpy(), offsets, rows) for d, s in det.scores(emb, sim, logits).items()}
    outs = []
    with torch.no_grad():
        for b, batch in enumerate(loaders["test"]):
            feats, dist, _, lg = m.push_forward(robustness.corrupt(t.prepare_input(batch["cine"]), "blur", 5, 3 + b))
            outs.append((det.embed(feats, dist), (1 - dist).float(), lg.float()))
    shifted = {d: oc.cine_mean_ref(s.cpu().numpy(), offsets, rows) for d, s in det.scores(*[torch.cat(x) for x in zip(*outs)]).items()}
    kind = np.array([0] * 3 + [1] * 3)
    for d in dets:
        both = np.concatenate([clean[d], shifted[d]])
        _, wt = oc.tally_ref(both, kind, np.array(res["detectors"][d]["tau"], np.float32))
        e = ev["detectors"][d]
        assert e["id_flagged_rate"] == [x / 3 for x in wt[:, 1].tolist()], d
        assert e["cells"]["blur"][5]["flagged_rate"] == [x / 3 for x in wt[:, 3].tolist()], d
        want_auc = oc.auroc_ref(both, kind)
        assert e["cells"]["blur"][5]["auroc"] == want_auc or (np.isnan(want_auc) and np.isnan(e["cells"]["blur"][5]["auroc"])), d
    m.train()
    # a named shift loader; clip level; bank == calibrate: the leave-one-out scan
    named = t.evaluate_ood("test", shift="other")
    assert list(named["detectors"]["knn"]["cells"]) == ["other"] and list(named["detectors"]["knn"]["cells"]["other"]) == [0]
    assert named["detectors"]["knn"]["id_flagged_rate"] == ev["detectors"]["knn"]["id_flagged_rate"]
    with pytest.raises(ValueError, match="shift"):
        t.evaluate_ood("test", shift="nowhere")
    with pytest.raises(ValueError, match="calibrated at level 'cine'"):
        t.evaluate_ood("test", level="clip")
    loo = t.fit_ood("train", "train", level="clip", tprs=(0.5,), detectors=("knn",), k=2, normalize=False)
    assert loo["rows"] == 6 and loo["bank_rows"] == 6 and loo["level"] == "clip"
    m.eval()
    (emb, _, _), _ = sweep("train")
    h = emb.cpu().numpy()
    want = oc.knn_ref(h, h, 2, self_base=0)[0][:, -1]
    assert (want > 0).all() and loo["detectors"]["knn"]["tau"] == [float(oc.threshold_ref(want, 0.5)[0])]
    clip = t.evaluate_ood("test", corruptions=("noise",), severities=(3,), level="clip", max_clips=5)
    assert clip["rows"] == 5 and clip["detectors"]["knn"]["cells"]["noise"][3]["rows"] == 5
    # the existing entries call exactly what they called before
    assert record() == before
    # PPNet and the CPU are refused
    tp = DPTrainer(synth_model(CFG_PPNET).to(DEV), {"abstain_class": False, "train": TRAIN_CFG}, {"train": [], "val": []}, log=lambda *_: None)
    with pytest.raises(NotImplementedError, match="out-of-distribution detection covers XProtoNet and Video_XProtoNet"):
        tp.fit_ood("train", "val")
    with pytest.raises(RuntimeError, match="GPU only"):
        ood.knn(torch.rand(3, 2), torch.rand(4, 2), 1)
