"""GPU: the grouped bootstrap (csrc/bootstrap.hip through protoasnet_amd.bootstrap) against the float64 / int64 numpy restatement of
tests/bootstrap_cases.py, against the project's existing kernels on host-expanded rows, and through SelectiveEvaluator.finish and
DPTrainer.evaluate_selective."""
import os

import numpy as np
import pytest
import torch

import bootstrap_cases as bc
from protoasnet_amd import bootstrap, metrics, selective
from protoasnet_amd.trainer import confusion_to_metrics
from test_cpu_trainer import TRAIN_CFG
from test_gpu_selective import _cine_loader, _Head, _same
from util import CFG_VIDEO_X3D, synth_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
# The statistics are ratios of exact integers (and, for the risk-coverage area, a mean of at most 2^31 such ratios in [0, 1]) in fp64 on
# both sides: a handful of roundings of 1.1e-16 each, and a mean's error grows at worst with log2 of its length.  1e-12 absolute is
# what the issue sets.
GATE = 1e-12
BOUND = bootstrap.lds_max_groups  # read through the library when a test runs (collection must not need the library)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _log(name, err, gate):
    """The largest observed error next to its gate (profiles/bootstrap_parity_observed.tsv); never changes the verdict."""
    if os.environ.get("PASN_PARITY_LOG"):
        with open(os.environ["PASN_PARITY_LOG"], "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{name}\tmax_err={err:.3g}\tgate={gate:.3g}\n")


def _host(rep):
    return {k: getattr(rep, k).cpu().numpy() for k in ("stats", "cm", "u2", "n_pos", "n_neg")}


def _check(probs, labels, u, groups, B, seed, name):
    """Integers exact, statistics within the gate, NaN in the same places; returns (device results on the host, restatement)."""
    want = bc.stats_ref(probs, labels, u, groups, B, seed)
    rep = bootstrap.replicates(*_dev(probs, labels, u), groups=groups, B=B, seed=seed)
    got = _host(rep)
    assert rep.stats.dtype == torch.float64 and rep.cm.dtype == torch.int64 and got["stats"].shape == (B + 1, 6)
    assert torch.equal(rep.point, rep.stats[B])
    for k in ("cm", "u2", "n_pos", "n_neg"):
        assert np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4])
    assert np.array_equal(np.isnan(got["stats"]), np.isnan(want["stats"])), (name, np.argwhere(np.isnan(got["stats"]) != np.isnan(want["stats"]))[:4])
    err = float(np.nanmax(np.abs(got["stats"] - want["stats"])))
    print(f"{name}: max |stats - restatement| = {err:.3g}")
    _log(name, err, GATE)
    assert err <= GATE, (name, err)
    return got, want


# ---- counts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,B", [(1, 3), (5, 7), (64, 4), (257, 33), (4099, 16)])
def test_counts_equal_the_restatement(G, B):
    seed = (G << 32) | 12345  # both key words
    got = bootstrap.draw_counts(G, B, seed=seed)
    assert got.dtype == torch.int32 and got.shape == (B, G)
    assert np.array_equal(got.cpu().numpy(), bc.counts_ref(G, B, seed))
    b0 = 2 if B > 4 else 1
    assert torch.equal(bootstrap.draw_counts(G, B - b0, seed=seed, b0=b0), got[b0:])  # replicates b0 .. are the matching slice
    assert torch.equal(bootstrap.draw_counts(G, B, seed=seed), got)


def test_counts_on_both_sides_of_the_lds_bound():
    """At and below the bound a block histograms its replicate in LDS (uint16 pairs: G and G - 1 cover an odd and an even number of
    halves); above, the threads add into the zeroed output.  65 535 / 65 536: where a uint16 count would stop, far inside the global path."""
    bound = BOUND()
    for G in (bound - 1, bound, bound + 1, 65535, 65536):
        got = bootstrap.draw_counts(G, 3, seed=G)
        assert np.array_equal(got.cpu().numpy(), bc.counts_ref(G, 3, G)), G
        assert torch.equal(bootstrap.draw_counts(G, 2, seed=G, b0=1), got[1:]), G


# ---- metrics, identity groups --------------------------------------------------------------------------------------------------------------
NO_CLASS_LOST = [(37, 3, 257, 0), (300, 4, 64, 1), (400, 16, 64, 2)]  # (M, K, B, seed): every replicate keeps every class


@pytest.mark.parametrize("M,K,B,seed", NO_CLASS_LOST)
def test_metrics_where_no_replicate_loses_a_class(M, K, B, seed):
    probs, labels, u = bc.metric_case(M, K, seed=10 * K + seed)
    got, want = _check(probs, labels, u, None, B, seed, f"identity M={M} K={K} B={B}")
    assert np.isfinite(want["stats"][:B, 3]).all()  # n_finite == B in the restatement: no missing-class path hides in this case
    assert bootstrap.intervals_of(got["stats"])["auc"]["n_finite"] == B
    for col in range(K):  # quantised to eighths: ties in every class column
        assert len(np.unique(probs[:, col])) <= 9


@pytest.mark.parametrize("M,K,B,seed,kind", [
    (1000, 2, 5, 0, "ties"), (1000, 3, 5, 1, "nan"), (5000, 4, 1, 2, "ties"), (5000, 2, 5, 0, "pad"), (300, 3, 5, 1, "pad"),
    (37, 2, 64, 2, "nan"), (1000, 4, 1, 1, "ties")])
def test_metrics_match_the_restatement(M, K, B, seed, kind):
    """1000 and 5000 rows: more than one sweep chunk of 2048 positions only at 5000; NaN u rows; padding rows (label -1)."""
    probs, labels, u = bc.metric_case(M, K, seed=7 * M + K, kind=kind)
    got, want = _check(probs, labels, u, None, B, seed, f"identity M={M} K={K} B={B} {kind}")
    if kind == "nan":  # a replicate that drew a NaN row has no error AUROC; its risk-coverage area stands
        drew = bc.counts_ref(M, B, seed)[:, [1, M - 2]].sum(1) > 0
        assert drew.any() and np.isnan(got["stats"][:B, 5][drew]).all() and np.isfinite(got["stats"][:, 4]).all() and np.isnan(got["stats"][B, 5])
    if kind == "pad":
        assert (got["cm"].sum((1, 2)) < M).all() and got["cm"][B].sum() == (labels >= 0).sum()


def test_metrics_above_the_lds_bound():
    """One row more than the bound, every row its own group: the blocks keep their counts in slices of the workspace and loop over the
    replicates (three slices would fit; B + 1 = 3 blocks)."""
    M = BOUND() + 1
    probs, labels, u = bc.metric_case(M, 2, seed=3)
    got, want = _check(probs, labels, u, None, 2, 4, f"identity M={M} K=2 B=2 (global counts)")
    assert np.array_equal(got["cm"][:2].sum((1, 2)), [M, M])
    # ... and the same rows in groups of two stay on the LDS side and draw other counts
    groups = selective.build_groups([i // 2 for i in range(M)])
    assert len(groups[2]) <= BOUND()
    rep = bootstrap.replicates(*_dev(probs, labels, u), groups=groups, B=2, seed=4)
    assert np.array_equal(rep.cm[2].cpu().numpy(), got["cm"][2]) and abs(float(rep.stats[2, 4]) - got["stats"][2, 4]) <= GATE


def test_blocks_that_reuse_their_count_slice():
    """Above the LDS bound with more replicates than blocks: a block redraws into the slice it has just read.  The restatement would take
    minutes here; replicates of the first and of the second pass and the point row are rebuilt from the device's own counts with the
    existing kernels instead."""
    from protoasnet_amd import _lib

    M, K, B = BOUND() + 1, 2, 601
    size = _lib.lib().pasn_bootstrap_workspace_bytes
    blocks = (size(M, M, K, B) - size(M, BOUND(), K, B)) // (4 * M)  # the slices of the workspace
    assert 1 <= blocks < B, blocks
    probs, labels, u = bc.metric_case(M, K, seed=21, kind="pad")
    d_probs, d_labels, d_u = _dev(probs, labels, u)
    got = _host(bootstrap.replicates(d_probs, d_labels, d_u, B=B, seed=8))
    for b in (0, blocks - 1, blocks, B - 1, B):
        counts = np.ones(M, np.int32) if b == B else bootstrap.draw_counts(M, 1, seed=8, b0=b)[0].cpu().numpy()
        sel = torch.from_numpy(bc.replicate_rows(counts, labels, K)).to(DEV)
        cm, stats = _existing(d_probs[sel], d_labels[sel], d_u[sel], K)
        assert np.array_equal(got["cm"][b], cm), b
        err = float(np.abs(got["stats"][b] - np.array(stats)).max())
        _log(f"slice reuse, replicate {b} of {B} on {blocks} blocks", err, GATE)
        assert err <= GATE, (b, got["stats"][b], stats)
    assert len({got["cm"][b].tobytes() for b in range(B)}) == B  # no replicate is another's copy


def test_the_undefined_case_on_purpose():
    """M = 12, K = 4: three rows per class, so a replicate often loses one.  Its AUC is NaN -- not pasn_roc_auc_ovr's 0.0 -- in exactly
    the replicates where the restatement's is, and the interval uses the finite ones."""
    probs, labels, u = bc.metric_case(12, 4, seed=5)
    for seed in (0, 1, 2):
        got, want = _check(probs, labels, u, None, 257, seed, f"undefined M=12 K=4 seed={seed}")
        lost = np.isnan(want["stats"][:257, 3])
        assert 25 <= lost.sum() <= 32 and np.array_equal(lost, ((got["n_pos"][:257] == 0) | (got["n_neg"][:257] == 0)).any(1))
        rep = bootstrap.replicates(*_dev(probs, labels, u), B=257, seed=seed)
        ci, ref = bootstrap.intervals(rep, 0.9), bc.intervals_ref(want["stats"], 0.9)
        assert ci["auc"]["n_finite"] == 257 - lost.sum() == ref["auc"]["n_finite"] and ci["acc"]["n_finite"] == 257
        for name in bootstrap.STAT_NAMES:
            for k in ("point", "lo", "hi", "se"):
                assert abs(ci[name][k] - ref[name][k]) <= GATE, (name, k)
        assert ci["auc"]["lo"] <= ci["auc"]["point"] <= 1.0 and ci["auc"]["lo"] < ci["auc"]["hi"]


# ---- groups ------------------------------------------------------------------------------------------------------------------------------
def test_random_non_contiguous_groups():
    probs, labels, u = bc.metric_case(300, 3, seed=8)
    groups = selective.build_groups(bc.random_groups(300, seed=4))
    assert np.diff(groups[0]).max() > 1 and (np.diff(groups[1]) != 1).any()
    got, _ = _check(probs, labels, u, groups, 16, 3, "random groups of 1..9 rows")
    assert len(set(got["cm"][:16].sum((1, 2)).tolist())) > 1  # groups of different sizes: the replicates differ in their number of rows


def test_one_group_holding_every_row():
    probs, labels, u = bc.metric_case(37, 3, seed=9)
    got, _ = _check(probs, labels, u, selective.build_groups(["all"] * 37), 3, 0, "G = 1")
    for k in got:  # the one unit is drawn once: every replicate is the sample
        assert all(np.array_equal(got[k][b], got[k][3], equal_nan=True) for b in range(3)), k


def test_a_giant_group_among_singletons():
    """A group of 400 rows among 100 singletons: drawn c times it puts 400 c rows into the replicate, and a row's weight times the
    weight before it goes into the hundreds of thousands (the int64 pair sums, the per-copy loop of the risk terms)."""
    probs, labels, u = bc.metric_case(500, 3, seed=10)
    keys = ["giant" if i % 5 else i for i in range(500)]
    groups = selective.build_groups(keys)
    assert np.diff(groups[0]).max() == 400 and len(groups[2]) == 101
    got, _ = _check(probs, labels, u, groups, 16, 1, "one giant group")
    drawn = bc.counts_ref(101, 16, 1)[:, groups[2].index("giant")]
    assert drawn.max() >= 2 and got["cm"][:16].sum((1, 2)).max() >= 800 and got["u2"].max() > 100_000


def test_groups_containing_padding_rows_and_unlisted_rows():
    probs, labels, u = bc.metric_case(300, 4, seed=11, kind="pad")
    groups = selective.build_groups(bc.random_groups(300, seed=6))
    _check(probs, labels, u, groups, 16, 2, "groups with padding rows")
    offsets, rows = groups[0][:21].copy(), groups[1][: groups[0][20]].copy()  # the first 20 groups only: the other rows never enter
    got, _ = _check(probs, labels, u, (offsets, rows), 5, 2, "unlisted rows")
    assert got["cm"][5].sum() == (labels[rows] >= 0).sum()
    with pytest.raises(ValueError, match="lie in"):
        bootstrap.replicates(*_dev(probs[:100], labels[:100], u[:100]), groups=groups, B=4)  # rows past the tensors
    with pytest.raises(ValueError, match="one group only"):
        bootstrap.replicates(*_dev(probs, labels, u), groups=(np.array([0, 2, 4]), np.array([0, 1, 1, 2])), B=4)


# ---- tie to the existing kernels -----------------------------------------------------------------------------------------------------------
def _existing(probs, labels, u, K):
    """(cm, acc, bal_acc, f1_mean, auc, aurc, error_auroc) of device rows from the kernels the project already has."""
    pred = selective.first_largest(probs)
    cm = torch.bincount(labels.long() * K + pred, minlength=K * K).view(K, K)
    m = confusion_to_metrics(cm)
    rc = selective.risk_coverage(probs, labels, u)
    auc, per = metrics.roc_auc_ovr_weighted(probs, labels, K, per_class=True)
    auc = float(auc) if bool(torch.isfinite(per).all()) else float("nan")  # the one deliberate difference
    return cm.cpu().numpy(), [float(cm.diag().sum()) / float(cm.sum()), m["accuracy"], m["f1_mean"], auc, float(rc.aurc), float(rc.error_auroc)]


def test_replicates_are_the_existing_kernels_on_expanded_rows():
    K = 3
    probs, labels, u = bc.metric_case(300, K, seed=12)
    groups = selective.build_groups(bc.random_groups(300, seed=13))
    d_probs, d_labels, d_u = _dev(probs, labels, u)
    rep = bootstrap.replicates(d_probs, d_labels, d_u, groups=groups, B=3, seed=6)
    counts = bootstrap.draw_counts(len(groups[2]), 3, seed=6).cpu().numpy()  # the device's own counts
    got = _host(rep)
    for b in range(4):
        idx = np.arange(300) if b == 3 else bc.replicate_rows(counts[b], labels, K, groups)
        sel = torch.from_numpy(idx).to(DEV)
        cm, stats = _existing(d_probs[sel], d_labels[sel], d_u[sel], K)
        assert np.array_equal(got["cm"][b], cm), b
        err = float(np.abs(got["stats"][b] - np.array(stats)).max())
        _log(f"existing kernels, replicate {b}", err, GATE)
        assert err <= GATE, (b, got["stats"][b], stats)


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_and_a_replicate_does_not_depend_on_B():
    probs, labels, u = bc.metric_case(1000, 4, seed=14)
    groups = selective.build_groups(bc.random_groups(1000, seed=15))
    args = _dev(probs, labels, u)
    a, b = _host(bootstrap.replicates(*args, groups=groups, B=64, seed=9)), _host(bootstrap.replicates(*args, groups=groups, B=64, seed=9))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    few = _host(bootstrap.replicates(*args, groups=groups, B=5, seed=9))
    for k in a:
        assert few[k][:5].tobytes() == a[k][:5].tobytes() and few[k][5].tobytes() == a[k][64].tobytes(), k
    other = _host(bootstrap.replicates(*args, groups=groups, B=5, seed=10))
    assert not np.array_equal(other["cm"][:5], few["cm"][:5]) and np.array_equal(other["cm"][5], few["cm"][5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        no_u = bootstrap.replicates(args[0], args[1], None, groups=groups, B=5, seed=9)
    side.synchronize()
    no_u = _host(no_u)
    assert np.isnan(no_u["stats"][:, 4:]).all() and no_u["stats"][:, :4].tobytes() == few["stats"][:, :4].tobytes()
    assert np.array_equal(no_u["u2"], few["u2"])


# ---- through the public entries ------------------------------------------------------------------------------------------------------------
def _without_ci(res):
    return {k: v for k, v in res.items() if k != "ci"}


def test_selective_evaluator_finish_with_bootstrap():
    rng = np.random.default_rng(16)
    Bt, nb, K = 7, 9, 4
    names = [f"cine{g}" for g in range(11)]
    keys = [names[int(g)] for g in rng.integers(0, len(names), Bt * nb)]  # repeated file names, interleaved
    y = np.array([names.index(k) % 3 for k in keys])
    lg = np.random.default_rng(17).uniform(-4.0, 4.0, (Bt * nb, K)).astype(np.float32)
    sel = selective.SelectiveEvaluator(_Head().to(DEV), abstain_class=True, capacity=8)
    for b in range(nb):
        s = slice(b * Bt, (b + 1) * Bt)
        sel.update(torch.from_numpy(lg[s]).to(DEV), torch.rand(Bt, 8, device=DEV), torch.from_numpy(y[s]).to(DEV), keys[s])
    probs, labels = sel.ev.probs[: sel.ev.rows], sel.ev.labels[: sel.ev.rows]
    u = selective.uncertainty(sel.ev.logits[: sel.ev.rows], True)
    groups = selective.build_groups(keys)
    for level, unit, rows in (("clip", "cine", (probs, labels, u, groups)), ("clip", "clip", (probs, labels, u, None)), ("cine", "cine", None)):
        plain = sel.finish(level=level)
        res = sel.finish(level=level, bootstrap=64, seed=3, confidence=0.9, unit=unit)
        assert "ci" not in plain and _same(_without_ci(res), plain)  # every other key is bitwise the bootstrap=0 result
        if rows is None:  # the rows are the cine predictions, every cine its own unit
            gp = selective.group_predictions(probs, u, labels, groups)
            rows = (gp.p_conf.float(), gp.labels, gp.u_mean.float(), None)
        want = bootstrap.intervals(bootstrap.replicates(*rows[:3], groups=rows[3], B=64, seed=3), 0.9)
        assert _same(res["ci"], want), (level, unit)
        assert list(res["ci"]) == list(bootstrap.STAT_NAMES) and res["ci"]["acc"]["n_finite"] == 64
        assert abs(res["ci"]["aurc"]["point"] - res["aurc"]) <= GATE and abs(res["ci"]["error_auroc"]["point"] - res["error_auroc"]) <= GATE
        if level == "cine":
            assert abs(res["ci"]["auc"]["point"] - res["auc"]) <= GATE and abs(res["ci"]["bal_acc"]["point"] - res["accuracy"]) <= GATE
    wide, narrow = sel.finish(level="clip", bootstrap=64, seed=3)["ci"]["acc"], sel.finish(level="clip", bootstrap=64, seed=3, unit="clip")["ci"]["acc"]
    assert wide["point"] == narrow["point"] and wide["se"] != narrow["se"]


@pytest.mark.timeout(900)
def test_trainer_evaluate_selective_with_bootstrap(tmp_path):
    from protoasnet_amd.trainer import DPTrainer

    m = synth_model(dict(CFG_VIDEO_X3D, num_classes=4, prototype_shape="(40, 256, 1, 1, 1)")).to(DEV)
    cfg = {"abstain_class": True, "save_dir": "", "train": TRAIN_CFG}
    loader = _cine_loader(4, 3, 70)
    t = DPTrainer(m, cfg, {"train": loader, "val": loader, "test": loader}, log=lambda *_: None)
    plain = t.evaluate_selective("test", level="clip")
    res = t.evaluate_selective("test", level="clip", bootstrap=16, seed=5)
    assert _same(_without_ci(res), plain) and "ci" not in plain
    sel = selective.SelectiveEvaluator(m, abstain_class=True)
    with torch.no_grad():
        for b in loader:
            lg, sim, _ = m(b["cine"].to(DEV))
            sel.update(lg, sim, b["target_AS"].to(DEV), b["filename"])
    ev = sel.ev
    u = selective.uncertainty(ev.logits[: ev.rows], True)
    want = bootstrap.intervals(bootstrap.replicates(ev.probs[: ev.rows], ev.labels[: ev.rows], u, selective.build_groups(sel.keys), B=16, seed=5))
    assert _same(res["ci"], want) and res["ci"]["acc"]["n_finite"] == 16
    cine = t.evaluate_selective("test", level="cine", bootstrap=16)
    assert cine["groups"] == 3 and cine["ci"]["acc"]["n_finite"] == 16 and _same(_without_ci(cine), t.evaluate_selective("test", level="cine"))
