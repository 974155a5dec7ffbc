"""CPU: the grouped bootstrap -- Philox4x32-10 known answers, the numpy restatement of tests/bootstrap_cases.py (what the GPU tests hold
the kernels to) against cases worked out by hand, the interval arithmetic, and the C-ABI / Python surface with its argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bootstrap_cases as bc
import protoasnet_amd
from protoasnet_amd import _lib, bootstrap, selective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pasn_bootstrap_lds_max_groups", "pasn_bootstrap_counts", "pasn_bootstrap_workspace_bytes", "pasn_bootstrap_metrics")


# ---- draws -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """The Random123 known-answer vectors of Philox4x32-10."""
    out = bc.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert out.dtype == np.uint32 and " ".join(f"{int(x):08x}" for x in out) == want
    both = bc.philox4x32_10(np.array([counter, [0, 0, 0, 0]], dtype=np.uint64), np.array([key, [0, 0]], dtype=np.uint64))  # vectorised
    assert " ".join(f"{int(x):08x}" for x in both[0]) == want and f"{int(both[1][0]):08x}" == "6627e8d5"


def test_counts_ref_rows_sum_to_G_and_do_not_depend_on_B():
    for G in (1, 5, 64, 257, 4099):
        c = bc.counts_ref(G, 7, seed=3)
        assert c.dtype == np.int32 and c.shape == (7, G) and (c.sum(1) == G).all() and c.min() >= 0
        assert np.array_equal(bc.counts_ref(G, 3, seed=3), c[:3])  # a replicate is independent of B ...
        assert np.array_equal(bc.counts_ref(G, 2, seed=3, b0=4), c[4:6])  # ... and of the replicates before it
    assert bc.counts_ref(1, 3).tolist() == [[1], [1], [1]]
    a, b = bc.counts_ref(257, 2, seed=0), bc.counts_ref(257, 2, seed=1 << 32)
    assert not np.array_equal(a, b) and not np.array_equal(a[0], a[1])  # both key words and the replicate index matter
    # draw d is word d & 3 of call d >> 2: the fifth draw is word 0 of the second call
    r = bc.philox4x32_10(np.array([1, 2, 0, 0], dtype=np.uint64), np.array([9, 0], dtype=np.uint64))
    assert bc.draws_ref(5, 2, 9)[4] == (int(r[0]) * 5) >> 32


# ---- the restatement against a hand case ---------------------------------------------------------------------------------------------------
HAND_PROBS = np.array([[0.75, 0.25], [0.25, 0.75], [0.5, 0.5], [0.25, 0.75], [0.75, 0.25], [0.5, 0.5]], dtype=np.float32)
HAND_LABELS = np.array([0, 1, 1, 0, 0, -1])
HAND_U = np.array([0.25, 0.125, 0.5, 0.5, 0.125, 0.0], dtype=np.float32)


def test_replicate_rows_by_hand():
    assert bc.replicate_rows([1, 2, 0, 1, 0, 3], HAND_LABELS, 2).tolist() == [0, 1, 1, 3]  # row 5 is padding: never, whatever its count
    groups = selective.build_groups(["a", "b", "a", "c", "b", "c"])  # a = rows 0, 2; b = 1, 4; c = 3, 5
    assert bc.replicate_rows([2, 0, 1], HAND_LABELS, 2, groups).tolist() == [0, 0, 2, 2, 3]  # ascending row index, copies adjacent
    assert bc.replicate_rows([1, 1], HAND_LABELS, 2, (np.array([0, 1, 3]), np.array([4, 0, 1]))).tolist() == [0, 1, 4]  # unlisted rows stay out
    assert bc.replicate_rows([1, 1, 1, 1, 1, 1], np.array([0, 2, 1, 0, 0, -1]), 2).tolist() == [0, 2, 3, 4]  # label >= K_real is padding


def test_stats_of_rows_by_hand():
    """Rows 0, 1, 1, 2, 3 of the hand case: a doubled row (1) and a tie in both class columns (row 2's 0.5 meets nobody else's, but rows 1
    and 3 share 0.25 / 0.75).  Predictions (first largest): 0, 1, 1, 0, 1; labels 0, 1, 1, 1, 0."""
    idx = np.array([0, 1, 1, 2, 3])
    r = bc.stats_of_rows(HAND_PROBS, HAND_LABELS, HAND_U, idx)
    assert r["cm"].tolist() == [[1, 1], [1, 2]]
    acc, bal, f1 = r["stats"][:3]
    assert acc == 3 / 5 and bal == (1 / 2 + 2 / 3) / 2 and np.isclose(f1, (2 * 1 / (2 + 2) + 2 * 2 / (3 + 3)) / 2, rtol=1e-15, atol=0)
    # class 0: positives (rows 0, 3) score 0.75, 0.25; negatives (1, 1, 2) score 0.25, 0.25, 0.5.
    #   0.75 beats all three: 2 * 3 = 6; 0.25 ties two and loses to one: 2.  U2 = 8 of 2 * 2 * 3 = 12
    # class 1: positives (1, 1, 2) score 0.75, 0.75, 0.5; negatives (0, 3) score 0.25, 0.75.
    #   0.75: beats 0.25 (2), ties 0.75 (1) = 3, twice; 0.5: beats 0.25 = 2.  U2 = 8 of 12
    assert r["u2"].tolist() == [8, 8] and r["n_pos"].tolist() == [2, 3] and r["n_neg"].tolist() == [3, 2]
    assert np.isclose(r["stats"][3], (2 * (8 / 12) + 3 * (8 / 12)) / 5, rtol=1e-15, atol=0)
    # u order: rows 1, 1 (0.125), 0 (0.25), then the tie at 0.5: row 2 before row 3.  Right / wrong: R R R W W
    assert np.isclose(r["stats"][4], (0 + 0 + 0 + 1 / 4 + 2 / 5) / 5, rtol=1e-15, atol=0)
    assert r["stats"][5] == 1.0  # both wrong rows are more uncertain than every right one
    # without u the last two are NaN; a replicate that lost class 1 has no AUC, and its other statistics stand
    r = bc.stats_of_rows(HAND_PROBS, HAND_LABELS, None, np.array([0, 3, 3]))
    assert np.isnan(r["stats"][3:]).all() and r["stats"][0] == 1 / 3 and r["n_pos"].tolist() == [3, 0] and r["u2"].tolist() == [0, 0]
    # every row right: no error AUROC; a NaN u among the rows: none either, but the risk-coverage area stands (NaN goes last)
    assert np.isnan(bc.stats_of_rows(HAND_PROBS, HAND_LABELS, HAND_U, np.array([0, 1, 4]))["stats"][5])
    u = HAND_U.copy()
    u[0] = np.nan
    r = bc.stats_of_rows(HAND_PROBS, HAND_LABELS, u, idx)
    assert np.isnan(r["stats"][5]) and np.isclose(r["stats"][4], (0 + 0 + 1 / 3 + 2 / 4 + 2 / 5) / 5, rtol=1e-15, atol=0)


def test_stats_ref_point_row_and_group_expansion():
    probs, labels, u = bc.metric_case(37, 3, seed=1)
    r = bc.stats_ref(probs, labels, u, None, B=3, seed=5)
    assert r["stats"].shape == (4, 6) and r["cm"].shape == (4, 3, 3) and r["u2"].shape == (4, 3)
    want = bc.stats_of_rows(probs, labels, u, np.arange(37))  # the point estimate: every count 1
    assert np.array_equal(r["stats"][3], want["stats"]) and np.array_equal(r["cm"][3], want["cm"])
    assert (r["cm"].sum((1, 2)) == 37).all()  # identity groups: a replicate has as many rows as the sample
    import metric_cases as mc

    assert abs(want["stats"][3] - mc.auc_ovr_weighted(probs, labels, 3)[0]) <= 1e-15  # where defined, pasn_roc_auc_ovr's number
    one = selective.build_groups(["all"] * 37)
    g = bc.stats_ref(probs, labels, u, one, B=2, seed=5)
    assert np.array_equal(g["stats"][0], g["stats"][2]) and np.array_equal(g["cm"][1], g["cm"][2])  # G = 1: every replicate is the sample
    # the cases whose finite count the GPU tests rely on
    assert len(np.unique(probs[:, 0])) <= 9 and len(np.unique(u)) <= 8 and np.bincount(labels).tolist() == [13, 12, 12]
    assert np.isnan(bc.metric_case(37, 3, 1, "nan")[2]).sum() == 2 and (bc.metric_case(300, 4, 1, "pad")[1] == -1).sum() > 10
    keys = bc.random_groups(300, 2)
    sizes = np.diff(selective.build_groups(keys)[0])
    assert sizes.min() >= 1 and sizes.max() <= 9 and sizes.sum() == 300


# ---- intervals ---------------------------------------------------------------------------------------------------------------------------
def test_interval_arithmetic():
    stats = np.zeros((6, 6))
    stats[:5, 0] = [0.1, 0.5, 0.2, 0.4, 0.3]
    stats[:5, 3] = [0.6, np.nan, 0.8, np.nan, 0.7]  # two replicates lost a class
    stats[:5, 4] = [np.nan, np.nan, np.nan, 0.25, np.nan]  # one finite value: no interval
    stats[:5, 5] = np.nan
    stats[5] = [0.3, 0, 0, 0.7, 0.2, np.nan]
    ci = bootstrap.intervals_of(stats, 0.5)
    a = ci["acc"]  # quartiles of 0.1 .. 0.5 by linear interpolation: 0.2 and 0.4
    assert a["point"] == 0.3 and np.isclose(a["lo"], 0.2, rtol=1e-15) and np.isclose(a["hi"], 0.4, rtol=1e-15) and a["n_finite"] == 5
    assert np.isclose(a["se"], np.sqrt(0.1 / 4), rtol=1e-15)  # ddof = 1: sum of squares 0.1 over 4
    a = ci["auc"]  # the finite ones: 0.6, 0.7, 0.8
    assert a["n_finite"] == 3 and np.isclose(a["lo"], 0.65, rtol=1e-15) and np.isclose(a["hi"], 0.75, rtol=1e-15) and np.isclose(a["se"], 0.1, rtol=1e-14)
    for name, n in (("aurc", 1), ("error_auroc", 0)):
        assert ci[name]["n_finite"] == n and all(np.isnan(ci[name][k]) for k in ("lo", "hi", "se"))
    assert ci["aurc"]["point"] == 0.2 and np.isnan(ci["error_auroc"]["point"])
    ci95 = bootstrap.intervals_of(stats)
    assert np.isclose(ci95["acc"]["lo"], 0.1 + 0.025 * 4 * 0.1, rtol=1e-14) and list(ci95) == list(bootstrap.STAT_NAMES)
    want = bc.intervals_ref(stats, 0.9)
    got = bootstrap.intervals_of(torch.from_numpy(stats), 0.9)
    assert all(np.array_equal([got[n][k] for k in got[n]], [want[n][k] for k in want[n]], equal_nan=True) for n in got)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="confidence"):
            bootstrap.intervals_of(stats, bad)
    with pytest.raises(ValueError, match="stats"):
        bootstrap.intervals_of(np.zeros((1, 6)))


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
    assert "bootstrap" in protoasnet_amd.__all__ and protoasnet_amd.bootstrap is bootstrap  # exported lazily, like its neighbours
    bound = int(re.search(r"#define PASN_BOOTSTRAP_LDS_MAX_G (\d+)", header).group(1))
    assert bootstrap.lds_max_groups() == bound and 1 < bound < 65536  # uint16 counts
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(d >> 2, b, 0, 0)"):  # the header states the generator
        assert word in raw, word


def test_c_abi_rejects_bad_arguments_before_launching():
    lib = _lib.lib()
    fake = 256  # never dereferenced: every call below fails its argument checks first

    def counts(G=5, B=3, b0=0, out=fake):
        return lib.pasn_bootstrap_counts(out, G, B, 7, b0, 0)

    def run(M=100, G=100, K_real=3, B=5, **null):
        a = dict(probs=fake, labels=fake, u=fake, offsets=0, rows=0)
        p = dict(stats=fake, cm=fake, u2=fake, n_pos=fake, n_neg=fake, workspace=fake)
        a.update({k: v for k, v in null.items() if k in a})
        p.update({k: v for k, v in null.items() if k in p})
        return lib.pasn_bootstrap_metrics(*a.values(), M, G, K_real, B, 7, *p.values(), 0)

    size = lib.pasn_bootstrap_workspace_bytes
    for K_real in (1, 17):
        assert run(K_real=K_real) == 1 and size(100, 100, K_real, 5) == 0
    with pytest.raises(ValueError, match="K_real"):
        _lib.check(run(K_real=17))
    for M in (0, (1 << 20) + 1):
        assert run(M=M, G=M) == 1 and size(M, M, 3, 5) == 0
    for G in (0, 101):
        assert run(G=G, offsets=fake, rows=fake) == 1 and size(100, G, 3, 5) == 0
    for B in (0, 65537):
        assert run(B=B) == 1 and size(100, 100, 3, B) == 0 and counts(B=B) == 1
    for G in (0, (1 << 20) + 1):
        assert counts(G=G) == 1
    assert counts(out=0) == 1 and counts(b0=-1) == 1 and counts(b0=(1 << 31) - 2) == 1
    assert run(G=50) == 1  # without groups every row is its own group
    with pytest.raises(ValueError, match="G must equal M"):
        _lib.check(run(G=50))
    assert run(offsets=fake) == 1 and run(rows=fake) == 1  # the two CSR arrays come together
    for k in ("probs", "labels", "stats", "cm", "u2", "n_pos", "n_neg", "workspace"):
        assert run(**{k: 0}) == 1, k
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(run(workspace=0))
    assert run(workspace=264) == 1  # misaligned
    # the workspace: per order (K_real class columns and u) the words and keys of every position, padded to sweep chunks of 2048, and
    # the ranks; group and info words per row; above the LDS bound the blocks' count slices
    assert size(2500, 2500, 3, 100) == 4 * (2 * 4096 * 4 + 2500 * 4) + 2 * 2500 * 4
    bound = bootstrap.lds_max_groups()
    M = bound + 1
    shared = 3 * (2 * 9 * 2048 * 4 + M * 4) + 2 * M * 4
    assert size(M, bound, 2, 5) == shared and size(M, M, 2, 5) == shared + 6 * M * 4  # a slice per block: B + 1 blocks at most


def test_python_surface_checks_its_arguments():
    probs, labels, u = torch.rand(4, 3), torch.zeros(4, dtype=torch.int64), torch.rand(4)
    with pytest.raises(RuntimeError, match="GPU only"):
        bootstrap.replicates(probs, labels, u, B=4)
    with pytest.raises(RuntimeError, match="GPU only"):
        bootstrap.draw_counts(5, 3, device="cpu")
    for bad in (dict(B=0), dict(B=65537), dict(B=2.5), dict(seed=-1), dict(seed=1 << 64), dict(G=0), dict(G=(1 << 20) + 1), dict(b0=-1)):
        with pytest.raises(ValueError):
            bootstrap.draw_counts(**{"G": 5, "B": 3, **bad})
    for bad in (dict(B=0), dict(seed=-1)):  # checked before anything touches the device
        with pytest.raises(ValueError):
            bootstrap._check_B_seed(**{"B": 5, "seed": 0, **bad})

    # finish checks its own arguments before it looks at the rows
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    for bad in (dict(unit="patient"), dict(bootstrap=-1), dict(bootstrap=1.5), dict(bootstrap=True), dict(bootstrap=4, confidence=1.0),
                dict(bootstrap=4, seed=-1), dict(bootstrap=65537), dict(level="patient")):
        with pytest.raises(ValueError):
            sel.finish(**bad)


def test_bootstrap_zero_is_the_call_as_it_was(monkeypatch):
    """``bootstrap=0`` (the default) adds no key and calls nothing of the new module: ``finish`` on stubbed device functions."""
    import inspect

    sig = inspect.signature(selective.SelectiveEvaluator.finish)
    assert [sig.parameters[k].default for k in ("bootstrap", "seed", "confidence", "unit")] == [0, 0, 0.95, "cine"]
    from protoasnet_amd.trainer import DPTrainer

    sig = inspect.signature(DPTrainer.evaluate_selective)
    assert [sig.parameters[k].default for k in ("bootstrap", "seed", "confidence", "unit")] == [0, 0, 0.95, "cine"]
    cs = [1.0, 0.5]

    class RC:
        def packed(self, coverages):
            return torch.tensor([0.5, 1.0, 0.4, 0.9, 0.3, 0.8, 0.75, 0.25, 6, 3, 0.25, 0.7, 6, 1], dtype=torch.float64)

    class Ev:
        K_real, rows = 2, 6
        probs, labels, logits = torch.zeros(6, 2), torch.zeros(6, dtype=torch.int32), torch.zeros(6, 3)

    def no_bootstrap(*a, **k):
        raise AssertionError("bootstrap=0 must not reach the bootstrap module")

    monkeypatch.setattr(selective, "uncertainty", lambda *a, **k: torch.zeros(6))
    monkeypatch.setattr(selective, "risk_coverage", lambda *a, **k: RC())
    monkeypatch.setattr(bootstrap, "replicates", no_bootstrap)
    sel = selective.SelectiveEvaluator.__new__(selective.SelectiveEvaluator)
    sel.ev, sel.keys, sel.abstain, sel.score, sel.ab_logitpath = Ev(), list("aabbcc"), True, "auto", "joined"
    res = sel.finish(cs, level="clip")
    assert "ci" not in res and sorted(res) == sorted(
        ["aurc", "error_auroc", "rows", "nan_rows"] + [f"{n}@{c}" for n in ("accuracy", "bal_accuracy", "f1_mean", "threshold") for c in ("1", "0.5")])
    assert res == sel.finish(cs, level="clip", bootstrap=0, seed=9, confidence=0.5, unit="clip")
    with pytest.raises(AssertionError, match="must not reach"):
        sel.finish(cs, level="clip", bootstrap=8)
