#!/usr/bin/env python3
"""G9: golden fixtures of the evaluation metrics, produced by RUNNING THE REFERENCE'S OWN CODE on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

Runs only in the build container (needs the reference tree).  Nothing of the reference is copied here, only the numbers it produces:

* sparsity: ``src/utils/metrics.py`` is imported as it lies.  ``torchmetrics`` is absent from this image: a placeholder ``Metric``
  whose ``add_state`` sets the attribute and whose ``__call__`` calls the reference's own ``update_and_compute`` is registered first.
  The metric runs over the seeded batches of ``tests/metric_cases.py::sparsity_batches``; per-batch values and ``compute()`` are stored.
* AUC (only if sklearn is installed): ``roc_auc_score(y, p, average="weighted", multi_class="ovr", labels=range(3))`` on
  ``metric_cases.auc_cases``; where it raises, 0.0 -- the reference's ``except ValueError: AUC = 0`` (Video_XProtoNet_e2e.py:256-266).
  A class without positive rows raises in the sklearn the reference pins; sklearn >= 1.6 only warns (UndefinedMetricWarning) and drops
  the class, so that warning is taken as the raise.
* prediction log (only if pandas is installed): ``BaseAgent.create_pred_log_df`` (src/agents/base.py:195-211) called as an unbound
  function on ``metric_cases.pred_log_batch`` with ``wandb``, ``torchsummary`` and the dataset / model imports stubbed; its
  ``reset_index(drop=True).to_csv()`` text is stored as g9_pred_log.csv.

A missing library is reported and its part skipped; the tests then hold the kernels to the restatements and hand cases only.
"""
import os
import importlib.util
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("PASN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)

import metric_cases as mc  # noqa: E402


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)
    return sys.modules[name]


class _Metric:
    def __init__(self, dist_sync_on_step=False):
        self._defaults = {}

    def add_state(self, name, default, dist_reduce_fx=None):
        self._defaults[name] = default.clone()
        setattr(self, name, default.clone())

    def reset(self):
        for k, v in self._defaults.items():
            setattr(self, k, v.clone())

    def __call__(self, *a, **k):
        return self.update_and_compute(*a, **k)


_placeholder("torchmetrics", Metric=_Metric)


def sparsity(out):
    from src.utils.metrics import SparsityMetric  # noqa: E402  (reference)

    for case, batches in mc.sparsity_batches().items():
        m = SparsityMetric(level=mc.LEVEL, device="cpu")
        vals = [float(m(b)) for b in batches]
        out[f"sparsity_{case}_batch"] = np.array(vals, dtype=np.float32)
        out[f"sparsity_{case}_epoch"] = np.array(float(m.compute()), dtype=np.float32)
        out[f"sparsity_{case}_sum"] = np.array([int(m.percentage_expl), int(m.total)], dtype=np.int64)
        print("sparsity", case, vals, float(m.compute()))


def auc(out):
    try:
        from sklearn.metrics import roc_auc_score
    except ImportError:
        print("sklearn is not installed: no AUC fixtures (the tests use the restatement and hand cases)")
        return
    from sklearn.exceptions import UndefinedMetricWarning

    for case, (p, y) in mc.auc_cases().items():
        try:
            with warnings.catch_warnings():
                # sklearn < 1.6 raises ValueError for a class without positives; later versions warn and drop the class.  The reference's
                # pinned sklearn raises, so the warning counts as the raise.
                warnings.simplefilter("error", UndefinedMetricWarning)
                a = roc_auc_score(y, p, average="weighted", multi_class="ovr", labels=range(3))
        except (ValueError, UndefinedMetricWarning) as e:
            print(f"auc {case}: sklearn raised ({e}); the reference stores 0")
            a = 0.0
        out[f"auc_{case}"] = np.array(a, dtype=np.float64)
        print("auc", case, a)


def pred_log():
    try:
        import pandas  # noqa: F401
    except ImportError:
        print("pandas is not installed: no prediction-log fixture (the tests use the hand cases)")
        return
    _placeholder("wandb")
    _placeholder("torchsummary", summary=lambda *a, **k: None)
    _placeholder("src.models", model_builder=types.ModuleType("model_builder"))
    _placeholder("src.utils.utils", print_cuda_statistics=lambda *a, **k: None)
    _placeholder("src.data.as_dataloader", get_as_dataloader=lambda *a, **k: None)
    # base.py alone: src/agents/__init__.py would import every agent and the dataset stack
    spec = importlib.util.spec_from_file_location("ref_agents_base", os.path.join(REF, "src", "agents", "base.py"))
    base = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(base)  # (reference)
    BaseAgent = base.BaseAgent

    b, logits = mc.pred_log_batch(optional=True)
    df = BaseAgent.create_pred_log_df(None, b, logits, mc.LOGIT_NAMES)
    text = df.reset_index(drop=True).to_csv()
    with open(os.path.join(HERE, "g9_pred_log.csv"), "w", newline="") as f:
        f.write(text)
    print(text)


def main():
    out = {}
    sparsity(out)
    auc(out)
    pred_log()
    path = os.path.join(HERE, "g9_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g9_metrics.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
