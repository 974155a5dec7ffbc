"""Shared by tests/test_cpu_optim.py and tests/test_gpu_optim.py: a float64 restatement of the update ``torch.optim.Adam`` applies
(``amsgrad=False, maximize=False, decoupled_weight_decay=False``), and the gate the library's Adam is held to.

The restatement, per parameter that holds a gradient (a parameter without one is skipped: moments and t stay):

    t += 1;  g += wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)

The gate is measured, not fixed in advance: ``torch.optim.Adam`` on the device, fed the same fp32 gradients, is compared with the same
restatement, and the library may be off by at most 4 x torch's own largest error on that tensor plus one fp32 ulp of the tensor's
largest magnitude.  The factor allows a different, equally valid order of the handful of fp32 roundings per element; the ulp term
covers tensors on which torch happens to be exact."""
import math
import os

import numpy as np
import torch


class AdamRef:
    """``params``: tensors (copied to float64 on the CPU); ``group_of[i]``: index into ``groups`` (dicts with lr, betas, eps,
    weight_decay -- the keys of an optimizer's ``param_groups``, read at every step so that a scheduler's new lr is seen)."""

    def __init__(self, params, group_of, groups, exp_avg=None, exp_avg_sq=None, steps=None):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p] if exp_avg is None else [m.detach().double().cpu().clone() for m in exp_avg]
        self.v = [torch.zeros_like(p) for p in self.p] if exp_avg_sq is None else [v.detach().double().cpu().clone() for v in exp_avg_sq]
        self.t = [0] * len(self.p) if steps is None else [int(s) for s in steps]
        self.group_of, self.groups = list(group_of), groups

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            h = self.groups[self.group_of[i]]
            lr, (b1, b2), eps, wd = float(h["lr"]), h["betas"], float(h["eps"]), float(h["weight_decay"])
            self.t[i] += 1
            t = self.t[i]
            g = g.detach().double().cpu() + wd * self.p[i]
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.p[i] = self.p[i] - (lr / (1 - b1 ** t)) * self.m[i] / (self.v[i].sqrt() / math.sqrt(1 - b2 ** t) + eps)


def ulp32(x: float) -> float:
    """The spacing of fp32 at magnitude ``x``."""
    return float(np.spacing(np.float32(abs(x)))) if x != 0 else float(np.spacing(np.float32(0.0)))


def max_err(t: torch.Tensor, ref: torch.Tensor) -> float:
    return float((t.detach().double().cpu().reshape(-1) - ref.reshape(-1)).abs().max())


def gate(torch_err: float, ref: torch.Tensor) -> float:
    return 4.0 * torch_err + ulp32(float(ref.abs().max()))


def check(name: str, flat: torch.Tensor, torch_t: torch.Tensor, ref: torch.Tensor):
    """Both observed errors go to PASN_PARITY_LOG (profiles/optim_parity_observed.tsv) before the assertion; returns them."""
    e_flat, e_torch = max_err(flat, ref), max_err(torch_t, ref)
    bound = gate(e_torch, ref)
    log = os.environ.get("PASN_PARITY_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}\t{name}\tn={ref.numel()}\tflat_err={e_flat:.3g}\t"
                     f"torch_err={e_torch:.3g}\tgate={bound:.3g}\tmax|ref|={float(ref.abs().max()):.3g}\n")
    assert e_flat <= bound, f"{name}: FlatAdam is {e_flat:.3g} from the float64 restatement, torch.optim.Adam {e_torch:.3g}; gate {bound:.3g}"
    return e_flat, e_torch
