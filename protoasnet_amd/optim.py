"""The optimizer side of a training step in the library: ``FlatAdam`` (one ``pasn_adam_step`` launch for every parameter that holds a
gradient) and ``GradAccumulator`` (at most two launches per micro-batch instead of autograd's one ``add_`` per parameter tensor).

What they replace: ``optimizer.step()`` and the undivided accumulation over micro-batches of ``Video_XProtoNet_e2e.py:137-142``, for the
optimizer all six of the reference's YAMLs select (``name: 'Adam'``, groups of ``XProtoNet_e2e.py:36-82``).  Opt-in
(``train.fused_optimizer`` in ``trainer.DPTrainer``); ``torch.optim.Adam`` stays the default.

Both drive a job table in device memory (csrc/optim.hip, the pattern of ``train.build_pack_tables``).  A table holds raw pointers, so
it is valid exactly as long as every tensor it names stays where it is: it is keyed by those pointers and built anew -- into freshly
allocated host and device memory, never over a table an earlier copy or launch may still read -- when one of them has moved.  The
training pass hands out its gradients in a fresh buffer per pass, which the caching allocator serves from the same one or two blocks
in steady state, so a few recent tables are kept.
"""
from __future__ import annotations

from collections import Counter, OrderedDict
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, dp

ADAM_JOB = np.dtype([("param", "u8"), ("grad", "u8"), ("exp_avg", "u8"), ("exp_avg_sq", "u8"), ("step", "u8"), ("n", "i8"),
                     ("group", "i4"), ("reserved", "i4")], align=True)  # struct pasn_adam_job
ACCUM_JOB = np.dtype([("dst", "u8"), ("src", "u8"), ("n", "i8")], align=True)  # struct pasn_accum_job
assert ADAM_JOB.itemsize == 56 and ACCUM_JOB.itemsize == 24
KEPT_TABLES = 4


def optim_chunk() -> int:
    return int(_lib.lib().pasn_optim_chunk())


def build_block_tables(sizes: Sequence[int], chunk: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(block_job, block_chunk)`` for jobs of ``sizes`` elements: block b works on elements ``[block_chunk[b] * chunk,
    (block_chunk[b] + 1) * chunk)`` of job ``block_job[b]`` (clipped to the job's size).  A pure function of its arguments."""
    sizes = np.asarray(sizes, dtype=np.int64)
    if sizes.ndim != 1 or (sizes <= 0).any() or chunk <= 0:
        raise ValueError("every job needs a positive size and the chunk must be positive")
    nb = (sizes + chunk - 1) // chunk
    first = np.cumsum(nb) - nb  # first block of each job
    block_job = np.repeat(np.arange(len(sizes), dtype=np.int64), nb)
    block_chunk = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(first, nb)
    return block_job.astype(np.int32), block_chunk.astype(np.int32)


class _Tables:
    """One job table on the host (the library checks it before the launch) and on the device (jobs, block_job, block_chunk in ONE
    freshly allocated buffer, one upload)."""

    def __init__(self, jobs: np.ndarray, device):
        bj, bc = build_block_tables(jobs["n"], optim_chunk())
        jb = jobs.view(np.uint8).reshape(-1)
        off = (jb.size + 15) // 16 * 16
        host = np.zeros(off + 4 * (bj.size + bc.size), dtype=np.uint8)
        host[: jb.size] = jb
        host[off: off + 4 * bj.size] = bj.view(np.uint8)
        host[off + 4 * bj.size:] = bc.view(np.uint8)
        self.host_jobs, self.njobs, self.nblocks = jobs, len(jobs), int(bj.size)
        self.dev = torch.from_numpy(host).to(device)  # a new allocation: nothing in flight can be reading it
        base = self.dev.data_ptr()
        self.jobs_ptr, self.bj_ptr, self.bc_ptr = base, base + off, base + off + 4 * bj.size


class _Recent(OrderedDict):
    """The last few tables by pointer key."""

    def lookup(self, key, make):
        t = self.get(key)
        if t is None:
            t = self[key] = make()
            while len(self) > KEPT_TABLES:
                self.popitem(last=False)
        else:
            self.move_to_end(key)
        return t


def _adam_defaults() -> dict:
    """The ``param_groups`` keys this torch's Adam writes (they changed between releases): a checkpoint must move both ways."""
    return dict(torch.optim.Adam([torch.zeros(1)]).defaults)


class FlatAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (``amsgrad=False, maximize=False, decoupled_weight_decay=False``) whose ``step()`` is ONE library call.

    Parameters, gradients and moments must be fp32, contiguous and on one GPU (``ValueError`` / ``RuntimeError`` otherwise: there is no
    CPU fallback).  ``group['lr']`` and the other hyper-parameters are read at every step and passed by value, so ``StepLR`` /
    ``ReduceLROnPlateau`` attach unchanged.  A parameter without a gradient is skipped: its moments and its step count do not move.

    State: ``state[p]`` holds ``exp_avg`` and ``exp_avg_sq`` as torch's Adam does; the per-parameter step counts live in one device
    tensor that the kernel advances (one 8-byte word each: t in the low half, the stamp of the call that advanced it in the high half).
    ``state_dict()`` writes them as torch does (``step``: a float32 scalar on the host) and ``load_state_dict()`` takes them back, so a
    checkpoint of either optimizer resumes in the other."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, maximize: bool = False, decoupled_weight_decay: bool = False):
        if amsgrad or maximize or decoupled_weight_decay:
            raise ValueError("FlatAdam implements Adam with amsgrad=False, maximize=False, decoupled_weight_decay=False only")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FlatAdam takes lr as a float (it is passed to the kernel by value)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = _adam_defaults()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._steps: Optional[torch.Tensor] = None  # int64 [parameters]: the step words
        self._slot: Dict[torch.nn.Parameter, int] = {}
        self._loaded_steps: Dict[torch.nn.Parameter, int] = {}  # from load_state_dict, until the words are (re)built
        self._tables = _Recent()
        self._stamp = 0
        self.library_calls = 0  # pasn_adam_step calls so far (one per step() that found a gradient)

    # ---- step words ---------------------------------------------------------------------------------------------------------------
    def _all_params(self) -> List[torch.nn.Parameter]:
        return [p for g in self.param_groups for p in g["params"]]

    def _step_counts(self) -> Dict[torch.nn.Parameter, int]:
        counts = dict(self._loaded_steps)
        if self._steps is not None:
            words = self._steps.cpu().numpy()
            counts.update({p: int(words[i]) & 0xFFFFFFFF for p, i in self._slot.items() if p not in self._loaded_steps})
        return counts

    def _ensure_steps(self, device) -> None:
        params = self._all_params()
        if self._steps is not None and not self._loaded_steps and len(self._slot) == len(params) and self._steps.device == device:
            return
        counts = self._step_counts()
        self._slot = {p: i for i, p in enumerate(params)}
        words = np.array([counts.get(p, 0) for p in params], dtype=np.int64)  # stamp 0: no call has advanced them
        self._steps = torch.from_numpy(words).to(device)
        self._loaded_steps = {}
        self._tables.clear()

    # ---- the update ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"FlatAdam: {len(self.param_groups)} parameter groups; the kernel's argument block holds {_lib.OPTIM_MAX_GROUPS}")
        groups = (_lib.AdamGroup * len(self.param_groups))()
        work = []  # (parameter, gradient, exp_avg, exp_avg_sq, group index)
        device = None
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise ValueError("FlatAdam: a parameter group asks for amsgrad, maximize or decoupled_weight_decay")
            b1, b2 = group["betas"]
            groups[gi] = _lib.AdamGroup(float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FlatAdam: a parameter lives on the CPU; the HIP path has no CPU fallback")
                if g.layout != torch.strided or p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous():
                    raise ValueError(f"FlatAdam: parameters and gradients must be contiguous float32 (got {tuple(p.shape)} {p.dtype}, "
                                     f"gradient {g.dtype}, contiguous {p.is_contiguous()} / {g.is_contiguous()})")
                if device is None:
                    device = p.device
                elif p.device != device or g.device != device:
                    raise ValueError("FlatAdam: every parameter and gradient must live on one device")
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                work.append((p, g, st["exp_avg"], st["exp_avg_sq"], gi))
        if not work:
            return loss
        self._ensure_steps(device)
        key = (self._steps.data_ptr(),) + tuple(x for p, g, m, v, _ in work for x in (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()))
        tables = self._tables.lookup(key, lambda: self._build(work, device))
        self._stamp = self._stamp % 0xFFFFFFFF + 1  # never 0, never the previous call's
        with torch.cuda.device(device):
            _lib.check(_lib.lib().pasn_adam_step(tables.jobs_ptr, tables.host_jobs.ctypes.data, tables.njobs, tables.bj_ptr, tables.bc_ptr,
                                                 tables.nblocks, groups, len(groups), self._stamp, _lib.current_stream()))
        self.library_calls += 1
        return loss

    def _build(self, work, device) -> _Tables:
        jobs = np.zeros(len(work), dtype=ADAM_JOB)
        base = self._steps.data_ptr()
        for i, (p, g, m, v, gi) in enumerate(work):
            for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape or t.device != device:
                    raise ValueError(f"FlatAdam: state {name} of a parameter {tuple(p.shape)} must be a contiguous float32 tensor of its shape "
                                     "on its device")
            jobs[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), base + 8 * self._slot[p], p.numel(), gi, 0)
        return _Tables(jobs, device)

    # ---- checkpoints: torch.optim.Adam's format ----------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        sd = super().state_dict()
        counts = self._step_counts()  # the one device-to-host read: at checkpoint time only
        for i, p in enumerate(self._all_params()):  # the base class numbers the parameters in this order
            if i in sd["state"]:
                sd["state"][i] = {"step": torch.tensor(float(counts.get(p, 0)), dtype=torch.float32), **sd["state"][i]}
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        super().load_state_dict(state_dict)  # moments cast to their parameter's device and dtype; ``step`` left as it was saved
        counts = {}  # the loaded state alone defines the counts: a parameter it does not hold starts over, as under torch.optim.Adam
        for p, st in self.state.items():
            if "step" in st:
                counts[p] = int(round(float(st.pop("step"))))
        self._loaded_steps, self._steps, self._slot = counts, None, {}
        self._tables.clear()


class GradAccumulator:
    """Gradient accumulation over micro-batches without one ``add_`` launch per parameter.

    ``absorb()`` after every ``loss.backward()``: the first call of a window adopts the ``p.grad`` tensors as they are; later calls add
    the new gradients into the adopted ones -- one ``pasn_add_inplace`` over the flat span when both sides lie in one buffer with the
    same layout (``dp.flat_gradient_view``: the training pass's gradient buffer), one ``pasn_grad_accumulate`` for everything else --
    and every call leaves ``p.grad = None``, so autograd never accumulates per tensor.  ``materialize()`` puts the adopted tensors back
    as ``p.grad`` (then the all-reduce and the optimizer run as usual); ``reset()`` starts a new window.  Each element sees the adds
    ``dst.add_(src)`` would have made, in the same order: the sums are bitwise those of autograd's accumulation.

    Between micro-batches ``p.grad`` is ``None`` while the accumulator holds the gradients."""

    def __init__(self, params: Iterable[torch.nn.Parameter]):
        self.params = list(params)
        self._held: Optional[Dict[int, torch.Tensor]] = None
        self._held_key: tuple = ()
        self._plans = _Recent()
        self.library_calls = 0  # pasn_add_inplace + pasn_grad_accumulate calls so far

    def absorb(self) -> None:
        held, first = self._held, self._held is None
        if first:
            held = {}
        idx, dsts, srcs, src_ptrs = [], [], [], []
        adopted = False
        for i, p in enumerate(self.params):  # one pass: this runs once per micro-batch over every parameter tensor
            g = p.grad
            if g is None:
                continue
            p.grad = None
            have = held.get(i)
            if have is None:
                held[i] = g  # the window's first gradient of this parameter (also one gained inside a window): adopted as it is
                adopted = True
            else:
                idx.append(i)
                dsts.append(have)
                srcs.append(g)
                src_ptrs.append(g.data_ptr())
        if adopted:
            self._held = held
            # Every adopted gradient and where it lies, fixed until the next adoption.  ALL of them belong in a plan's key, not only the
            # ones being added to: whether the span add may be taken depends on every adopted gradient that lies inside the span.
            self._held_key = tuple((i, held[i].data_ptr()) for i in sorted(held))
        if dsts:
            self._add(dsts, srcs, (self._held_key, tuple(idx), tuple(src_ptrs)))

    def materialize(self) -> None:
        self.absorb()  # a backward since the last absorb() belongs to the window too (right after an absorb(): one pass that finds nothing)
        for i, g in (self._held or {}).items():
            self.params[i].grad = g

    def reset(self) -> None:
        self._held, self._held_key = None, ()

    # ---- dst += src for a list of pairs, at most two launches ------------------------------------------------------------------------
    def _add(self, dsts: List[torch.Tensor], srcs: List[torch.Tensor], key) -> None:
        d0 = dsts[0]
        if not d0.is_cuda:
            raise RuntimeError("GradAccumulator: a gradient lives on the CPU; the HIP path has no CPU fallback")
        span, tables = self._plans.lookup(key, lambda: self._plan(list(zip(dsts, srcs))))
        lib, st = _lib.lib(), _lib.current_stream()
        with torch.cuda.device(d0.device):
            if span is not None:
                _lib.check(lib.pasn_add_inplace(span[0], span[1], span[2], _lib.F32, st))
                self.library_calls += 1
            if tables is not None:
                _lib.check(lib.pasn_grad_accumulate(tables.jobs_ptr, tables.host_jobs.ctypes.data, tables.njobs, tables.bj_ptr, tables.bc_ptr,
                                                    tables.nblocks, st))
                self.library_calls += 1

    def _plan(self, pairs):
        """((dst pointer, src pointer, elements) of the span or None, table of the rest or None)."""
        for d, s in pairs:  # (a table is keyed by the pointers it holds: the same pointers are the same tensors, checked once)
            if s.shape != d.shape or s.dtype != d.dtype or s.device != d.device:
                raise ValueError("GradAccumulator: a gradient changed its shape, dtype or device inside a window")
            if d.dtype != torch.float32 or not d.is_contiguous() or not s.is_contiguous() or d.layout != torch.strided or s.layout != torch.strided:
                raise ValueError("GradAccumulator: gradients must be contiguous float32")
        span, rest = self._span(pairs)
        jobs = [(d.data_ptr(), s.data_ptr(), d.numel()) for d, s in rest if d.numel()]
        if span is not None:
            fd, fs = span
            n8 = fd.numel() // 8 * 8  # pasn_add_inplace moves whole groups of 8; the few elements behind them ride with the rest
            if n8 < fd.numel():
                jobs.append((fd.data_ptr() + 4 * n8, fs.data_ptr() + 4 * n8, fd.numel() - n8))
            span = (fd.data_ptr(), fs.data_ptr(), n8)
        tables = _Tables(np.array(jobs, dtype=ACCUM_JOB), pairs[0][0].device) if jobs else None
        return span, tables

    def _span(self, pairs):
        """The pairs that lie in ONE destination buffer and ONE source buffer with the same layout, as two flat views, and the others."""
        where = Counter((d.untyped_storage().data_ptr(), s.untyped_storage().data_ptr()) for d, s in pairs)
        (dbase, sbase), count = where.most_common(1)[0]
        if count < 2:
            return None, pairs
        inside = [(d, s) for d, s in pairs if d.untyped_storage().data_ptr() == dbase and s.untyped_storage().data_ptr() == sbase]
        fd, fs = dp.flat_gradient_view([d for d, _ in inside]), dp.flat_gradient_view([s for _, s in inside])
        if fd is None or fs is None or fd.numel() != fs.numel() or fd.numel() < 8 or (fd.data_ptr() | fs.data_ptr()) % 16:
            return None, pairs
        if any(d.storage_offset() - fd.storage_offset() != s.storage_offset() - fs.storage_offset() for d, s in inside):
            return None, pairs
        # the span add touches everything between its first and last gradient: no adopted gradient that is NOT one of these pairs may lie there
        lo, hi = fd.storage_offset(), fd.storage_offset() + fd.numel()
        mine = {d.data_ptr() for d, _ in inside}
        for h in self._held.values():
            if h.data_ptr() not in mine and h.untyped_storage().data_ptr() == dbase and h.storage_offset() < hi and h.storage_offset() + h.numel() > lo:
                return None, pairs
        return (fd, fs), [(d, s) for d, s in pairs if not (d.untyped_storage().data_ptr() == dbase and s.untyped_storage().data_ptr() == sbase)]
