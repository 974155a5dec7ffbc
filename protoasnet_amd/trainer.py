"""Data-parallel training harness: the reference's agent loop around the compiled training step.

What it reproduces, with the reference lines it follows:

* optimizer groups and learning rates -- ``lr_same`` (all parameters, ``weight_decay=1e-3``) or ``lr_disjoint`` (trunk / add-on /
  occurrence module with weight decay, prototypes and last layer without): ``src/agents/XProtoNet_e2e.py:36-82``;
* the loss recipe and its classes: ``XProtoNet_Base.py:54-81`` + ``Video_XProtoNet_e2e.py:86-110`` (``protoasnet_amd.losses`` has the
  classes with the reference's names and ``compute`` signatures);
* gradient accumulation WITHOUT dividing the loss, ``optimizer.step()`` every ``accumulation_steps`` micro-batches:
  ``Video_XProtoNet_e2e.py:137-142``;
* ``ReduceLROnPlateau`` stepped on the validation mean F1 (``StepLR`` stepped unconditionally), the warm push at
  ``num_warm_epochs`` without replacement, the push every ``push_rate`` epochs from ``push_start`` followed by a ``val_push`` epoch:
  ``XProtoNet_e2e.py:110-148``;
* the checkpoint dictionary ``{epoch, iteration, state_dict, optimizer}`` and the files ``last.pth`` / ``model_best.pth`` /
  ``epoch_<k>.pth``: ``src/agents/base.py:143-169``, ``XProtoNet_e2e.py:84-107``.

What it changes, because it has to scale:

* **one process per GPU**; every rank iterates its own loader shard; parameter gradients are SUMMED over ranks in ONE all-reduce of
  the flat bucket at each accumulation boundary (``dp.allreduce_gradients``), and each rank accumulates ``accumulation_steps / world``
  micro-batches -- so W ranks x k micro-batches take exactly the optimizer step of one process with W*k micro-batches (tested);
* **no per-batch host synchronisation**: the reference calls ``.item()`` seven times and runs sklearn on every batch
  (``Video_XProtoNet_e2e.py:112-135,143-153``); here predictions feed a confusion matrix that stays on the device, the loss terms
  accumulate in a device vector, and both come to the host once per epoch (after one tiny all-reduce across ranks, so every rank
  takes the same scheduler / best-model decisions);
* ``TransformLoss`` is skipped when its ``loss_weight`` is 0 (the reference returns before the second trunk pass too: loss.py:284);
  in ``val`` / ``val_push`` epochs -- where the reference computes the term as well (``Video_XProtoNet_e2e.py:72,98``) -- the warped clips
  ride in the SAME forward as the originals (one 2N-clip launch list; exact in eval mode, where the norm layers use running statistics);
* **every rank holds the same model**: parameters and buffers are broadcast from rank 0 at construction; the norm layers' running
  estimates (updated per rank from its own micro-batches, as under plain BatchNorm) are averaged over the ranks before every
  evaluation epoch, push and checkpoint, so all ranks evaluate, project and save ONE model;
* every rank must bring the same number of micro-batches per epoch (checked with one MIN/MAX all-reduce at the start of the epoch: a
  rank with fewer would issue fewer gradient all-reduces and hang the job); gradients of a trailing partial accumulation are kept
  across the epoch boundary, as the reference keeps them (it never zeroes at the start of an epoch).

Evaluation metrics (``protoasnet_amd.metrics``): on a GPU model every epoch, in every mode as in the reference, also accumulates the
weighted one-vs-rest ROC AUC, the prototype sparsity, the diversity counters and the similarity sums on the device (one launch per batch;
Video_XProtoNet_e2e.py:154-173, 256-281) and returns them with the confusion-matrix metrics; ``val_push`` / ``test`` epochs write the
reference's per-clip prediction CSV (``save_dir/csv_<mode>/e<epoch>_f1_<f1>.csv``, :313-319).  Across ranks the additive counters ride in
the one per-epoch all-reduce, the AUC sees every rank's rows (one ``all_gather``), and the CSV rows reach rank 0 rank-major: rank 0's
clips in its loader order, then rank 1's, and so on.  ``evaluate(mode)`` is the reference's ``eval_only`` entry (main.py:52-53).

``train.fused_optimizer`` (not a key of the reference's configs; default off): Adam's update as one library call per optimizer step and
the micro-batches' gradients summed in at most two (``protoasnet_amd.optim``); ``p.grad`` is ``None`` between micro-batches then.

Out of scope: wandb, plots, the ``classification_report`` text.
"""
from __future__ import annotations

import contextlib
import logging
import os
from copy import deepcopy
from typing import Dict, Optional, Sequence

import torch
import torch.distributed as dist

from . import _lib, data, dp, losses, metrics as metrics_mod
from . import push as push_mod


def confusion_to_metrics(cm: torch.Tensor) -> Dict[str, object]:
    """Balanced accuracy and per-class F1 (``zero_division=0``) from a (K, K) confusion matrix [true, predicted] -- what
    ``sklearn.metrics.balanced_accuracy_score`` / ``f1_score(average=None, labels=range(K))`` return (Video_XProtoNet_e2e.py:244-252)."""
    cm = cm.double()
    tp = cm.diag()
    support, predicted = cm.sum(1), cm.sum(0)
    recall = torch.where(support > 0, tp / support.clamp(min=1), torch.zeros_like(tp))
    present = support > 0
    accu = float(recall[present].mean()) if bool(present.any()) else 0.0  # classes absent from y_true do not count
    denom = support + predicted
    f1 = torch.where(denom > 0, 2 * tp / denom.clamp(min=1), torch.zeros_like(tp))
    return {"accuracy": accu, "f1": f1.tolist(), "f1_mean": float(f1.mean())}


def _loader_capacity(loader) -> int:
    """``len(loader) * batch_size`` when the loader knows both, else 0: the rows a per-clip device buffer is sized for."""
    return len(loader) * int(getattr(loader, "batch_size", 0) or 0) if hasattr(loader, "__len__") else 0


class DPTrainer:
    """``config`` carries the reference's keys: ``abstain_class``, ``save_dir`` and ``train`` (``num_train_epochs``,
    ``num_warm_epochs``, ``accumulation_steps``, ``push_start``, ``push_rate``, ``save``, ``save_step``, ``criterion``, ``optimizer``,
    ``lr_schedule``) as in ``src/configs/Ours_ProtoASNet_Video.yml:19-74``.  ``data_loaders`` maps ``train`` / ``val`` /
    ``train_push`` to iterables of ``{"cine", "target_AS", "filename"}`` batches -- already sharded per rank for train / val (a
    ``DistributedSampler`` or disjoint file lists); the push loader is the FULL loader (the sweep shards it itself)."""

    def __init__(self, model: torch.nn.Module, config: dict, data_loaders: Dict[str, object], rank: int = 0, world_size: int = 1,
                 log=logging.info):
        self.model, self.config, self.train_config = model, config, config["train"]
        self.data_loaders, self.rank, self.world_size, self.log = data_loaders, rank, world_size, log
        acc = int(self.train_config.get("accumulation_steps", 1))
        if acc % world_size != 0:
            raise ValueError(f"accumulation_steps={acc} must be a multiple of the world size {world_size}: every rank accumulates "
                             "accumulation_steps / world micro-batches before the one gradient all-reduce")
        if world_size > 1 and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("DPTrainer(world_size > 1) needs an initialised process group (one process per GPU)")
        self.local_accumulation = acc // world_size
        self.device = next(model.parameters()).device
        self.current_epoch, self.current_iteration, self.best_metric = 0, 0, 0.0
        self.temperature_fit = None  # calibration.TemperatureFit of the last fit_temperature()
        self.conformal_fit = None  # conformal.ConformalFit of the last fit_conformal()
        self.operating_fit = None  # ordinal.OperatingFit of the last fit_operating_points()
        self.ood_fit = None  # ood.OODFit of the last fit_ood(), with its detector, level and thresholds
        self.num_real_classes = model.num_classes - 1 if config.get("abstain_class") else model.num_classes
        self.get_criterion()
        self.get_optimizer()
        self.scheduler = self.get_lr_scheduler()
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]
        self._clip_pipe = None  # built on the first single-channel batch (clip_pipeline)
        self._copy_stream = None  # side stream of raw-batch uploads (staged)
        self.sync_model_state()  # ranks built from different seeds / checkpoints would otherwise stay different models for ever

    # ---- one model on every rank ------------------------------------------------------------------------------------------------
    def sync_model_state(self) -> None:
        """Broadcast every parameter and buffer from rank 0 (what DistributedDataParallel does at construction)."""
        if self.world_size <= 1:
            return
        with torch.no_grad():
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                buf = push_mod._for_collective(t.detach())
                dist.broadcast(buf, src=0)
                if buf.data_ptr() != t.data_ptr():  # staged through the host (gloo rehearsal): bring it back; RCCL wrote t itself
                    t.copy_(buf.to(t.device))
        if hasattr(self.model, "cnn_backbone") and hasattr(self.model.cnn_backbone, "invalidate_plans"):
            self.model.cnn_backbone.invalidate_plans()  # a broadcast straight into the storage bumps no version counter
        self._norm_dirty = False

    def sync_norm_buffers(self) -> None:
        """Average the norm layers' running means / variances over the ranks and take the largest batch counter: each rank's estimates
        saw only its own micro-batches; evaluation, push and the checkpoint must use ONE model.

        Only when a training epoch ran since the last sync (``_norm_dirty``; every rank runs the same epochs, so the flag agrees
        across ranks and the collective stays matched): a sync of already-equal buffers would still ``copy_`` into every buffer, bump
        its version counter and make the next eval forward re-plan and re-pack every weight -- and for world sizes that are not powers
        of two ``(a + a + a) / 3`` need not be ``a``, so the statistics would drift by an ulp per call.  Only norm statistics are
        exchanged: ``prototype_class_identity``-like constants and ``ones`` are equal by construction."""
        if self.world_size <= 1:
            return
        norms = [m for m in self.model.modules() if isinstance(m, torch.nn.modules.batchnorm._NormBase) and m.running_mean is not None]
        # The decision to skip is COLLECTIVE (round 5, ADVICE): the local flag only knows about run_epoch("train"); a train-mode forward
        # outside it, or a per-rank load_state_dict, also moves the statistics.  One 3-word MAX-reduce: [any rank dirty, max, -min] of the
        # ranks' summed batch counters -- a sync runs when any rank trained since the last one or the counters disagree; every rank then
        # takes the same branch, so the collectives below stay matched.
        nbt = sum(int(m.num_batches_tracked) for m in norms if m.num_batches_tracked is not None)
        probe = torch.tensor([int(bool(getattr(self, "_norm_dirty", True))), nbt, -nbt], dtype=torch.int64, device=self.device)
        probe = push_mod._for_collective(probe)
        dist.all_reduce(probe, op=dist.ReduceOp.MAX)
        if int(probe[0]) == 0 and int(probe[1]) == -int(probe[2]):
            return
        fl = [b for m in norms for b in (m.running_mean, m.running_var)]
        it = [m.num_batches_tracked for m in norms if m.num_batches_tracked is not None]
        with torch.no_grad():
            if fl:
                flat = push_mod._for_collective(torch.cat([b.detach().float().flatten() for b in fl]))
                dist.all_reduce(flat)
                flat = (flat / self.world_size).to(self.device)
                o = 0
                for b in fl:
                    b.copy_(flat[o:o + b.numel()].view_as(b).to(b.dtype))
                    o += b.numel()
            if it:
                flat = push_mod._for_collective(torch.cat([b.detach().flatten().to(torch.int64) for b in it]))
                dist.all_reduce(flat, op=dist.ReduceOp.MAX)
                flat = flat.to(self.device)
                o = 0
                for b in it:
                    b.copy_(flat[o:o + b.numel()].view_as(b).to(b.dtype))
                    o += b.numel()
        self._norm_dirty = False

    # ---- reference surface: XProtoNet_Base.py:54-81 ---------------------------------------------------------------------------
    def get_criterion(self) -> None:
        cfg = deepcopy(self.train_config["criterion"])
        K = self.model.num_classes
        if self.config.get("abstain_class"):
            self.CeLoss = losses.CeLossAbstain(**cfg["CeLossAbstain"])
        else:
            self.CeLoss = losses.CeLoss(**cfg["CeLoss"])
        self.Cluster = losses.ClusterRoiFeat(num_classes=K, **cfg["ClusterRoiFeat"])
        self.Separation = losses.SeparationRoiFeat(num_classes=K, **cfg["SeparationRoiFeat"], abstain_class=bool(self.config.get("abstain_class")))
        self.Orthogonality = losses.OrthogonalityLoss(num_classes=K, **cfg["OrthogonalityLoss"])
        self.Lnorm_occurrence = losses.L_norm(**cfg["Lnorm_occurrence"])
        self.Trans_occurrence = losses.TransformLoss(**cfg["trans_occurrence"])
        self.Lnorm_fc = losses.L_norm(**cfg["Lnorm_FC"], mask=1 - torch.t(self.model.prototype_class_identity))
        # a pruned model whose classes own different numbers of prototypes: the class-grouped costs group by the class identity, not by
        # reshaping (N, P) to (N, K, P / K), so that an eval epoch reports the loss of the model as it stands (training refuses it)
        from . import prune

        balanced = prune.is_balanced(self.model)
        if not balanced:
            cls = prune.proto_classes(self.model)
            self.Cluster.proto_class = self.Separation.proto_class = self.Orthogonality.proto_class = cls
        # train.fused_loss (not a key of the reference's configs; default off): the same seven objects evaluated by one library call
        self.fused = None
        if self.train_config.get("fused_loss", False):
            if not balanced:
                prune.require_balanced(self.model, "train.fused_loss (the one-launch criterion indexes equal class blocks)")
            self.fused = losses.FusedCriterion(self.CeLoss, self.Cluster, self.Separation, self.Orthogonality, self.Lnorm_occurrence,
                                               self.Trans_occurrence, self.Lnorm_fc)

    # ---- XProtoNet_e2e.py:36-82 --------------------------------------------------------------------------------------------------
    def get_optimizer(self) -> None:
        cfg = deepcopy(self.train_config["optimizer"])
        name, mode = cfg.pop("name"), cfg.pop("mode")
        m = self.model
        if mode == "lr_same":
            specs = [{"params": m.parameters(), "lr": cfg["lr_same"], "weight_decay": 1e-3}]
        elif mode == "lr_disjoint":
            lr = cfg["lr_disjoint"]
            specs = [
                {"params": m.cnn_backbone.parameters(), "lr": lr["cnn_backbone"], "weight_decay": 1e-3},
                {"params": m.add_on_layers.parameters(), "lr": lr["add_on_layers"], "weight_decay": 1e-3},
                {"params": m.occurrence_module.parameters(), "lr": lr["occurrence_module"], "weight_decay": 1e-3},
                {"params": m.prototype_vectors, "lr": lr["prototype_vectors"]},
                {"params": m.last_layer.parameters(), "lr": lr["last_layer"]},
            ]
        else:
            raise ValueError(f"optimizer mode {mode} not valid.")
        # train.fused_optimizer (not a key of the reference's configs; default off): the same groups under optim.FlatAdam -- one library
        # call per optimizer step -- and the micro-batches' gradients summed by optim.GradAccumulator instead of autograd's per-tensor adds
        self.accumulator = None
        if self.train_config.get("fused_optimizer", False):
            if name != "Adam":
                raise ValueError(f"train.fused_optimizer implements Adam, the optimizer of the reference's configs; optimizer.name is {name!r}")
            from . import optim

            self.optimizer = optim.FlatAdam(specs)
            self.accumulator = optim.GradAccumulator(p for g in self.optimizer.param_groups for p in g["params"])
            return
        self.optimizer = torch.optim.__dict__[name](specs)

    def get_lr_scheduler(self):
        cfg = deepcopy(self.train_config["lr_schedule"])
        name = cfg.pop("name")
        cfg.pop("verbose", None)  # accepted by the torch 1.13 the reference pins, gone from current torch
        return torch.optim.lr_scheduler.__dict__[name](self.optimizer, **cfg)

    # ---- base.py:143-169, XProtoNet_e2e.py:84-107 ------------------------------------------------------------------------------
    def get_state(self) -> dict:
        state = {"epoch": self.current_epoch, "iteration": self.current_iteration, "state_dict": self.model.state_dict(),
                 "optimizer": self.optimizer.state_dict()}
        from . import prune

        pruned = prune.state(self.model)
        if pruned:  # (a model that was never pruned writes the keys it always wrote)
            state["pruned_prototypes"] = pruned  # indices into the model as built: load_checkpoint removes them before load_state_dict
        return state

    def save_checkpoint(self, is_best: bool = False) -> None:
        if not self.train_config.get("save", True):
            return
        self.sync_norm_buffers()  # a collective: every rank takes part before rank 0 writes
        if self.rank != 0:
            return
        state, d = self.get_state(), self.config["save_dir"]
        os.makedirs(d, exist_ok=True)
        step = self.train_config.get("save_step")
        if step is not None and self.current_epoch % step == 0:
            torch.save(state, os.path.join(d, f"epoch_{self.current_epoch}.pth"))
        if is_best:
            torch.save(state, os.path.join(d, "model_best.pth"))
        torch.save(state, os.path.join(d, "last.pth"))

    def load_checkpoint(self, file_name: Optional[str]) -> bool:
        if file_name is None or not os.path.exists(file_name):
            self.log(f"No checkpoint exists from '{file_name}'. Skipping...")
            return False
        ck = torch.load(file_name, map_location=self.device)
        self.current_epoch, self.current_iteration = ck["epoch"], ck["iteration"]
        if ck.get("pruned_prototypes"):
            from . import prune

            if prune.state(self.model) != list(ck["pruned_prototypes"]):
                prune.restore(self.model, ck["pruned_prototypes"])
                self._rebuild_after_surgery()
        self.model.load_state_dict(ck["state_dict"])
        self.optimizer.load_state_dict(ck["optimizer"])
        self.log(f"Checkpoint loaded successfully from '{file_name}' at (epoch {ck['epoch']}) at (iteration {ck['iteration']})")
        return True

    # ---- single-channel clips: augmentation and normalisation on the device --------------------------------------------------------
    def clip_pipeline(self) -> "data.DeviceClipPipeline":
        """The device input pipeline of single-channel batches, from the reference's ``data`` keys (augmentation, rotation, crop ratio,
        normalize); its generator is seeded by ``train.seed`` and the rank, so ranks draw different crops and a rerun draws the same."""
        if self._clip_pipe is None:
            seed = int(self.train_config.get("seed", 0) or 0) * 7919 + self.rank
            self._clip_pipe = data.DeviceClipPipeline.from_config(self.model, self.config.get("data", {}) or {}, seed=seed)
        return self._clip_pipe

    def prepare_input(self, cine: torch.Tensor, train: bool = False) -> torch.Tensor:
        """A batch's ``cine`` as the model takes it: a 3-channel clip moves to the device as it is; a single-channel (N,1,...) clip
        (fp32 / bf16 in [0, 1], or uint8) becomes the normalised grey clip in ONE launch, augmented in ``train`` epochs when the config's
        ``data.augmentation`` says so (the reference's train split; val, test and push clips are never augmented)."""
        if isinstance(cine, data.RawCineBatch) or (cine.dim() >= 4 and cine.shape[1] == 1):
            pipe = self.clip_pipeline()
            return pipe.normalized(cine, train and pipe.augment)
        return cine.to(self.device, non_blocking=True)

    def staged(self, loader):
        """The loader's samples, each raw batch (``data.RawCineBatch``) already uploaded: batch i + 1's copy is issued on a side stream
        before batch i is handed out, so it overlaps step i; the resize waits on the copy's event (``RawCineBatch.ready``)."""
        pending = None
        for sample in loader:
            if self.device.type == "cuda" and isinstance(sample, dict) and isinstance(sample.get("cine"), data.RawCineBatch):
                sample = dict(sample, cine=self._upload_raw(sample["cine"]))
                if pending is not None:
                    yield pending
                pending = sample
                continue
            if pending is not None:  # clip batches are handed out as they come
                yield pending
                pending = None
            yield sample
        if pending is not None:
            yield pending

    def _upload_raw(self, raw: "data.RawCineBatch") -> "data.RawCineBatch":
        if raw.device == self.device:
            return raw
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._copy_stream):
            dev = raw.to(self.device, non_blocking=True)
            dev.ready = torch.cuda.Event()
            dev.ready.record(self._copy_stream)
        dev.buffer.record_stream(main)  # allocated on the copy stream, read on the compute stream
        return dev

    # ---- Video_XProtoNet_e2e.py:36-361, minus the per-batch host work ------------------------------------------------------------
    def compute_loss(self, inp, target, logit, similarities, occurrence_map, occurrence_map_transformed=None, affine_config=None, stats=None):
        if self.fused is not None:  # ``stats``: the epoch's (confusion matrix, loss_sum), updated in the criterion's launch
            if self.Trans_occurrence.loss_weight == 0:
                trans = None
            elif occurrence_map_transformed is not None:
                trans = self.Trans_occurrence.compute_from_maps(occurrence_map, occurrence_map_transformed, affine_config)
            else:
                trans = self.Trans_occurrence.compute(inp, occurrence_map, self.model)
            return self.fused.compute(logit, similarities, occurrence_map, self.model.prototype_vectors, self.model.last_layer.weight, target,
                                      transform_term=trans, stats=stats)
        terms = [
            self.CeLoss.compute(logits=logit, target=target),
            self.Cluster.compute(similarities, target),
            self.Separation.compute(similarities, target),
            self.Orthogonality.compute(self.model.prototype_vectors),
            self.Lnorm_occurrence.compute(occurrence_map, dim=(-3, -2, -1) if occurrence_map.dim() == 6 else (-2, -1)),
        ]
        if self.Trans_occurrence.loss_weight == 0:
            terms.append(torch.zeros((), device=logit.device))
        elif occurrence_map_transformed is not None:  # eval epochs: the warped clips rode in the same forward (run_epoch)
            terms.append(self.Trans_occurrence.compute_from_maps(occurrence_map, occurrence_map_transformed, affine_config))
        else:
            terms.append(self.Trans_occurrence.compute(inp, occurrence_map, self.model))
        terms.append(self.Lnorm_fc.compute(self.model.last_layer.weight))
        return sum(terms), torch.stack([t.detach().float().reshape(()) for t in terms])

    def run_epoch(self, epoch: int, mode: str = "train") -> Dict[str, object]:
        self.model.train() if mode == "train" else self.model.eval()
        loader = self.data_loaders[mode.split("_")[0] if "_push" in mode else mode]
        K = self.num_real_classes
        cm = torch.zeros(K * K, dtype=torch.int64, device=self.device)
        loss_sum = torch.zeros(7, dtype=torch.float32, device=self.device)
        n_batches = 0
        fused_stats = {"stats": (cm, loss_sum)} if self.fused is not None else {}
        if self.world_size > 1:
            if hasattr(loader, "__len__"):  # a rank with fewer micro-batches would issue fewer collectives: the job would hang in RCCL
                n = torch.tensor([len(loader), -len(loader)], dtype=torch.int64, device=self.device)
                n = push_mod._for_collective(n)
                dist.all_reduce(n, op=dist.ReduceOp.MAX)
                if int(n[0]) != -int(n[1]):
                    raise RuntimeError(f"{mode} epoch {epoch}: the ranks' loaders hold between {-int(n[1])} and {int(n[0])} batches; every rank "
                                       "must bring the same number (shard with a DistributedSampler(drop_last=True) or equal file lists)")
            if mode != "train":
                self.sync_norm_buffers()
        # the reference's second trunk pass (loss.py:302) rides in the first one's launch list: eval epochs on running statistics, training
        # epochs with two statistics groups (model.forward_pair; PASN_NO_TRAIN_PAIR=1: two passes)
        warp_in_batch = self.Trans_occurrence.loss_weight != 0 and (mode != "train" or (hasattr(self.model, "forward_pair") and _lib.tuning_get("PASN_NO_TRAIN_PAIR") != "1"))
        write_csv = mode in ("val_push", "test") and bool(self.config.get("save_dir"))
        ev = self.evaluator(loader, keep_logits=write_csv)  # None on a CPU model: its epoch dict stays the confusion-matrix one
        metas = []
        with torch.set_grad_enabled(mode == "train"):
            for i, sample in enumerate(self.staged(loader)):
                inp = self.prepare_input(sample["cine"], train=mode == "train")
                target = sample["target_AS"].to(self.device, non_blocking=True)
                if warp_in_batch:  # the reference's second trunk pass (loss.py:302) shares the launch list of the first
                    cfg = losses.get_affine_config()
                    nb = inp.shape[0]
                    warped = losses.affine_warp(inp, cfg["angle"], cfg["scale"])
                    if hasattr(self.model, "forward_pair"):
                        (logit, similarities, occurrence_map), occ_t = self.model.forward_pair(inp, warped)
                    else:
                        logit, similarities, occurrence_map = self.model(torch.cat([inp, warped]))
                        occ_t = occurrence_map[nb:]
                        logit, similarities, occurrence_map = logit[:nb], similarities[:nb], occurrence_map[:nb]
                    loss, terms = self.compute_loss(inp, target, logit, similarities, occurrence_map, occ_t, cfg, **fused_stats)
                else:
                    logit, similarities, occurrence_map = self.model(inp)
                    loss, terms = self.compute_loss(inp, target, logit, similarities, occurrence_map, **fused_stats)
                if not fused_stats:  # (the fused criterion counted and summed in its launch)
                    pred = logit[:, :K].argmax(dim=1)  # softmax is monotone: the class of the largest real-class logit
                    cm += torch.bincount(target.clamp(0, K - 1) * K + pred, minlength=K * K)
                    loss_sum += terms
                n_batches += 1
                if ev is not None:
                    ev.update(logit, similarities, target)
                    if write_csv:
                        metas.append(metrics_mod.batch_log_meta(sample))
                if mode == "train":
                    self._norm_dirty = True  # this rank's running statistics moved on their own
                    loss.backward()  # undivided, as the reference accumulates it
                    if self.accumulator is not None:
                        self.accumulator.absorb()  # p.grad is None from here to the boundary: the accumulator holds the sums
                    if (i + 1) % self.local_accumulation == 0:
                        if self.accumulator is not None:
                            self.accumulator.materialize()
                        dp.allreduce_gradients(self.params, average=False)  # ONE exchange per optimizer step: SUM over ranks
                        self.optimizer.step()
                        self.optimizer.zero_grad(set_to_none=True)
                        if self.accumulator is not None:
                            self.accumulator.reset()
                    self.current_iteration += 1
        stats = torch.cat([cm.float(), loss_sum, torch.tensor([float(n_batches)], device=self.device)])
        evm = None
        if ev is not None:  # the evaluation counters ride in the same single all-reduce (fp64; the stats come back as the fp32 sums)
            evm, stats = ev.finish_with(self.world_size, stats)
            stats = stats.float()
        elif self.world_size > 1:  # one tiny all-reduce per epoch: every rank sees the global confusion matrix and takes the same decisions
            stats = push_mod._for_collective(stats)
            dist.all_reduce(stats)
        stats = stats.cpu()
        metrics = confusion_to_metrics(stats[: K * K].view(K, K))
        nb = max(float(stats[-1]), 1.0)
        metrics["loss_terms"] = (stats[K * K: K * K + 7] / nb).tolist()
        metrics["loss"] = float(sum(metrics["loss_terms"]))
        self.log(f"Epoch: {epoch} | {mode} | loss {metrics['loss']:.4f} | acc {metrics['accuracy']:.2%} | f1 {metrics['f1_mean']:.3f}")
        if evm is not None:
            metrics.update(evm)
            div = f"diversity {evm['diversity']}" + ("" if evm["diversity_abstain"] is None else f" | diversity_abstain {evm['diversity_abstain']}")
            self.log(f"Epoch: {epoch} | {mode} | AUC {evm['auc']:.4f} | sparsity {evm['sparsity']:.3f} | {div}")
            if write_csv:
                self.write_prediction_log(epoch, mode, metrics["f1_mean"], metas, ev)
        return metrics

    # ---- evaluation metrics: Video_XProtoNet_e2e.py:154-173, 221-233, 240-319 -------------------------------------------------------
    def evaluator(self, loader, keep_logits: bool = False) -> Optional["metrics_mod.EpochEvaluator"]:
        """The epoch's device metric state (``metrics.EpochEvaluator``), or None on a CPU model; its buffers sized ``len(loader) *
        batch_size`` when the loader knows both."""
        if self.device.type != "cuda":
            return None
        return metrics_mod.EpochEvaluator(self.model, level=0.8, keep_logits=keep_logits, abstain_class=bool(self.config.get("abstain_class")),
                                          capacity=_loader_capacity(loader))

    def write_prediction_log(self, epoch: int, mode: str, f1_mean: float, metas, ev) -> Optional[str]:
        """The reference's per-clip CSV (base.py:195-211; file name Video_XProtoNet_e2e.py:314-318).  With several ranks every rank's rows
        reach rank 0 through ``all_gather_object``, rank-major; rank 0 writes."""
        names = metrics_mod.logit_names(self.num_real_classes, bool(self.config.get("abstain_class")), self.config.get("class_labels"))
        rows = metrics_mod.prediction_rows(metas, ev.logits[: ev.rows].cpu().numpy(), names)
        if self.world_size > 1:
            every = [None] * self.world_size
            dist.all_gather_object(every, rows)
            rows = [r for part in every for r in part]
        if self.rank != 0:
            return None
        d = os.path.join(self.config["save_dir"], f"csv_{mode}")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"e{epoch:02d}_f1_{f1_mean:.0%}.csv")
        metrics_mod.write_prediction_log(path, rows)
        return path

    def evaluate(self, mode: str = "val") -> Dict[str, object]:
        """One evaluation epoch at the current epoch (the reference's ``eval_only`` run: main.py:52-53, ProtoPNet_Base.py:203-205);
        ``mode`` is ``val``, ``val_push`` or ``test`` -- a key of ``data_loaders`` (``val_push`` reads ``val``)."""
        if mode == "train":
            raise ValueError("evaluate runs an evaluation epoch: val, val_push or test")
        return self.run_epoch(self.current_epoch, mode)

    def evaluate_selective(self, mode: str = "test", level: str = "cine", coverages=(1.0, 0.9, 0.8, 0.7, 0.5), score: str = "auto",
                           bootstrap: int = 0, seed: int = 0, confidence: float = 0.95, unit: str = "cine", calibration: int = 0,
                           temperature=None, conformal=None, conformal_mondrian: bool = False, ordinal=None,
                           ordinal_net_benefit_at=()) -> Dict[str, object]:
        """Selective-prediction metrics of ``data_loaders[mode]`` (``protoasnet_amd.selective``): an eval-mode, forward-only sweep (no
        loss; the ``staged`` / ``prepare_input`` path of ``run_epoch``), the clips grouped by ``sample["filename"]`` -- with
        ``iterate_intervals`` every cardiac cycle of a cine is a row of its own -- and ``SelectiveEvaluator.finish(coverages, level)``'s
        dict: the risk-coverage curve read at ``coverages``, ``aurc``, ``error_auroc`` and, at cine level, one prediction per cine.  The
        uncertainty is ``score`` (``auto``: the abstention output when the config has ``abstain_class``, else 1 - the largest
        probability; ``CeLossAbstain``'s ``ab_logitpath`` says how the abstention logit is read).  With ``save_dir`` set and
        ``level="cine"`` it writes ``save_dir/csv_<mode>_cine/e<epoch>.csv``: ``filename, target_AS, n_clips, prob_<label>...,
        uncertainty, pred``.  ``bootstrap=B > 0`` adds ``res["ci"]``: grouped-bootstrap confidence intervals of the level's rows
        (``SelectiveEvaluator.finish``; ``protoasnet_amd.bootstrap``), each rank on its own loader's rows.  ``calibration=n_bins > 0``
        adds ``res["calibration"]`` (``protoasnet_amd.calibration``: reliability bins, ECE, MCE, class-wise ECE, Brier, NLL, confidence
        gap; with ``save_dir`` also ``save_dir/csv_<mode>_reliability/e<epoch>.csv``: ``bin, lo, hi, n, accuracy, confidence``), and
        ``temperature`` -- a float ``T > 0``, a ``calibration.TemperatureFit`` or ``"fitted"``: what ``fit_temperature`` left in
        ``self.temperature_fit`` -- rescales the class probabilities the call scores.  ``conformal`` -- a ``conformal.ConformalFit`` or
        ``"fitted"``: what ``fit_conformal`` left in ``self.conformal_fit`` -- adds ``res["conformal"]`` (prediction sets of the level's
        rows: coverage, set sizes, per-class and size-stratified coverage, mean uncertainty by set size; ``conformal_mondrian``: each
        class its own threshold) and, at cine level, ``"set@<alpha>"`` to every cine; with ``save_dir`` also
        ``save_dir/conformal_<mode>.csv``, one row per alpha.  ``ordinal`` -- ``True``, an ``ordinal.OperatingFit`` or ``"fitted"``: what
        ``fit_operating_points`` left in ``self.operating_fit`` -- adds ``res["ordinal"]`` (``protoasnet_amd.ordinal``: the agreement
        statistics that use the order of the grades, and every cut ``grade >= c`` as a screening test: AUC, average precision,
        operating points; a fit's thresholds applied unchanged under ``"fitted"``; ``ordinal_net_benefit_at``: net benefit at those
        threshold probabilities), with ``bootstrap`` also their intervals in ``res["ci"]``.

        It issues NO collectives: each rank that calls it sweeps the loader it was given and reports on those rows alone (call it on one
        rank with the full loader, or on every rank for per-shard figures; ranks need not call it together).  The model is left in the
        mode it was in; no training or epoch state is touched."""
        if isinstance(temperature, str):
            if temperature != "fitted":
                raise ValueError(f"temperature must be a number, a TemperatureFit or 'fitted', got {temperature!r}")
            if self.temperature_fit is None:
                raise ValueError("temperature='fitted' needs fit_temperature() first")
            temperature = self.temperature_fit
        if isinstance(conformal, str):
            if conformal != "fitted":
                raise ValueError(f"conformal must be a ConformalFit, 'fitted' or None, got {conformal!r}")
            if self.conformal_fit is None:
                raise ValueError("conformal='fitted' needs fit_conformal() first")
            conformal = self.conformal_fit
        if isinstance(ordinal, str):
            if ordinal != "fitted":
                raise ValueError(f"ordinal must be True, an OperatingFit, 'fitted' or None, got {ordinal!r}")
            if self.operating_fit is None:
                raise ValueError("ordinal='fitted' needs fit_operating_points() first")
            ordinal = self.operating_fit
        extra = {} if conformal is None else {"conformal": conformal, "conformal_mondrian": conformal_mondrian}  # (None: the call as it was)
        if ordinal is not None:
            extra.update(ordinal=ordinal, ordinal_net_benefit_at=ordinal_net_benefit_at)
        res = self._selective_sweep(mode, score).finish(coverages, level, bootstrap=bootstrap, seed=seed, confidence=confidence, unit=unit,
                                                        calibration=calibration, temperature=temperature, **extra)
        self.log(f"Epoch: {self.current_epoch} | {mode} | selective ({level}) | AURC {res['aurc']:.4f} | error AUROC {res['error_auroc']:.4f}")
        if level == "cine" and self.config.get("save_dir"):
            d = os.path.join(self.config["save_dir"], f"csv_{mode}_cine")
            os.makedirs(d, exist_ok=True)
            names = metrics_mod.logit_names(self.num_real_classes, False, self.config.get("class_labels"))
            from . import selective

            selective.write_cine_log(os.path.join(d, f"e{self.current_epoch:02d}.csv"), res["cines"], names)
        if calibration and self.config.get("save_dir"):
            import csv

            d = os.path.join(self.config["save_dir"], f"csv_{mode}_reliability")
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, f"e{self.current_epoch:02d}.csv"), "w", newline="") as f:
                w = csv.writer(f, lineterminator="\n")
                w.writerow(["bin", "lo", "hi", "n", "accuracy", "confidence"])
                for j, b in enumerate(res["calibration"]["bins"]):
                    w.writerow([j, repr(b["lo"]), repr(b["hi"]), b["n"], repr(b["accuracy"]), repr(b["confidence"])])
        if conformal is not None:
            c = res["conformal"]
            for lv in c["levels"]:
                self.log(f"Epoch: {self.current_epoch} | {mode} | conformal {c['kind']} ({level}) | alpha {lv['alpha']:g} | coverage "
                         f"{lv['coverage']:.4f} | mean set size {lv['mean_size']:.3f}")
            if self.config.get("save_dir"):
                import csv

                os.makedirs(self.config["save_dir"], exist_ok=True)
                with open(os.path.join(self.config["save_dir"], f"conformal_{mode}.csv"), "w", newline="") as f:
                    w = csv.writer(f, lineterminator="\n")
                    w.writerow(["alpha", "kind", "mondrian", "level", "qhat", "rows", "coverage", "mean_size", "empty", "singleton",
                                "singleton_accuracy", "min_coverage_by_size"])
                    for q, lv in zip(c["qhat"], c["levels"]):
                        w.writerow([repr(lv["alpha"]), c["kind"], int(c["mondrian"]), level, repr(q), lv["rows"]]
                                   + [repr(lv[k]) for k in ("coverage", "mean_size", "empty", "singleton", "singleton_accuracy",
                                                            "min_coverage_by_size")])
        if ordinal is not None:
            o = res["ordinal"]
            self.log(f"Epoch: {self.current_epoch} | {mode} | ordinal ({level}) | MAE {o['agreement']['mae']:.4f} | under "
                     f"{o['agreement']['under']:.4f} | over {o['agreement']['over']:.4f} | kappa(quadratic) {o['agreement']['kappa_quadratic']:.4f} | "
                     + " | ".join(f"cut>={c['cut']}: AUC {c['auc']:.4f} AP {c['ap']:.4f}" for c in o["cuts"]))
        return res

    def _selective_sweep(self, mode: str, score: str = "auto"):
        """The eval-mode, forward-only sweep of ``data_loaders[mode]`` behind ``evaluate_selective`` and ``fit_temperature``: a
        ``SelectiveEvaluator`` holding every row's logits, probabilities, label and file name.  The model is left in the mode it was in;
        no collectives, no training or epoch state."""
        from . import selective

        abstain = bool(self.config.get("abstain_class"))
        path = self.CeLoss.ab_logitpath if abstain else "joined"
        with self._forward_only(mode, head_b="selective evaluation covers") as batches:
            sel = selective.SelectiveEvaluator(self.model, abstain, score=score, ab_logitpath=path,
                                               capacity=_loader_capacity(self.data_loaders[mode]))
            for sample, x in batches:
                logit, similarities, _ = self.model(x)
                sel.update(logit, similarities, sample["target_AS"].to(self.device, non_blocking=True), list(sample["filename"]))
        return sel

    @contextlib.contextmanager
    def _forward_only(self, mode: str, head_b: Optional[str] = None, max_clips: Optional[int] = None):
        """A forward-only pass over ``data_loaders[mode]``: for the length of the ``with`` block the model is in eval mode under
        ``torch.no_grad()``, and the mode it was in comes back however the block ends.  The block receives the generator of
        ``(sample, x)``: the ``staged`` samples and their ``prepare_input`` clips, ending after ``max_clips`` clips.  ``head_b``
        ("<feature> covers"): the pass is for XProtoNet / Video_XProtoNet on the GPU and refuses anything else."""
        if head_b is not None:
            from .explain import _is_xproto

            if not _is_xproto(self.model):
                raise NotImplementedError(f"{head_b} XProtoNet and Video_XProtoNet")
            if self.device.type != "cuda":
                raise RuntimeError("protoasnet_amd models run on the GPU only; there is no CPU fallback")
        if max_clips is not None and max_clips < 1:
            raise ValueError(f"max_clips must be positive, got {max_clips}")

        def batches():
            seen = 0
            for sample in self.staged(self.data_loaders[mode]):
                x = self.prepare_input(sample["cine"])
                if max_clips is not None:
                    x = x[: max_clips - seen]
                yield sample, x
                seen += int(x.shape[0])
                if max_clips is not None and seen >= max_clips:
                    break

        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                yield batches()
        finally:
            self.model.train(was_training)

    def _rebuild_after_surgery(self) -> None:
        """Prototype surgery replaced parameters: the criterion's class mask and grouping, the optimizer and the scheduler are built again
        on the model as it stands.  BOTH start afresh: the optimizer's moments are dropped and the learning-rate schedule restarts from its
        initial state (a ReduceLROnPlateau forgets its best value and its reductions), so a prune in the middle of training resets the
        schedule; prune before training or between schedules."""
        self.get_criterion()
        self.get_optimizer()
        self.scheduler = self.get_lr_scheduler()
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]

    def prune_prototypes(self, mode: str = "val", apply: bool = False, **kw):
        """Prototype pruning on ``data_loaders[mode]`` (``protoasnet_amd.prune``): ONE forward-only sweep that keeps the similarities and
        the labels on the device, then ``prune.eliminate(sim, last layer, labels, K_real, class of each prototype, **kw)`` (``budget``,
        ``keep_per_class``, ``min_per_class``, ``max_extra_errors``, ``margin_fraction``).  Logs the trace and returns the
        ``PruneResult``.  ``apply=True`` also edits the model (``prune.apply``; the criterion, optimizer and scheduler are rebuilt) and
        returns ``(result, evaluate(mode) before, evaluate(mode) after)``.  With ``world_size > 1`` the rows of every rank are gathered
        to every rank, rank-major, and every rank computes the same result (a collective: every rank calls it)."""
        from . import prune, sweep

        sims, labels = [], []
        with self._forward_only(mode) as batches:
            for sample, x in batches:
                out = self.model(x)  # head B: (logits, similarities, maps); head A: (logits, min distances)
                sims.append((out[1] if len(out) == 3 else self.model.distance_2_similarity(out[1])).float())
                labels.append(sample["target_AS"].to(self.device, non_blocking=True).to(torch.int32))
        if not sims:
            raise ValueError("no rows: the loader is empty")
        sim, lab = torch.cat(sims), torch.cat(labels)
        if self.world_size > 1:
            n = torch.tensor([sim.shape[0]], dtype=torch.int64, device=self.device)
            most = max(int(t[0]) for (t,) in sweep.gather_ranks([n], self.device))
            pad = most - sim.shape[0]  # all_gather takes equal shapes: pad with rows that carry no label
            sim = torch.cat([sim, sim.new_zeros(pad, sim.shape[1])])
            lab = torch.cat([lab, lab.new_full((pad,), -1)])
            parts = sweep.gather_ranks([sim, lab], self.device)
            sim, lab = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        cls = prune.proto_classes(self.model).to(self.device)
        res = prune.eliminate(sim, self.model.last_layer.weight.detach().float(), lab, self.num_real_classes, cls, **kw)
        out = res.read()
        t = out["table"]
        self.log(f"Epoch: {self.current_epoch} | {mode} | prune | rows {sim.shape[0]} | wrong {t['wrong_0']} | margin sum {t['margin_sum_0']:.6f}")
        for r, step in enumerate(out["trace"]):
            self.log(f"Epoch: {self.current_epoch} | {mode} | prune round {r} | removed {step['removed']} | wrong {step['wrong']} | "
                     f"margin sum {step['margin_sum']:.6f}")
        if not apply:
            return res
        before = self.evaluate(mode)
        if out["order"]:
            prune.apply(self.model, out["order"])
            self._rebuild_after_surgery()
        return res, before, self.evaluate(mode)

    def fit_temperature(self, mode: str = "val") -> Dict[str, object]:
        """Temperature scaling fitted on the clips of ``data_loaders[mode]`` (``calibration.fit_temperature``; the sweep of
        ``evaluate_selective``): keeps the device result in ``self.temperature_fit`` -- ``evaluate_selective(temperature="fitted")``
        applies it --, logs ``T`` and the NLL before and after, and returns ``{temperature, beta, nll_before, nll_after, status}``.  No
        collectives; the model is left in the mode it was in; no training or epoch state is touched."""
        from . import calibration

        ev = self._selective_sweep(mode).ev
        if ev.rows == 0:
            raise ValueError("no rows: the loader is empty")
        self.temperature_fit = calibration.fit_temperature(ev.logits[: ev.rows], ev.labels[: ev.rows], ev.K_real)
        res = self.temperature_fit.read()
        self.log(f"Epoch: {self.current_epoch} | {mode} | temperature {res['temperature']:.4f} ({res['status']}) | "
                 f"NLL {res['nll_before']:.4f} -> {res['nll_after']:.4f}")
        return res

    def fit_conformal(self, mode: str = "val", alphas=(0.1,), kind: str = "aps", level: str = "cine", temperature=None,
                      randomized: bool = True, seed: int = 0, lam: float = 0.0, k_reg: int = 1, score: str = "auto") -> Dict[str, object]:
        """Conformal thresholds calibrated on ``data_loaders[mode]`` (``conformal.calibrate``; the forward-only sweep of
        ``evaluate_selective``): keeps the device result in ``self.conformal_fit`` -- ``evaluate_selective(conformal="fitted")`` applies
        it --, logs the thresholds and returns ``ConformalFit.read()``.  ``level="cine"`` (the default) calibrates on one row per
        cine, ``p_conf.float()`` with the cine's label, exactly the rows ``evaluate_selective(level="cine")`` scores: the clips of one
        cine are not exchangeable with the clips of another patient's, so a clip-level guarantee on correlated clips is not a
        guarantee.  ``temperature`` as in ``evaluate_selective`` (apply the same one there).  No collectives; the model is left in the
        mode it was in; no training or epoch state is touched."""
        from . import calibration, conformal, selective

        if level not in ("clip", "cine"):
            raise ValueError(f"level must be 'clip' or 'cine', got {level!r}")
        al = conformal.check_alphas(alphas)
        conformal.check_settings(kind, randomized, seed, lam, k_reg)
        if isinstance(temperature, str):
            if temperature != "fitted":
                raise ValueError(f"temperature must be a number, a TemperatureFit or 'fitted', got {temperature!r}")
            if self.temperature_fit is None:
                raise ValueError("temperature='fitted' needs fit_temperature() first")
            temperature = self.temperature_fit
        if temperature is not None:
            calibration._check_temperature(temperature)
        sel = self._selective_sweep(mode, score)
        ev = sel.ev
        if ev.rows == 0:
            raise ValueError("no rows: the loader is empty")
        logits, probs, labels = ev.logits[: ev.rows], ev.probs[: ev.rows], ev.labels[: ev.rows]
        if temperature is not None:
            probs = calibration.scaled_probs(logits, ev.K_real, temperature)
        if level == "cine":
            if temperature is not None and selective.score_mode(sel.abstain, sel.score, sel.ab_logitpath) == selective.MAXPROB:
                u = 1.0 - probs.amax(dim=1)  # what scaled_probs(with_u=True) returns, bitwise
            else:
                u = selective.uncertainty(logits, sel.abstain, sel.score, sel.ab_logitpath)
            gp = selective.group_predictions(probs, u, labels, selective.build_groups(sel.keys)[:2])
            probs, labels = gp.p_conf.float(), gp.labels
        self.conformal_fit = conformal.calibrate(probs, labels, al, kind, randomized, seed, lam, k_reg)
        res = self.conformal_fit.read()
        self.log(f"Epoch: {self.current_epoch} | {mode} | conformal {kind} ({level}) | n {res['n']} | "
                 + " | ".join(f"alpha {a:g}: qhat {q:.6f}" for a, q in zip(res["alphas"], res["qhat"])))
        return res

    def fit_operating_points(self, mode: str = "val", level: str = "cine", specificities=(0.9,), sensitivities=(0.9,), temperature=None,
                             score: str = "auto") -> Dict[str, object]:
        """Screening thresholds fitted on ``data_loaders[mode]`` (``ordinal.fit_operating_points``; the forward-only sweep of
        ``evaluate_selective``): per cut ``grade >= c`` the threshold that reaches each stated specificity and sensitivity, and
        Youden's.  Keeps the device result in ``self.operating_fit`` -- ``evaluate_selective(ordinal="fitted")`` applies it unchanged
        --, logs the thresholds and returns ``OperatingFit.read()``.  ``level="cine"`` (the default) fits on one row per cine,
        ``p_conf.float()`` with the cine's label, exactly the rows ``evaluate_selective(level="cine")`` scores.  ``temperature`` as in
        ``evaluate_selective`` (apply the same one there).  No collectives; the model is left in the mode it was in; no training or
        epoch state is touched."""
        from . import calibration, ordinal, selective

        if level not in ("clip", "cine"):
            raise ValueError(f"level must be 'clip' or 'cine', got {level!r}")
        spec, sens = ordinal.check_targets(specificities, "specificities"), ordinal.check_targets(sensitivities, "sensitivities")
        if isinstance(temperature, str):
            if temperature != "fitted":
                raise ValueError(f"temperature must be a number, a TemperatureFit or 'fitted', got {temperature!r}")
            if self.temperature_fit is None:
                raise ValueError("temperature='fitted' needs fit_temperature() first")
            temperature = self.temperature_fit
        if temperature is not None:
            calibration._check_temperature(temperature)
        sel = self._selective_sweep(mode, score)
        ev = sel.ev
        if ev.rows == 0:
            raise ValueError("no rows: the loader is empty")
        logits, probs, labels = ev.logits[: ev.rows], ev.probs[: ev.rows], ev.labels[: ev.rows]
        # the rows SelectiveEvaluator.finish scores, by the calls it makes
        if temperature is None:
            u = selective.uncertainty(logits, sel.abstain, sel.score, sel.ab_logitpath)
        elif selective.score_mode(sel.abstain, sel.score, sel.ab_logitpath) == selective.MAXPROB:
            probs, u = calibration.scaled_probs(logits, ev.K_real, temperature, with_u=True)
        else:
            probs = calibration.scaled_probs(logits, ev.K_real, temperature)
            u = selective.uncertainty(logits, sel.abstain, sel.score, sel.ab_logitpath)
        if level == "cine":
            gp = selective.group_predictions(probs, u, labels, selective.build_groups(sel.keys)[:2])
            probs, labels = gp.p_conf.float(), gp.labels
        self.operating_fit = ordinal.fit_operating_points(probs, labels, spec, sens)
        res = self.operating_fit.read()
        self.log(f"Epoch: {self.current_epoch} | {mode} | operating points ({level}) | "
                 + " | ".join(f"cut>={c + 1}: " + ", ".join(f"{k}{'' if t is None else f'={t:g}'} {th:.6f}" for k, t, th in zip(res["kinds"], res["targets"], row))
                              for c, row in enumerate(res["thresholds"])))
        return res

    def evaluate_faithfulness(self, mode: str = "val", steps: int = 10, select: int = 1, max_clips: Optional[int] = None,
                              max_batch: int = 64, seed: int = 0, kinds: Sequence[str] = ("model", "random"),
                              rise: Optional[Dict[str, object]] = None) -> Dict[str, object]:
        """Are the occurrence maps faithful on ``data_loaders[mode]``?  (``protoasnet_amd.faithfulness``)  An eval-mode sweep: per batch
        (through ``prepare_input``) the deletion and insertion curves of the ``select`` best prototypes of the predicted class under the
        model's maps and under a random map, summed in fp64 on the device and read once.  Returns
        ``FaithfulnessAccumulator.result()``: the mean curves, the mean areas, the random control's and their differences.  With "rise"
        among ``kinds`` the same curves are swept under RISE maps (``saliency.rise`` with the arguments ``rise``), the black-box baseline:
        ``res["rise"]`` and ``res["difference_rise"]``, and one more log line.  ``max_clips`` ends the sweep after that many clips.  Each rank sweeps its own loader; no collectives, no training or epoch state; the model is
        left in the mode it was in."""
        from . import faithfulness

        with self._forward_only(mode, head_b="faithfulness curves cover", max_clips=max_clips) as batches:
            acc = faithfulness.FaithfulnessAccumulator(self.model, select=select, steps=steps, max_batch=max_batch,
                                                       abstain_class=bool(self.config.get("abstain_class")), seed=seed, kinds=kinds, rise=rise)
            for _, x in batches:
                acc.update(x)
        res = acc.result()
        for kind in acc.kinds[1:] or ("model",):
            versus = {m: f" vs {kind} {float(res[kind][m]['auc_prob'].mean()):.4f}" if kind != "model" else "" for m in faithfulness.MODES}
            self.log(f"Epoch: {self.current_epoch} | {mode} | faithfulness ({res['clips']} clips) | deletion AUC (prob) "
                     f"{float(res['deletion']['auc_prob'].mean()):.4f}{versus['deletion']} | "
                     f"insertion AUC (prob) {float(res['insertion']['auc_prob'].mean()):.4f}{versus['insertion']}")
        return res

    def evaluate_robustness(self, mode: str = "val", corruptions: Optional[Sequence[str]] = None, severities: Sequence[int] = (1, 3, 5),
                            select: int = 1, top_fraction: float = 0.1, max_clips: Optional[int] = None, seed: int = 0) -> Dict[str, object]:
        """Do the prediction and its explanation survive echo-style corruptions of ``data_loaders[mode]``?
        (``protoasnet_amd.robustness``)  An eval-mode sweep: per batch (through ``prepare_input``) one clean ``push_forward`` and one
        corrupted one per (corruption, severity) cell (``corruptions=None``: all of ``robustness.CORRUPTIONS``), compared on the device
        and summed in fp64 there, read once.  Returns ``RobustnessAccumulator.result()``: per cell the accuracy clean and corrupted, the
        flip rate, the mean total variation and probability drop, the top-``select`` prototype overlap and per prototype rank the mean
        similarity change, map correlation, top-set IoU and argmax shift.  ``max_clips`` ends the sweep after that many clips.  Each
        rank sweeps its own loader; no collectives, no training or epoch state; the model is left in the mode it was in."""
        from . import robustness

        with self._forward_only(mode, head_b="robustness evaluation covers", max_clips=max_clips) as batches:
            acc = robustness.RobustnessAccumulator(self.model, corruptions=corruptions, severities=severities, select=select,
                                                   top_fraction=top_fraction, seed=seed, abstain_class=bool(self.config.get("abstain_class")))
            for sample, x in batches:
                acc.update(x, torch.as_tensor(sample["target_AS"])[: int(x.shape[0])])
        res = acc.result()
        for name, by_severity in res["cells"].items():
            for sev, c in by_severity.items():
                self.log(f"Epoch: {self.current_epoch} | {mode} | robustness ({res['clips']} clips) | {name} severity {sev} | accuracy "
                         f"{c['acc_clean']:.4f} -> {c['acc_corrupted']:.4f} | flip rate {c['flip_rate']:.4f} | tv {c['tv']:.4f} | "
                         f"prob drop {c['prob_drop']:.4f} | top-{select} overlap {c['overlap']:.4f} | map corr {float(c['corr'][0]):.4f} | "
                         f"IoU {float(c['iou'][0]):.4f} | shift {float(c['shift'][0]):.4f}")
        return res

    # ---- out-of-distribution detection (protoasnet_amd.ood) ------------------------------------------------------------------------------
    def _ood_sweep(self, mode: str, det, max_clips: Optional[int] = None, fit: bool = False, cells=(), seed: int = 0) -> Dict[str, object]:
        """One forward-only ``push_forward`` sweep of ``data_loaders[mode]``: the rows' embedding, similarities, logits, labels and file
        names (``fit``: the detector's bank and moments are filled on the way), and for every (corruption, severity) of ``cells`` the
        same three of the corrupted copies (batch ``b`` corrupts with ``seed + b``).  Device tensors, concatenated; no read."""
        from . import robustness

        names = ("emb", "sim", "logits")
        parts = {n: [] for n in names}
        shifted = {c: {n: [] for n in names} for c in cells}
        labels, keys = [], []

        def outputs(x):
            feats, proto_dist, _, logits = self.model.push_forward(x)
            return det.embed(feats, proto_dist), (1 - proto_dist).float().contiguous(), logits.float().contiguous()

        with self._forward_only(mode, head_b="out-of-distribution detection covers", max_clips=max_clips) as batches:
            for b, (sample, x) in enumerate(batches):
                n = int(x.shape[0])
                out = outputs(x)
                y = torch.as_tensor(sample["target_AS"])[:n].to(self.device, non_blocking=True)
                if fit:
                    det.fit_update(out[0], y)
                for name, t in zip(names, out):
                    parts[name].append(t)
                labels.append(y)
                keys += list(sample["filename"])[:n]
                for c in cells:
                    for name, t in zip(names, outputs(robustness.corrupt(x, c[0], c[1], seed + b))):
                        shifted[c][name].append(t)
        if not labels:
            raise ValueError("no rows: the loader is empty")
        rows = {n: torch.cat(v) for n, v in parts.items()}
        rows.update(labels=torch.cat(labels), keys=keys, shifted={c: {n: torch.cat(v) for n, v in d.items()} for c, d in shifted.items()})
        return rows

    def _ood_level_rows(self, det, rows: Dict[str, object], level: str, groups=None, self_base: int = -1):
        """``(scores, correct)`` of swept rows at ``level``: per detector the (M,) fp32 scores and whether the model's prediction is the
        label; at cine level one row per cine -- the fp64 mean of its clips' scores in row order (``selective.group_predictions`` with
        the score in the place of ``u``, ``u_mean`` cast once to fp32) and the cine's ``p_conf`` prediction."""
        from . import calibration, selective

        scores = det.scores(rows["emb"], rows["sim"], rows["logits"], self_base=self_base)
        probs = calibration.scaled_probs(rows["logits"], self.num_real_classes, 1.0)
        labels = rows["labels"].to(torch.int32)
        if level == "clip":
            return scores, (selective.first_largest(probs) == labels).to(torch.int32)
        u = selective.uncertainty(rows["logits"], bool(self.config.get("abstain_class")))
        gp = selective.group_predictions(probs, u, labels, groups, check=False)
        correct = (selective.first_largest(gp.p_conf.float()) == gp.labels).to(torch.int32)
        return {d: selective.group_predictions(probs, s, labels, groups, check=False).u_mean.float() for d, s in scores.items()}, correct

    def fit_ood(self, bank: str = "train", calibrate: str = "val", level: str = "cine", tprs=(0.95,), max_bank: Optional[int] = None,
                **detector_kw) -> Dict[str, object]:
        """Fits the out-of-distribution detectors (``protoasnet_amd.ood.OODDetector(**detector_kw)``: ``detectors``, ``embedding``, ``k``,
        ``normalize``, ``shrink``) and calibrates their thresholds.  One forward-only ``push_forward`` sweep of ``data_loaders[bank]``
        (its first ``max_bank`` clips) fills the kNN bank and the Mahalanobis moments; one sweep of ``data_loaders[calibrate]`` gives
        the in-distribution scores whose ``ceil((n + 1) tpr)``-th smallest is the threshold of level ``tpr``: an exchangeable
        in-distribution row is then flagged with probability at most ``1 - tpr``.  ``level="cine"`` (the default) calibrates on one row
        per cine, the fp64 mean of its clips' scores -- the clips of one cine are not exchangeable with another patient's, so a
        clip-level guarantee on correlated clips is not a guarantee (``fit_conformal``); ``level="clip"`` calibrates on the rows.  With
        ``bank == calibrate`` the rows of the one sweep are scored against the bank they are in, and the kNN scan leaves every row out
        of its own neighbours; the Mahalanobis fit is NOT leave-one-out (its means and covariance include the row), so its thresholds
        are optimistic then.  Keeps the fit, with its detector, level and thresholds, in ``self.ood_fit`` -- ``evaluate_ood`` applies it
        --, logs the thresholds and returns ``{level, bank_rows, rows, tprs, detectors: {name: {tau, n, nan_rows}}}``.  Without an
        abstention class the default detectors leave ``"abstain"`` out.  No collectives; the model is left in the mode it was in; no
        training or epoch state is touched."""
        from . import ood, selective

        if level not in ("clip", "cine"):
            raise ValueError(f"level must be 'clip' or 'cine', got {level!r}")
        tp = ood.check_tprs(tprs)
        ood.OODDetector(**detector_kw)  # the detector's own checks, before any sweep
        abstain = bool(self.config.get("abstain_class"))
        kw = dict(detector_kw)
        kw.setdefault("abstain_class", abstain)
        kw.setdefault("num_classes", self.num_real_classes)
        if not abstain:
            kw.setdefault("detectors", tuple(d for d in ood.DETECTORS if d != "abstain"))
        det = ood.OODDetector(**kw)
        rows = self._ood_sweep(bank, det, max_clips=max_bank, fit=True)
        fit = det.fit_finish()
        same = bank == calibrate
        cal = rows if same else self._ood_sweep(calibrate, det)
        groups = selective.build_groups(cal["keys"])[:2] if level == "cine" else None
        scores, _ = self._ood_level_rows(det, cal, level, groups, self_base=0 if same else -1)
        th = det.calibrate(scores, tp)
        fit.detector, fit.level = det, level
        self.ood_fit = fit
        res = th.read()
        res.update(level=level, bank_rows=int(rows["emb"].shape[0]), rows=int(next(iter(scores.values())).shape[0]))
        for d, r in res["detectors"].items():
            self.log(f"Epoch: {self.current_epoch} | {calibrate} | ood {d} ({level}) | n {r['n']} | "
                     + " | ".join(f"tpr {t:g}: tau {q:.6f}" for t, q in zip(res["tprs"], r["tau"])))
        return res

    def evaluate_ood(self, mode: str = "test", shift="corruptions", corruptions: Optional[Sequence[str]] = None,
                     severities: Sequence[int] = (1, 3, 5), level: str = "cine", max_clips: Optional[int] = None,
                     seed: int = 0) -> Dict[str, object]:
        """Do the fitted detectors (``fit_ood``) tell shifted clips from ``data_loaders[mode]``'s?  In-distribution scores come from the
        split; shifted scores from the SAME clips through ``robustness.corrupt``, per (corruption, severity) cell (``corruptions=None``:
        all of ``robustness.CORRUPTIONS``), or, when ``shift`` names a loader, from ``data_loaders[shift]`` (one cell, severity 0).
        Returns ``{level, rows, tprs, detectors: {name: {tau, id_flagged_rate, accuracy_kept, accuracy_flagged (one per tpr),
        nan_rows, cells: {cell: {severity: {auroc, flagged_rate (one per tpr), rows}}}}}}``: the rate at the FITTED threshold and the
        AUROC (shifted rows positive), not the literature's FPR@95, whose threshold is chosen on the test rows themselves.  ``level``
        must be the fit's (a cine's mean score and a clip's do not share a threshold).  Tallies stay on the device until the ONE read
        at the end.  Each rank sweeps its own loaders; no collectives, no training or epoch state; the model is left in the mode it
        was in."""
        from . import ood, robustness, selective

        if self.ood_fit is None or self.ood_fit.thresholds is None:
            raise ValueError("evaluate_ood needs fit_ood() first")
        if level not in ("clip", "cine"):
            raise ValueError(f"level must be 'clip' or 'cine', got {level!r}")
        det, th = self.ood_fit.detector, self.ood_fit.thresholds
        if level != self.ood_fit.level:
            raise ValueError(f"the thresholds were calibrated at level {self.ood_fit.level!r} (fit_ood), not {level!r}")
        if shift == "corruptions":
            names = tuple(robustness.CORRUPTIONS) if corruptions is None else tuple(corruptions)
            cells = [(n, int(s)) for n in names for s in severities]
            for n, s in cells:
                robustness.describe(n, s, (1, 1, 2, 2, 2))  # unknown names and severities fail here, not in the middle of a sweep
            if not cells:
                raise ValueError("at least one corruption and one severity")
        elif isinstance(shift, str) and shift in self.data_loaders:
            cells = []
        else:
            raise ValueError(f"shift must be 'corruptions' or a key of data_loaders, got {shift!r}")
        rows = self._ood_sweep(mode, det, max_clips=max_clips, cells=tuple(cells), seed=seed)
        groups = selective.build_groups(rows["keys"])[:2] if level == "cine" else None
        s_id, correct = self._ood_level_rows(det, rows, level, groups)
        shifted = []
        for c in cells:
            shifted.append((c, self._ood_level_rows(det, dict(rows, **rows["shifted"][c]), level, groups)[0]))
        if not cells:
            other = self._ood_sweep(shift, det, max_clips=max_clips)
            g2 = selective.build_groups(other["keys"])[:2] if level == "cine" else None
            shifted.append(((shift, 0), self._ood_level_rows(det, other, level, g2)[0]))
        n_id = int(correct.shape[0])
        packed, counts = [torch.cat([th.tau[d].double() for d in s_id])], []
        for c, s_c in shifted:
            n_c = int(next(iter(s_c.values())).shape[0])
            kind = torch.cat([torch.zeros(n_id, dtype=torch.int32, device=self.device), torch.ones(n_c, dtype=torch.int32, device=self.device)])
            ok = torch.cat([correct, torch.zeros(n_c, dtype=torch.int32, device=self.device)])
            packed.append(ood.evaluate({d: torch.cat([s_id[d], s_c[d]]) for d in s_id}, kind, th, ok).packed())
            counts.append(n_c)
        host = torch.cat(packed).cpu().numpy()  # the one read
        dets, A = list(s_id), len(th.tprs)
        res = {"level": level, "rows": n_id, "tprs": list(th.tprs), "detectors": {}}
        per = len(dets) * (A * ood.TALLY_WORDS + 1)
        evs = [ood.OODEvaluation.unpack(host[len(dets) * A + j * per: len(dets) * A + (j + 1) * per], dets, th.tprs) for j in range(len(shifted))]
        for i, d in enumerate(dets):
            first = evs[0][d]["levels"]
            out = {"tau": host[i * A: (i + 1) * A].tolist(), "id_flagged_rate": [lv["id_flagged_rate"] for lv in first],
                   "accuracy_kept": [lv["accuracy_kept"] for lv in first], "accuracy_flagged": [lv["accuracy_flagged"] for lv in first],
                   "nan_rows": first[0]["nan_rows"], "cells": {}}
            for (c, _), ev, n_c in zip(shifted, evs, counts):
                out["cells"].setdefault(c[0], {})[c[1]] = {"auroc": ev[d]["auroc"], "rows": n_c,
                                                          "flagged_rate": [lv["ood_flagged_rate"] for lv in ev[d]["levels"]]}
                self.log(f"Epoch: {self.current_epoch} | {mode} | ood {d} ({level}) | {c[0]} severity {c[1]} | AUROC {ev[d]['auroc']:.4f} | "
                         f"flagged {ev[d]['levels'][0]['ood_flagged_rate']:.4f} (in-distribution {first[0]['id_flagged_rate']:.4f})")
            res["detectors"][d] = out
        return res

    def push(self, replace_prototypes: bool = True):
        abstain = bool(self.config.get("abstain_class"))
        self.sync_norm_buffers()  # every shard of the sweep must see the same eval-mode statistics
        return push_mod.push_prototypes(
            self.data_loaders["train_push"], self.model, class_specific=True, abstain_class=abstain,
            root_dir_for_saving_prototypes=self.config.get("save_dir") and os.path.join(self.config["save_dir"], "img"),
            epoch_number=self.current_epoch, log=self.log, replace_prototypes=replace_prototypes, rank=self.rank, world_size=self.world_size,
            preprocess_input_function=self.prepare_input)

    # ---- global explanations: XProtoNet_Base.py:613-667 and the explain_global stub ----------------------------------------------------
    def _sim_scores_paths(self, epoch: int, mode: str):
        d = os.path.join(self.config["save_dir"], "ranking_prototypes")
        return os.path.join(d, f"sim_scores_{mode}_epoch{epoch}.pth"), os.path.join(d, f"targets_{mode}.pth")

    def get_sim_scores(self, mode: str = "train") -> None:
        """The reference's ``get_sim_scores``: the (N, P) similarities of ``data_loaders[mode]`` and its targets, saved as CPU float32
        tensors under ``save_dir/ranking_prototypes/`` with the reference's file names.  Batches are read by ``cine`` / ``target_AS``
        and go through ``prepare_input``.  Several ranks: every rank sweeps its loader, rank 0 writes the rank-major concatenation.
        The model is left in the mode it was in; no training state is touched."""
        epoch = self.current_epoch
        self.log(f"Epoch: {epoch} generating the sim scores for dataset:{mode}")
        if self.world_size > 1:
            self.sync_norm_buffers()
        sims, targets = [], []
        with self._forward_only(mode) as batches:
            for sample, x in batches:
                _, similarities, _ = self.model(x)
                sims.append(similarities.float())
                targets.append(torch.as_tensor(sample["target_AS"]).detach().cpu().to(torch.float32))
        P = self.model.num_prototypes
        sim_scores = torch.cat(sims).cpu() if sims else torch.empty((0, P), dtype=torch.float32)
        y_true_all = torch.cat(targets) if targets else torch.empty((0,), dtype=torch.float32)
        if self.world_size > 1:
            every = [None] * self.world_size
            dist.all_gather_object(every, (sim_scores, y_true_all))
            sim_scores, y_true_all = torch.cat([e[0] for e in every]), torch.cat([e[1] for e in every])
        if self.rank != 0:
            return
        sim_path, target_path = self._sim_scores_paths(epoch, mode)
        os.makedirs(os.path.dirname(sim_path), exist_ok=True)
        torch.save(sim_scores, sim_path)
        torch.save(y_true_all, target_path)

    def load_sim_scores(self, epoch: int, mode: str):
        sim_path, target_path = self._sim_scores_paths(epoch, mode)
        return torch.load(sim_path), torch.load(target_path)

    def explain_global(self, mode: str = "val", k: int = 10):
        """What the reference's ``explain_global`` stub leaves open: ``global_explain.nearest_clips`` over ``data_loaders[mode]``; rank 0
        writes ``save_dir/global/{mode}/epoch-{epoch}/nearest_info.pickle`` (numpy arrays under the ``GlobalExplanation`` field names).
        Several ranks: the sweep shards the loader itself, as the push does, so ``mode`` must name a FULL sequential loader."""
        import pickle

        from . import global_explain

        if self.world_size > 1:
            self.sync_norm_buffers()
        result = global_explain.nearest_clips(
            self.data_loaders[mode], self.model, k=k, class_specific=False, abstain_class=bool(self.config.get("abstain_class")),
            preprocess_input_function=self.prepare_input, rank=self.rank, world_size=self.world_size, log=self.log)
        if self.rank == 0 and self.config.get("save_dir"):
            d = os.path.join(self.config["save_dir"], "global", mode, f"epoch-{self.current_epoch}")
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, "nearest_info.pickle")
            with open(path, "wb") as handle:
                pickle.dump(result.to_numpy(), handle, protocol=pickle.HIGHEST_PROTOCOL)
            self.log(f"data successfully saved in {path}")
        return result

    def save_model_w_condition(self, model_name: str, metric_dict: dict, threshold: float) -> None:
        name, metric = next(iter(metric_dict.items()))
        if metric > threshold and self.rank == 0 and self.train_config.get("save", True):
            os.makedirs(self.config["save_dir"], exist_ok=True)
            torch.save(self.get_state(), os.path.join(self.config["save_dir"], f"{model_name}_{name}-{metric:.4f}.pth"))

    def train(self) -> Dict[str, list]:
        tc = self.train_config
        history = {"train": [], "val": [], "val_push": []}
        for epoch in range(self.current_epoch, tc["num_train_epochs"]):
            self.current_epoch = epoch
            history["train"].append(self.run_epoch(epoch, mode="train"))
            val = self.run_epoch(epoch, mode="val")
            history["val"].append(val)
            if tc["lr_schedule"]["name"] == "StepLR":
                self.scheduler.step()
            else:
                self.scheduler.step(val["f1_mean"])
            if epoch == tc["num_warm_epochs"]:
                self.push(replace_prototypes=False)
            if epoch >= tc["push_start"] and epoch % tc["push_rate"] == 0:
                self.push()
                vp = self.run_epoch(epoch, mode="val_push")
                history["val_push"].append(vp)
                self.save_model_w_condition(model_name=f"{epoch}push", metric_dict={"f1": vp["f1_mean"]}, threshold=0.65)
                is_best = vp["f1_mean"] > self.best_metric
                if is_best:
                    self.best_metric = vp["f1_mean"]
                    self.log(f"achieved best model with mean_f1 of {vp['f1_mean']}")
                self.save_checkpoint(is_best=is_best)
            self.save_checkpoint(is_best=False)
        return history
