"""Epoch loop with the reference's call signatures (src/yolo/training/trainer.py:23,133,220).

One train step = zero_grad -> model(images) -> criterion -> backward -> clip_grad_norm_(10) -> step.
On a ROCm device every piece of that runs on the HIP kernels: the model and the loss as single
autograd nodes, and -- when the optimizer is ``yolo.optim.Adam`` built with ``max_grad_norm=10`` --
clipping + Adam as one fused pass (the separate clip call is then skipped).  With
``torch.distributed`` initialised, gradients are averaged over the ranks before the update
(yolo.parallel; the reference is single-device).
"""

from __future__ import annotations

import time

import torch
import torch.distributed as dist

from ..metrics import evaluate_model
from ..parallel import make_grad_reducer
from .checkpoints import save_best_map_model, save_best_model, save_checkpoint

_PARTS = ("total", "coord", "conf_obj", "conf_noobj", "class")
_CLIP = 10.0


class LRWarmup:
    """Linear learning-rate warm-up over the first ``steps`` optimizer steps of a run, for both epoch loops (this one and ``classify``): step k
    (from 0) runs with every group's learning rate multiplied by (k + 1) / steps while k < steps, on top of whatever the scheduler set.  The
    scheduled rates are put back as soon as the step is enqueued, so the scheduler (MultiStepLR multiplies the rate it finds) and the
    checkpoints never see a warmed one.  ``done``: optimizer steps the run has behind it (a resume at epoch e: e x steps per epoch)."""

    def __init__(self, optimizer, steps: int, done: int = 0):
        self.optimizer, self.steps, self.k = optimizer, int(steps), int(done)

    def step(self):
        """``optimizer.step()``, warmed while the warm-up lasts"""
        k, self.k = self.k, self.k + 1
        if k >= self.steps:
            return self.optimizer.step()
        scheduled = [g["lr"] for g in self.optimizer.param_groups]
        for g in self.optimizer.param_groups:
            g["lr"] = g["lr"] * (k + 1) / self.steps
        try:
            return self.optimizer.step()
        finally:
            for g, lr in zip(self.optimizer.param_groups, scheduled):
                g["lr"] = lr


def make_warmup(optimizer, warmup_steps: int, start_epoch: int, train_loader, accum_steps: int = 1):
    """the ``LRWarmup`` of a run that begins at ``start_epoch`` (None when ``warmup_steps`` is 0: no learning rate is ever written)"""
    if not warmup_steps:
        return None
    return LRWarmup(optimizer, warmup_steps, done=(start_epoch - 1) * (len(train_loader) // max(int(accum_steps), 1)))


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, writer=None, scaler=None, ema=None, accum_steps: int = 1,
                warmup=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean of each loss component.  ``ema``: a ``yolo.optim.ModelEMA`` of ``model``, moved after every
    optimizer step (on a device it is enqueued like the step itself, nothing waits).

    ``accum_steps`` = K > 1: gradient accumulation (``yolo.optim.GradAccumulator``) -- K batches per optimizer step, EMA update and all-reduce;
    the effective batch is K times the loader's (times the ranks).  A last group of fewer than K batches is dropped, not applied (the spirit of
    ``drop_last=True``), and its losses do not enter the returned means.

    ``scaler`` (the reference's fp16 autocast + GradScaler branch, trainer.py:69-83) is accepted and not used: on a ROCm
    device the engine already computes in bf16 with fp32 accumulation and fp32 master weights, which needs no loss scaling;
    on the CPU the stock fp32 path runs."""
    model.train()
    sums = dict.fromkeys(_PARTS, 0.0)
    n = 0
    fused_clip = getattr(optimizer, "max_grad_norm", None) is not None
    # data parallel: the reducer is chosen once per model (it may attach a gradient arena to the model's plan) -- on a GPU
    # the all-reduce overlaps the backward pass, the path bench.py measures
    allreduce = None
    if dist.is_available() and dist.is_initialized():
        allreduce = getattr(model, "_yolo_grad_reducer", None)
        if allreduce is None:
            allreduce = make_grad_reducer(model, device)
            model._yolo_grad_reducer = allreduce
    if accum_steps > 1:
        return _train_epoch_accum(model, dataloader, criterion, optimizer, device, epoch, writer, ema, int(accum_steps), allreduce, fused_clip, warmup)
    t0 = time.time()
    for batch_idx, (images, targets) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)
        loss, parts = criterion(model(images), targets)
        loss.backward()
        if allreduce is not None:
            allreduce.all_reduce_mean()
        if not fused_clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=_CLIP)
        if hasattr(optimizer, "skip_if"):
            # yolo.optim.Adam: a step whose targets the loss kernel flagged as invalid updates nothing (the error itself surfaces at
            # the read of `parts` below; the reference raises inside the loss, before any update)
            optimizer.skip_if = getattr(parts, "device_flag", None)
        if warmup is None:
            optimizer.step()
        else:
            warmup.step()
        if ema is not None:
            ema.update(model)
        for k in _PARTS:
            sums[k] += parts[k]
        n += 1
        if (batch_idx + 1) % 10 == 0:
            print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{len(dataloader)}] Loss: {parts['total']:.4f} "
                  f"(coord: {parts['coord']:.4f}, conf_obj: {parts['conf_obj']:.4f}, conf_noobj: {parts['conf_noobj']:.4f}, "
                  f"class: {parts['class']:.4f}) Time: {time.time() - t0:.2f}s")
            if writer is not None:
                step = (epoch - 1) * len(dataloader) + batch_idx
                for k in _PARTS:
                    writer.add_scalar(f"batch/{k}_loss", parts[k], step)
            t0 = time.time()
    return {k: v / max(n, 1) for k, v in sums.items()}


def _train_epoch_accum(model, dataloader, criterion, optimizer, device, epoch, writer, ema, K, allreduce, fused_clip, warmup=None) -> dict[str, float]:
    """train_epoch's loop with K batches per optimizer step.  The accumulator is kept on the model like the reducer it mutes (its buffers are as
    large as the gradients); it starts every epoch at the head of a group."""
    from ..optim import GradAccumulator
    accum = getattr(model, "_yolo_grad_accumulator", None)
    if accum is None or accum.steps != K or accum.reducer is not allreduce:
        accum = model._yolo_grad_accumulator = GradAccumulator(model, K, allreduce)
    accum.micro = 0
    sums = dict.fromkeys(_PARTS, 0.0)
    n = 0
    group = []                      # the loss parts of the open group: they count once its step is applied
    t0 = time.time()
    for batch_idx, (images, targets) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)        # the accumulator holds the sum (and with an arena the views are re-assigned anyway)
        accum.before_backward()
        loss, parts = criterion(model(images), targets)
        loss.backward()
        group.append(parts)
        if accum.after_backward(getattr(parts, "device_flag", None)):
            if not fused_clip:
                torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=_CLIP)
            if hasattr(optimizer, "skip_if"):
                optimizer.skip_if = accum.skip_if    # one flagged batch cancels the group's step (and, through last_skip, the EMA's)
            if warmup is None:
                optimizer.step()
            else:
                warmup.step()
            if ema is not None:
                ema.update(model)
            for done in group:
                for k in _PARTS:
                    sums[k] += done[k]
                n += 1
            group = []
        if (batch_idx + 1) % 10 == 0:
            print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{len(dataloader)}] Loss: {parts['total']:.4f} "
                  f"(coord: {parts['coord']:.4f}, conf_obj: {parts['conf_obj']:.4f}, conf_noobj: {parts['conf_noobj']:.4f}, "
                  f"class: {parts['class']:.4f}) Time: {time.time() - t0:.2f}s")
            if writer is not None:
                step = (epoch - 1) * len(dataloader) + batch_idx
                for k in _PARTS:
                    writer.add_scalar(f"batch/{k}_loss", parts[k], step)
            t0 = time.time()
    for r in getattr(accum, "_overlapped", ()):
        r.muted = False              # a dropped incomplete group leaves the reducer as it was found
    return {k: v / max(n, 1) for k, v in sums.items()}


def validate(model, dataloader, criterion, device, compute_map: bool = False, num_classes: int = 20) -> dict[str, float]:
    """Mean loss components over ``dataloader`` (+ mAP metrics when ``compute_map``)."""
    model.eval()
    sums = dict.fromkeys(_PARTS, 0.0)
    n = 0
    with torch.no_grad():
        for images, targets in dataloader:
            _, parts = criterion(model(images.to(device)), targets.to(device))
            for k in _PARTS:
                sums[k] += parts[k]
            n += 1
    results = {k: v / max(n, 1) for k, v in sums.items()}
    if compute_map:
        m = evaluate_model(model=model, dataloader=dataloader, device=device, num_classes=num_classes,
                           iou_thresholds=None, conf_threshold=0.01, nms_threshold=0.4)
        for k in ("mAP50:95", "mAP50", "mAP75", "precision", "recall", "mAP50:95_small", "mAP50:95_medium", "mAP50:95_large"):
            if k in m:
                results[k] = m[k]
    return results


def seed_epoch(seed: int, epoch: int, train_loader=None) -> None:
    """all generators of the process from (seed, epoch); the loader's own generator (shuffling, the base seed of its workers) too"""
    import random

    import numpy as np
    s = (int(seed) * 1000003 + int(epoch)) % (1 << 31)
    torch.manual_seed(s)                # host generator and every device's
    np.random.seed(s)
    random.seed(s)
    gen = getattr(train_loader, "generator", None)
    if gen is not None:
        gen.manual_seed(s)


def train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, num_epochs: int, checkpoint_dir,
          save_frequency: int = 5, writer=None, compute_map: bool = False, map_frequency: int = 5, num_classes: int = 20,
          start_epoch: int = 1, best_val_loss_init: float = None, best_map_init: float = None, scaler=None,
          seed: int | None = None, record: dict | None = None, ema=None, accum_steps: int = 1, warmup_steps: int = 0) -> dict[str, float]:
    """Epoch loop with the reference's checkpoint policy: latest every epoch, every ``save_frequency``
    epochs, best validation loss, best mAP50:95.

    ``seed``: every epoch starts from generators seeded by (seed, epoch) -- torch (host and device: the dropout masks), numpy, ``random`` and
    the train loader's shuffling generator -- so epoch e of a resumed run draws what epoch e of the uninterrupted run drew, and no generator
    state has to travel in the checkpoint.  ``record``: extra plain entries for the epoch checkpoints (train.py: seed, deterministic).

    ``ema``: a ``yolo.optim.ModelEMA`` of ``model``: updated after every step, and the copy that is validated -- best-loss and best-mAP selection
    follow the averaged weights.  Every checkpoint then carries them next to the raw ones (checkpoints.py).  With several ranks each keeps its own
    average; they are identical because the parameters are, and nothing is communicated.

    ``accum_steps``: batches per optimizer step (``train_epoch``).  ``warmup_steps``: linear learning-rate warm-up over the run's first optimizer
    steps (``LRWarmup``); a run resumed at ``start_epoch`` continues where the warm-up stood."""
    warmup = make_warmup(optimizer, warmup_steps, start_epoch, train_loader, accum_steps)
    best_val = float("inf") if best_val_loss_init is None else best_val_loss_init
    best_map = 0.0 if best_map_init is None else best_map_init
    final_train = None
    for epoch in range(start_epoch, num_epochs + 1):
        print(f"\n===== Epoch {epoch}/{num_epochs} =====")
        if seed is not None:
            seed_epoch(seed, epoch, train_loader)
        tr = train_epoch(model, train_loader, criterion, optimizer, device, epoch, writer, scaler, ema=ema, accum_steps=accum_steps, **({"warmup": warmup} if warmup is not None else {}))
        print("  train:", {k: round(v, 4) for k, v in tr.items()})
        want_map = compute_map and (epoch % map_frequency == 0 or epoch == num_epochs)
        va = validate(model if ema is None else ema.module, val_loader, criterion, device, compute_map=want_map, num_classes=num_classes)
        print("  val:  ", {k: round(float(v), 4) for k, v in va.items()})
        scheduler.step()
        lr = optimizer.param_groups[0]["lr"]
        print(f"  learning rate: {lr:.6f}")
        if writer is not None:
            for k in _PARTS:
                writer.add_scalar(f"epoch/train_{k}", tr[k], epoch)
                writer.add_scalar(f"epoch/val_{k}", va[k], epoch)
            writer.add_scalar("epoch/lr", lr, epoch)
        # checkpoints are written by rank 0 only (every rank holds the same parameters and optimizer state; BatchNorm running
        # statistics are per rank -- there is no SyncBN, as in the reference -- and rank 0's are the ones saved); the other
        # ranks wait, so that nobody runs ahead of a file that a later --resume on all ranks would read
        writer_rank = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        if writer_rank:
            save_checkpoint(checkpoint_dir / "yolo_latest.pth", epoch, model, optimizer, scheduler, tr, va, record, ema=ema)
            if epoch % save_frequency == 0:
                save_checkpoint(checkpoint_dir / f"yolo_epoch_{epoch}.pth", epoch, model, optimizer, scheduler, tr, va, record, ema=ema)
        if va["total"] < best_val:
            best_val = va["total"]
            if writer_rank:
                save_best_model(checkpoint_dir / "yolo_best.pth", epoch, model, optimizer, va, "val_loss", best_val, ema=ema)
        if "mAP50:95" in va and va["mAP50:95"] > best_map:
            best_map = va["mAP50:95"]
            if writer_rank:
                save_best_map_model(checkpoint_dir / "yolo_best_map.pth", epoch, model, optimizer, va, best_map, ema=ema)
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
        final_train = tr["total"]
    out = {"best_val_loss": best_val, "final_train_loss": final_train}
    if best_map > 0:
        out["best_mAP50:95"] = best_map
    return out
