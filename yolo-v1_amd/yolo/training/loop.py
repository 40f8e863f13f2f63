"""The training step loop and the epoch skeleton, written once for the detector (``trainer``) and the classification pretraining (``classify``).

One step = zero_grad -> [accumulator.before_backward] -> model(images) -> criterion -> backward -> all-reduce, or accumulator.after_backward ->
clip (fused into ``yolo.optim`` on a device) -> skip_if from the loss flag -> step, or warmup.step -> ema.update.  Nothing waits for the device
inside a step; when the loss components are read is the caller's policy (``train_epoch``: ``eager``).
"""

from __future__ import annotations

import time

import torch
import torch.distributed as dist

from ..parallel import make_grad_reducer
from .checkpoints import save_checkpoint

CLIP = 10.0


class LRWarmup:
    """Linear learning-rate warm-up over the first ``steps`` optimizer steps of a run: step k (from 0) runs with every group's learning rate
    multiplied by (k + 1) / steps while k < steps, on top of whatever the scheduler set.  The
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


class Means:
    """running means of the loss components ``keys``; ``fold`` reads the batches queued so far (a read waits for the device)"""

    def __init__(self, keys):
        self.sums, self.n, self.queued = dict.fromkeys(keys, 0.0), 0, []

    def fold(self) -> None:
        for parts in self.queued:
            for k in self.sums:
                self.sums[k] += parts[k]
            self.n += 1
        self.queued = []

    def result(self) -> dict[str, float]:
        self.fold()
        return {k: v / max(self.n, 1) for k, v in self.sums.items()}


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, keys, progress, eager: bool, every: int = 10, ema=None,
                accum_steps: int = 1, warmup=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean of each loss component ``keys`` over the batches whose step was applied.

    ``accum_steps`` = K > 1: gradient accumulation (``yolo.optim.GradAccumulator``) -- K batches per optimizer step, EMA update and all-reduce.
    The accumulator is kept on the model like the reducer it mutes (its buffers are as large as the gradients) and starts every epoch at the head
    of a group; a last group of fewer than K batches is dropped, not applied, and its losses do not enter the means.  K = 1 builds none.

    ``eager``: when the loss parts are read.  True (the detector): those of every applied step at once -- the read is what raises on invalid
    targets before the next step.  False (the classifier): they are queued and read every ``every`` batches and at the end, when all but the
    newest is a copy that landed long ago.  ``progress(batch_idx, parts, t0)`` prints the line of every ``every``-th batch."""
    model.train()
    means = Means(keys)
    fused_clip = getattr(optimizer, "max_grad_norm", None) is not None
    # data parallel: the reducer is chosen once per model (it may attach a gradient arena to each of the model's plans) -- on a GPU
    # the all-reduce overlaps the backward pass, the path bench.py measures
    allreduce = None
    if dist.is_available() and dist.is_initialized():
        allreduce = getattr(model, "_yolo_grad_reducer", None)
        if allreduce is None:
            allreduce = make_grad_reducer(model, device)
            model._yolo_grad_reducer = allreduce
    accum = None
    if accum_steps > 1:
        from ..optim import GradAccumulator
        accum = getattr(model, "_yolo_grad_accumulator", None)
        if accum is None or accum.steps != int(accum_steps) or accum.reducer is not allreduce:
            accum = model._yolo_grad_accumulator = GradAccumulator(model, int(accum_steps), allreduce)
        accum.micro = 0
    group = []                      # the loss parts of the open group: they count once its step is applied
    t0 = time.time()
    for batch_idx, (images, targets) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)        # (an accumulator holds the sum, and with an arena the views are re-assigned anyway)
        if accum is not None:
            accum.before_backward()
        loss, parts = criterion(model(images), targets)
        loss.backward()
        group.append(parts)
        if accum is not None:
            apply = accum.after_backward(getattr(parts, "device_flag", None))
        else:
            apply = True
            if allreduce is not None:
                allreduce.all_reduce_mean()
        if apply:
            if not fused_clip:
                torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=CLIP)
            if hasattr(optimizer, "skip_if"):
                # yolo.optim: a step whose targets the loss kernel flagged as invalid updates nothing (the error itself surfaces at the read of
                # the parts; the reference raises inside the loss, before any update).  One flagged batch cancels its group's step (and, through
                # last_skip, the EMA's)
                optimizer.skip_if = accum.skip_if if accum is not None else getattr(parts, "device_flag", None)
            if warmup is None:
                optimizer.step()
            else:
                warmup.step()
            if ema is not None:
                ema.update(model)
            means.queued += group
            group = []
            if eager:
                means.fold()
        if (batch_idx + 1) % every == 0:
            means.fold()
            progress(batch_idx, parts, t0)
            t0 = time.time()
    for r in getattr(accum, "_overlapped", ()):
        r.muted = False              # a dropped incomplete group leaves the reducer as it was found
    return means.result()


def validate(model, dataloader, criterion, device, keys, every: int = 1) -> dict[str, float]:
    """Mean loss components ``keys`` over ``dataloader`` (means of the batch means), read every ``every`` batches"""
    model.eval()
    means = Means(keys)
    with torch.no_grad():
        for batch_idx, (images, targets) in enumerate(dataloader):
            _, parts = criterion(model(images.to(device)), targets.to(device))
            means.queued.append(parts)
            if (batch_idx + 1) % every == 0:
                means.fold()
    return means.result()


def epochs(train_one, validate_one, model, train_loader, optimizer, scheduler, num_epochs: int, start_epoch: int, seed, ema,
           accum_steps: int, warmup_steps: int):
    """The epoch skeleton of both ``train`` functions, as a generator: per epoch it seeds, trains (``train_one(epoch, **warmup)``), validates the
    averaged copy where there is one (``validate_one(epoch, module)``), steps the scheduler and prints their lines, then yields
    ``(epoch, train means, validation means, learning rate, writer_rank)`` for the caller's checkpoints.  Checkpoints are written by rank 0 only
    (every rank holds the same parameters and optimizer state; BatchNorm running statistics are per rank -- there is no SyncBN, as in the
    reference -- and rank 0's are the ones saved); behind the caller's turn the other ranks wait at a barrier, so that nobody runs ahead of a file
    that a later --resume on all ranks would read."""
    warmup = make_warmup(optimizer, warmup_steps, start_epoch, train_loader, accum_steps)
    for epoch in range(start_epoch, num_epochs + 1):
        print(f"\n===== Epoch {epoch}/{num_epochs} =====")
        if seed is not None:
            seed_epoch(seed, epoch, train_loader)
        tr = train_one(epoch, **({"warmup": warmup} if warmup is not None else {}))
        print("  train:", {k: round(v, 4) for k, v in tr.items()})
        va = validate_one(epoch, model if ema is None else ema.module)
        print("  val:  ", {k: round(float(v), 4) for k, v in va.items()})
        scheduler.step()
        lr = optimizer.param_groups[0]["lr"]
        print(f"  learning rate: {lr:.6f}")
        distributed = dist.is_available() and dist.is_initialized()
        yield epoch, tr, va, lr, not distributed or dist.get_rank() == 0
        if distributed:
            dist.barrier()


def save_epoch(checkpoint_dir, epoch: int, save_frequency: int, *state, **kw) -> None:
    """the latest checkpoint, and one every ``save_frequency`` epochs (``checkpoints.save_checkpoint``'s arguments behind the epoch)"""
    save_checkpoint(checkpoint_dir / "yolo_latest.pth", epoch, *state, **kw)
    if epoch % save_frequency == 0:
        save_checkpoint(checkpoint_dir / f"yolo_epoch_{epoch}.pth", epoch, *state, **kw)
