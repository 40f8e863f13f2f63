"""Epoch loop of the classification pretraining (pretrain.py), shaped like ``trainer.train_epoch`` / ``validate`` / ``train``.

One step = zero_grad -> model(images) -> SoftmaxCrossEntropy -> backward -> [all-reduce] -> clip (fused into ``yolo.optim`` on a device) ->
skip_if from the loss flag -> step -> ema.update: the order of calls of the detector's loop.  Nothing waits for the device inside a step; the
loss components are read at the print interval only (the epoch means are folded there too: all but the newest is then a copy that landed long
ago).  ``images`` is an fp32 batch or a ``yolo.augment.U8Batch`` (``pretrain.py --device-augment``).

Several ranks and ``accum_steps`` work as in the detector's loop: the classifier runs two plans (trunk, head), ``parallel.make_grad_reducer``
gives each its overlapped reducer and ``yolo.optim.GradAccumulator`` each its arena and accumulator (both find them through
``model.hip_plans()``).  ``SoftmaxCrossEntropy`` is the mean over the local batch, so with equal micro-batches and equal shards the folded,
rank-averaged gradient is the one of the concatenated batch.
"""

from __future__ import annotations

import time

import torch
import torch.distributed as dist

from ..parallel import make_grad_reducer
from .checkpoints import save_best_model, save_checkpoint
from .trainer import _CLIP, make_warmup, seed_epoch

_PARTS = ("total", "top1", "top5")
PRINT_EVERY = 10


class _Means:
    """running means of the loss components; ``fold`` reads the batches queued so far (their copies landed long ago, but for the last)"""

    def __init__(self):
        self.sums, self.n, self.queued = dict.fromkeys(_PARTS, 0.0), 0, []

    def fold(self) -> None:
        for parts in self.queued:
            for k in _PARTS:
                self.sums[k] += parts[k]
            self.n += 1
        self.queued = []

    def result(self) -> dict[str, float]:
        self.fold()
        return {k: v / max(self.n, 1) for k, v in self.sums.items()}


def _progress(epoch, batch_idx, total, parts, t0) -> None:
    print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{total}] Loss: {parts['total']:.4f} "
          f"(top1: {parts['top1']:.4f}, top5: {parts['top5']:.4f}) Time: {time.time() - t0:.2f}s")


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, ema=None, accum_steps: int = 1, warmup=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean loss, top-1 and top-5 accuracy of its batches.  With ``torch.distributed`` initialised the
    gradients are averaged over the ranks before the update.  ``accum_steps`` = K > 1: K batches per optimizer step, EMA update and all-reduce
    (``trainer.train_epoch``); a last group of fewer than K batches is dropped and its losses do not enter the means."""
    model.train()
    means = _Means()
    fused_clip = getattr(optimizer, "max_grad_norm", None) is not None
    allreduce = None
    if dist.is_available() and dist.is_initialized():          # chosen once per model: it attaches a gradient arena to each of its plans
        allreduce = getattr(model, "_yolo_grad_reducer", None)
        if allreduce is None:
            allreduce = make_grad_reducer(model, device)
            model._yolo_grad_reducer = allreduce
    if accum_steps > 1:
        return _train_epoch_accum(model, dataloader, criterion, optimizer, device, epoch, ema, int(accum_steps), allreduce, fused_clip, warmup)
    t0 = time.time()
    for batch_idx, (images, labels) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)
        loss, parts = criterion(model(images), labels)
        loss.backward()
        if allreduce is not None:
            allreduce.all_reduce_mean()
        if not fused_clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=_CLIP)
        if hasattr(optimizer, "skip_if"):
            optimizer.skip_if = getattr(parts, "device_flag", None)      # a batch with a label outside [0, K) updates nothing; the error surfaces at the read
        if warmup is None:
            optimizer.step()
        else:
            warmup.step()
        if ema is not None:
            ema.update(model)
        means.queued.append(parts)
        if (batch_idx + 1) % PRINT_EVERY == 0:
            means.fold()
            _progress(epoch, batch_idx, len(dataloader), parts, t0)
            t0 = time.time()
    return means.result()


def _train_epoch_accum(model, dataloader, criterion, optimizer, device, epoch, ema, K, allreduce, fused_clip, warmup=None) -> dict[str, float]:
    """train_epoch's loop with K batches per optimizer step: ``trainer._train_epoch_accum`` with this loop's loss parts.  The accumulator is kept
    on the model like the reducer it mutes; it starts every epoch at the head of a group."""
    from ..optim import GradAccumulator
    accum = getattr(model, "_yolo_grad_accumulator", None)
    if accum is None or accum.steps != K or accum.reducer is not allreduce:
        accum = model._yolo_grad_accumulator = GradAccumulator(model, K, allreduce)
    accum.micro = 0
    means = _Means()
    group = []                      # the loss parts of the open group: they count once its step is applied
    t0 = time.time()
    for batch_idx, (images, labels) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)        # the accumulator holds the sum (and with an arena the views are re-assigned anyway)
        accum.before_backward()
        loss, parts = criterion(model(images), labels)
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
            means.queued += group
            group = []
        if (batch_idx + 1) % PRINT_EVERY == 0:
            means.fold()
            _progress(epoch, batch_idx, len(dataloader), parts, t0)
            t0 = time.time()
    for r in getattr(accum, "_overlapped", ()):
        r.muted = False              # a dropped incomplete group leaves the reducer as it was found
    return means.result()


def validate(model, dataloader, criterion, device) -> dict[str, float]:
    """Mean loss, top-1 and top-5 accuracy over ``dataloader`` (means of the batch means, like ``trainer.validate``)."""
    model.eval()
    means = _Means()
    with torch.no_grad():
        for batch_idx, (images, labels) in enumerate(dataloader):
            _, parts = criterion(model(images.to(device)), labels.to(device))
            means.queued.append(parts)
            if (batch_idx + 1) % PRINT_EVERY == 0:
                means.fold()
    return means.result()


def train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, num_epochs: int, checkpoint_dir, save_frequency: int = 5,
          start_epoch: int = 1, best_top1_init: float | None = None, seed: int | None = None, record: dict | None = None, ema=None,
          accum_steps: int = 1, warmup_steps: int = 0) -> dict[str, float]:
    """Epoch loop: the latest checkpoint every epoch (``yolo_latest.pth``), one every ``save_frequency`` epochs, and the best validation top-1
    (``yolo_best_top1.pth``).  Checkpoints are ``checkpoints.save_checkpoint``'s, key for key; ``record`` adds ``num_classes`` / ``image_size``
    (and ``seed`` / ``deterministic``).  ``seed``, ``ema``: as in ``trainer.train`` -- the averaged copy is the one validated.
    ``accum_steps``: batches per optimizer step (``train_epoch``).  With several ranks the conduct is ``trainer.train``'s: every rank validates
    (the replicas are identical), rank 0 alone writes the checkpoints and prints their lines, and a barrier follows.  ``warmup_steps``: the
    linear learning-rate warm-up of ``trainer.LRWarmup``, continued across a resume."""
    warmup = make_warmup(optimizer, warmup_steps, start_epoch, train_loader, accum_steps)
    best_top1 = -1.0 if best_top1_init is None else best_top1_init
    final_train = None
    for epoch in range(start_epoch, num_epochs + 1):
        print(f"\n===== Epoch {epoch}/{num_epochs} =====")
        if seed is not None:
            seed_epoch(seed, epoch, train_loader)
        tr = train_epoch(model, train_loader, criterion, optimizer, device, epoch, ema=ema, accum_steps=accum_steps, **({"warmup": warmup} if warmup is not None else {}))
        print("  train:", {k: round(v, 4) for k, v in tr.items()})
        va = validate(model if ema is None else ema.module, val_loader, criterion, device)
        print("  val:  ", {k: round(float(v), 4) for k, v in va.items()})
        scheduler.step()
        print(f"  learning rate: {optimizer.param_groups[0]['lr']:.6f}")
        rec = {**(record or {}), "val_top1": float(va["top1"]), "val_top5": float(va["top5"])}
        # rank 0 writes, the others wait: nobody runs ahead of a file that a later --resume on all ranks would read (trainer.train)
        distributed = dist.is_available() and dist.is_initialized()
        writer_rank = not distributed or dist.get_rank() == 0
        if writer_rank:
            save_checkpoint(checkpoint_dir / "yolo_latest.pth", epoch, model, optimizer, scheduler, tr, va, rec, ema=ema)
            if epoch % save_frequency == 0:
                save_checkpoint(checkpoint_dir / f"yolo_epoch_{epoch}.pth", epoch, model, optimizer, scheduler, tr, va, rec, ema=ema)
        if va["top1"] > best_top1:
            best_top1 = va["top1"]
            if writer_rank:
                save_best_model(checkpoint_dir / "yolo_best_top1.pth", epoch, model, optimizer, va, "val_top1", best_top1, ema=ema)
        if distributed:
            dist.barrier()
        final_train = tr["total"]
    return {"best_val_top1": best_top1, "final_train_loss": final_train}
