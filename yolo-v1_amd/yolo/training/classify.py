"""Epoch loop of the classification pretraining (pretrain.py), shaped like ``trainer.train_epoch`` / ``validate`` / ``train``.

One step = zero_grad -> model(images) -> SoftmaxCrossEntropy -> backward -> [all-reduce] -> clip (fused into ``yolo.optim`` on a device) ->
skip_if from the loss flag -> step -> ema.update: ``loop.train_epoch``, the detector's loop.  Nothing waits for the device inside a step; the
loss components are read at the print interval only (the epoch means are folded there too: all but the newest is then a copy that landed long
ago).  ``images`` is an fp32 batch or a ``yolo.augment.U8Batch`` (``pretrain.py --device-augment``).

Several ranks and ``accum_steps`` work as in the detector's loop: the classifier runs two plans (trunk, head), ``parallel.make_grad_reducer``
gives each its overlapped reducer and ``yolo.optim.GradAccumulator`` each its arena and accumulator (both find them through
``model.hip_plans()``).  ``SoftmaxCrossEntropy`` is the mean over the local batch, so with equal micro-batches and equal shards the folded,
rank-averaged gradient is the one of the concatenated batch.
"""

from __future__ import annotations

import time

from . import loop
from .checkpoints import save_best_model

_PARTS = ("total", "top1", "top5")
PRINT_EVERY = 10


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, ema=None, accum_steps: int = 1, warmup=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean loss, top-1 and top-5 accuracy of its batches.  With ``torch.distributed`` initialised the
    gradients are averaged over the ranks before the update.  ``accum_steps`` = K > 1: K batches per optimizer step, EMA update and all-reduce
    (``trainer.train_epoch``); a last group of fewer than K batches is dropped and its losses do not enter the means."""
    def progress(batch_idx, parts, t0):
        print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{len(dataloader)}] Loss: {parts['total']:.4f} "
              f"(top1: {parts['top1']:.4f}, top5: {parts['top5']:.4f}) Time: {time.time() - t0:.2f}s")
    return loop.train_epoch(model, dataloader, criterion, optimizer, device, epoch, _PARTS, progress, eager=False, every=PRINT_EVERY, ema=ema,
                            accum_steps=accum_steps, warmup=warmup)


def validate(model, dataloader, criterion, device) -> dict[str, float]:
    """Mean loss, top-1 and top-5 accuracy over ``dataloader`` (means of the batch means, like ``trainer.validate``)."""
    return loop.validate(model, dataloader, criterion, device, _PARTS, every=PRINT_EVERY)


def train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, num_epochs: int, checkpoint_dir, save_frequency: int = 5,
          start_epoch: int = 1, best_top1_init: float | None = None, seed: int | None = None, record: dict | None = None, ema=None,
          accum_steps: int = 1, warmup_steps: int = 0) -> dict[str, float]:
    """Epoch loop: the latest checkpoint every epoch (``yolo_latest.pth``), one every ``save_frequency`` epochs, and the best validation top-1
    (``yolo_best_top1.pth``).  Checkpoints are ``checkpoints.save_checkpoint``'s, key for key; ``record`` adds ``num_classes`` / ``image_size``
    (and ``seed`` / ``deterministic``).  ``seed``, ``ema``: as in ``trainer.train`` -- the averaged copy is the one validated.
    ``accum_steps``: batches per optimizer step (``train_epoch``).  With several ranks the conduct is ``trainer.train``'s (``loop.epochs``): every
    rank validates (the replicas are identical), rank 0 alone writes the checkpoints and prints their lines, and a barrier follows.
    ``warmup_steps``: the linear learning-rate warm-up of ``loop.LRWarmup``, continued across a resume."""
    best_top1 = -1.0 if best_top1_init is None else best_top1_init
    final_train = None

    def train_one(epoch, **warm):
        return train_epoch(model, train_loader, criterion, optimizer, device, epoch, ema=ema, accum_steps=accum_steps, **warm)

    def validate_one(epoch, module):
        return validate(module, val_loader, criterion, device)

    for epoch, tr, va, _, writer_rank in loop.epochs(train_one, validate_one, model, train_loader, optimizer, scheduler, num_epochs, start_epoch,
                                                     seed, ema, accum_steps, warmup_steps):
        rec = {**(record or {}), "val_top1": float(va["top1"]), "val_top5": float(va["top5"])}
        if writer_rank:
            loop.save_epoch(checkpoint_dir, epoch, save_frequency, model, optimizer, scheduler, tr, va, rec, ema=ema)
        if va["top1"] > best_top1:
            best_top1 = va["top1"]
            if writer_rank:
                save_best_model(checkpoint_dir / "yolo_best_top1.pth", epoch, model, optimizer, va, "val_top1", best_top1, ema=ema)
        final_train = tr["total"]
    return {"best_val_top1": best_top1, "final_train_loss": final_train}
