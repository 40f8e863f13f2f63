"""Epoch loop with the reference's call signatures (src/yolo/training/trainer.py:23,133,220).

One train step = zero_grad -> model(images) -> criterion -> backward -> clip_grad_norm_(10) -> step: ``loop.train_epoch``, which the
classification pretraining (``classify``) runs too.  On a ROCm device every piece of that runs on the HIP kernels: the model and the loss as
single autograd nodes, and -- when the optimizer is ``yolo.optim.Adam`` built with ``max_grad_norm=10`` --
clipping + Adam as one fused pass (the separate clip call is then skipped).  With
``torch.distributed`` initialised, gradients are averaged over the ranks before the update
(yolo.parallel; the reference is single-device).
"""

from __future__ import annotations

import time

from ..metrics import evaluate_model
from . import loop
from .checkpoints import save_best_map_model, save_best_model
from .loop import LRWarmup, make_warmup, seed_epoch  # noqa: F401  (their home before the loop was shared)

_PARTS = ("total", "coord", "conf_obj", "conf_noobj", "class")


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, writer=None, scaler=None, ema=None, accum_steps: int = 1,
                warmup=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean of each loss component.  ``ema``: a ``yolo.optim.ModelEMA`` of ``model``, moved after every
    optimizer step (on a device it is enqueued like the step itself, nothing waits).

    ``accum_steps`` = K > 1: gradient accumulation (``yolo.optim.GradAccumulator``) -- K batches per optimizer step, EMA update and all-reduce;
    the effective batch is K times the loader's (times the ranks).  A last group of fewer than K batches is dropped, not applied (the spirit of
    ``drop_last=True``), and its losses do not enter the returned means.

    The loss parts of every applied step are read at once (``loop.train_epoch(eager=True)``): that read raises on invalid targets.

    ``scaler`` (the reference's fp16 autocast + GradScaler branch, trainer.py:69-83) is accepted and not used: on a ROCm
    device the engine already computes in bf16 with fp32 accumulation and fp32 master weights, which needs no loss scaling;
    on the CPU the stock fp32 path runs."""
    def progress(batch_idx, parts, t0):
        print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{len(dataloader)}] Loss: {parts['total']:.4f} "
              f"(coord: {parts['coord']:.4f}, conf_obj: {parts['conf_obj']:.4f}, conf_noobj: {parts['conf_noobj']:.4f}, "
              f"class: {parts['class']:.4f}) Time: {time.time() - t0:.2f}s")
        if writer is not None:
            step = (epoch - 1) * len(dataloader) + batch_idx
            for k in _PARTS:
                writer.add_scalar(f"batch/{k}_loss", parts[k], step)
    return loop.train_epoch(model, dataloader, criterion, optimizer, device, epoch, _PARTS, progress, eager=True, ema=ema, accum_steps=accum_steps,
                            warmup=warmup)


def validate(model, dataloader, criterion, device, compute_map: bool = False, num_classes: int = 20) -> dict[str, float]:
    """Mean loss components over ``dataloader`` (+ mAP metrics when ``compute_map``)."""
    results = loop.validate(model, dataloader, criterion, device, _PARTS)
    if compute_map:
        m = evaluate_model(model=model, dataloader=dataloader, device=device, num_classes=num_classes,
                           iou_thresholds=None, conf_threshold=0.01, nms_threshold=0.4)
        for k in ("mAP50:95", "mAP50", "mAP75", "precision", "recall", "mAP50:95_small", "mAP50:95_medium", "mAP50:95_large"):
            if k in m:
                results[k] = m[k]
    return results


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
    best_val = float("inf") if best_val_loss_init is None else best_val_loss_init
    best_map = 0.0 if best_map_init is None else best_map_init
    final_train = None

    def train_one(epoch, **warm):
        return train_epoch(model, train_loader, criterion, optimizer, device, epoch, writer, scaler, ema=ema, accum_steps=accum_steps, **warm)

    def validate_one(epoch, module):
        want_map = compute_map and (epoch % map_frequency == 0 or epoch == num_epochs)
        return validate(module, val_loader, criterion, device, compute_map=want_map, num_classes=num_classes)

    for epoch, tr, va, lr, writer_rank in loop.epochs(train_one, validate_one, model, train_loader, optimizer, scheduler, num_epochs, start_epoch,
                                                      seed, ema, accum_steps, warmup_steps):
        if writer is not None:
            for k in _PARTS:
                writer.add_scalar(f"epoch/train_{k}", tr[k], epoch)
                writer.add_scalar(f"epoch/val_{k}", va[k], epoch)
            writer.add_scalar("epoch/lr", lr, epoch)
        if writer_rank:
            loop.save_epoch(checkpoint_dir, epoch, save_frequency, model, optimizer, scheduler, tr, va, record, ema=ema)
        if va["total"] < best_val:
            best_val = va["total"]
            if writer_rank:
                save_best_model(checkpoint_dir / "yolo_best.pth", epoch, model, optimizer, va, "val_loss", best_val, ema=ema)
        if "mAP50:95" in va and va["mAP50:95"] > best_map:
            best_map = va["mAP50:95"]
            if writer_rank:
                save_best_map_model(checkpoint_dir / "yolo_best_map.pth", epoch, model, optimizer, va, best_map, ema=ema)
        final_train = tr["total"]
    out = {"best_val_loss": best_val, "final_train_loss": final_train}
    if best_map > 0:
        out["best_mAP50:95"] = best_map
    return out
