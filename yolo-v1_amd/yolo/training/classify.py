"""Epoch loop of the classification pretraining (pretrain.py), shaped like ``trainer.train_epoch`` / ``validate`` / ``train``.

One step = zero_grad -> model(images) -> SoftmaxCrossEntropy -> backward -> clip (fused into ``yolo.optim`` on a device) -> skip_if from the
loss flag -> step -> ema.update: the order of calls of the detector's loop.  Nothing waits for the device inside a step; the loss components
are read at the print interval only (the epoch means are folded there too: all but the newest is then a copy that landed long ago).
Single process, one batch per step: ``--accum-steps`` and several ranks are written against ONE plan's gradient arena
(``yolo.optim.GradAccumulator``, ``yolo.parallel``) and this model runs two -- the follow-up.
"""

from __future__ import annotations

import time

import torch

from .checkpoints import save_best_model, save_checkpoint
from .trainer import _CLIP, seed_epoch

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


def train_epoch(model, dataloader, criterion, optimizer, device, epoch: int, ema=None) -> dict[str, float]:
    """One pass over ``dataloader``; returns the mean loss, top-1 and top-5 accuracy of its batches."""
    model.train()
    means = _Means()
    fused_clip = getattr(optimizer, "max_grad_norm", None) is not None
    t0 = time.time()
    for batch_idx, (images, labels) in enumerate(dataloader):
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        optimizer.zero_grad(set_to_none=True)
        loss, parts = criterion(model(images), labels)
        loss.backward()
        if not fused_clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=_CLIP)
        if hasattr(optimizer, "skip_if"):
            optimizer.skip_if = getattr(parts, "device_flag", None)      # a batch with a label outside [0, K) updates nothing; the error surfaces at the read
        optimizer.step()
        if ema is not None:
            ema.update(model)
        means.queued.append(parts)
        if (batch_idx + 1) % PRINT_EVERY == 0:
            means.fold()
            print(f"Epoch [{epoch}] Batch [{batch_idx + 1}/{len(dataloader)}] Loss: {parts['total']:.4f} "
                  f"(top1: {parts['top1']:.4f}, top5: {parts['top5']:.4f}) Time: {time.time() - t0:.2f}s")
            t0 = time.time()
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
          start_epoch: int = 1, best_top1_init: float | None = None, seed: int | None = None, record: dict | None = None, ema=None) -> dict[str, float]:
    """Epoch loop: the latest checkpoint every epoch (``yolo_latest.pth``), one every ``save_frequency`` epochs, and the best validation top-1
    (``yolo_best_top1.pth``).  Checkpoints are ``checkpoints.save_checkpoint``'s, key for key; ``record`` adds ``num_classes`` / ``image_size``
    (and ``seed`` / ``deterministic``).  ``seed``, ``ema``: as in ``trainer.train`` -- the averaged copy is the one validated."""
    best_top1 = -1.0 if best_top1_init is None else best_top1_init
    final_train = None
    for epoch in range(start_epoch, num_epochs + 1):
        print(f"\n===== Epoch {epoch}/{num_epochs} =====")
        if seed is not None:
            seed_epoch(seed, epoch, train_loader)
        tr = train_epoch(model, train_loader, criterion, optimizer, device, epoch, ema=ema)
        print("  train:", {k: round(v, 4) for k, v in tr.items()})
        va = validate(model if ema is None else ema.module, val_loader, criterion, device)
        print("  val:  ", {k: round(float(v), 4) for k, v in va.items()})
        scheduler.step()
        print(f"  learning rate: {optimizer.param_groups[0]['lr']:.6f}")
        rec = {**(record or {}), "val_top1": float(va["top1"]), "val_top5": float(va["top5"])}
        save_checkpoint(checkpoint_dir / "yolo_latest.pth", epoch, model, optimizer, scheduler, tr, va, rec, ema=ema)
        if epoch % save_frequency == 0:
            save_checkpoint(checkpoint_dir / f"yolo_epoch_{epoch}.pth", epoch, model, optimizer, scheduler, tr, va, rec, ema=ema)
        if va["top1"] > best_top1:
            best_top1 = va["top1"]
            save_best_model(checkpoint_dir / "yolo_best_top1.pth", epoch, model, optimizer, va, "val_top1", best_top1, ema=ema)
        final_train = tr["total"]
    return {"best_val_top1": best_top1, "final_train_loss": final_train}
