"""Checkpoint files with the reference's dictionary keys (src/yolo/training/checkpoints.py:32-113), so
checkpoints are interchangeable in both directions: ``epoch, model_state_dict, optimizer_state_dict,
[scheduler_state_dict], [train_loss], val_loss, [mAP50:95, mAP50, mAP75]`` (+ ``seed``, ``deterministic`` from ``train.py --seed / --deterministic``;
+ ``ema_state_dict``, ``ema_updates`` from ``train.py --ema-decay``: the averaged weights next to the raw ones, which stay in ``model_state_dict`` so that
``--resume`` continues the optimizer's trajectory exactly; the reference's loader never reads the extra keys)."""

from __future__ import annotations

import os
from pathlib import Path

import torch


def _atomic_save(data: dict, path) -> None:
    """write next to the target and rename: a reader (or a crash) never sees a half-written checkpoint"""
    tmp = f"{path}.tmp.{os.getpid()}"
    torch.save(data, tmp)
    os.replace(tmp, path)


def _with_map(data: dict, val_losses: dict) -> dict:
    if "mAP50:95" in val_losses:
        for k in ("mAP50:95", "mAP50", "mAP75"):
            data[k] = float(val_losses[k])       # plain floats: NumPy scalars would need pickle to load (weights_only=True refuses them)
    return data


def _with_ema(data: dict, ema) -> dict:
    """``ema``: a ``yolo.optim.ModelEMA`` (None: the file is the reference's, key for key).  Tensors and an int: loads with weights_only=True"""
    if ema is not None:
        sd = ema.state_dict()
        data.update(ema_state_dict=sd["module"], ema_updates=int(sd["updates"]))
    return data


NO_EMA = "checkpoint {path} has no 'ema_state_dict': it was written by a run without --ema-decay (drop --use-ema to load its raw weights)"


def weights_of(ck: dict, use_ema: bool, path="") -> dict:
    """the state dict evaluate.py / predict.py load: the raw weights, or the averaged ones (``--use-ema``)"""
    if not use_ema:
        return ck["model_state_dict"]
    if "ema_state_dict" not in ck:
        raise SystemExit(NO_EMA.format(path=path))
    return ck["ema_state_dict"]


def save_checkpoint(checkpoint_path: Path, epoch: int, model, optimizer, scheduler, train_losses: dict, val_losses: dict, record: dict | None = None,
                    ema=None) -> None:
    """``record``: extra plain entries (train.py: ``seed``, ``deterministic``) -- keys the reference's loader never reads, so the file still loads there"""
    data = {**(record or {}), "epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
            "scheduler_state_dict": scheduler.state_dict(), "train_loss": float(train_losses["total"]), "val_loss": float(val_losses["total"])}
    _atomic_save(_with_ema(_with_map(data, val_losses), ema), checkpoint_path)
    print(f"  checkpoint saved: {checkpoint_path}")


def save_best_model(checkpoint_path: Path, epoch: int, model, optimizer, val_losses: dict, metric_name: str, metric_value: float, ema=None) -> None:
    data = {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(), "val_loss": float(val_losses["total"])}
    _atomic_save(_with_ema(_with_map(data, val_losses), ema), checkpoint_path)
    print(f"  new best model ({metric_name}={metric_value:.4f}) saved: {checkpoint_path}")


def save_best_map_model(checkpoint_path: Path, epoch: int, model, optimizer, val_losses: dict, best_map: float, ema=None) -> None:
    save_best_model(checkpoint_path, epoch, model, optimizer, val_losses, "mAP50:95", best_map, ema)
