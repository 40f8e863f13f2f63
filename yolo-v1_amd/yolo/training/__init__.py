"""Training orchestration (glue around the HIP hot path; reference: src/yolo/training/): ``loop`` is the step loop and epoch skeleton that
``trainer`` (detection) and ``classify`` (pretraining) call, ``cli`` what train.py and pretrain.py share."""

from .checkpoints import save_best_map_model, save_best_model, save_checkpoint
from .trainer import train, train_epoch, validate
from . import classify  # noqa: F401  (the classification pretraining loop: classify.train / train_epoch / validate)

__all__ = ["save_best_map_model", "save_best_model", "save_checkpoint", "train", "train_epoch", "validate"]
