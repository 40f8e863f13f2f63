#!/usr/bin/env python3
"""Training entry point (the reference's src/train.py without the Modal cloud wrapper).

    python yolo-v1_amd/train.py --device cuda --backbone yolov1 --synthetic 512 --epochs 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 yolo-v1_amd/train.py --device cuda ...

Defaults follow src/train.py:269-338: batch 64, lr 1e-4, weight decay 5e-4, LR decay x0.1 at epochs
75 and 105, lambda_coord 5, lambda_noobj 0.5.  ``--backbone`` is additive (the reference hard-codes
ResNet50, which needs torchvision); ``--synthetic N`` trains on N random images instead of PASCAL VOC;
``--backbone yolov1 --backbone-weights PATH`` starts from a trunk that pretrain.py trained as a classifier (the paper's first stage);
``--init kaiming`` gives what that file does not hold (or, without one, the whole network) He initialisation -- the default, the
reference's, does not train the 24-layer network from scratch (``yolo.models.init_kaiming_``).
What this script shares with pretrain.py (the common options, seeding, ranks, loaders, optimizer, ``--resume``, EMA) is ``yolo.training.cli``.
"""

from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from yolo import YOLOLoss, YOLOv1, ResNetBackbone, YOLOv1Backbone  # noqa: E402
from yolo import training  # noqa: E402
from yolo.dataset import SyntheticYOLODataset, create_voc_datasets  # noqa: E402
from yolo.parallel import broadcast_parameters  # noqa: E402
from yolo.training import cli  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_common_arguments(ap, optimizer="adam", lr=1e-4, epochs=135, lr_decay_epochs="75,105", checkpoint_dir="checkpoints")
    ap.add_argument("--backbone", choices=["resnet50", "yolov1"], default="resnet50")
    ap.add_argument("--lambda-coord", type=float, default=5.0)
    ap.add_argument("--lambda-noobj", type=float, default=0.5)
    ap.add_argument("--freeze-backbone", action="store_true")
    ap.add_argument("--no-pretrained", action="store_true", help="random-init ResNet50 (no torchvision / ImageNet weights available)")
    ap.add_argument("--compute-map", action="store_true")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images (no dataset needed)")
    ap.add_argument("--device-augment", action="store_true",
                    help="VOC only: loaders ship decoded uint8 images + sampled parameters, crop / resize / colour jitter / normalise run on the device")
    ap.add_argument("--augment", choices=["reference", "darknet"], default="reference",
                    help="VOC only, the training augmentation: reference = RandomResizedCrop + ColorJitter; darknet = the YOLOv1 paper's recipe (scaling "
                         "and translation by up to 20 %% past the image border, horizontal flip, exposure and saturation up to x1.5 and hue +-0.1 in "
                         "HSV); with and without --device-augment")
    ap.add_argument("--voc-root", default=None, help="dataset root (default: $VOC_ROOT or ./data)")
    ap.add_argument("--backbone-weights", default=None,
                    help="--backbone yolov1 only: a classification checkpoint of pretrain.py whose trunk (features.N.*) initialises the backbone "
                         "(YOLOv1Backbone.load_pretrained); --resume wins over it.  Default: random initialisation")
    ap.add_argument("--use-ema", action="store_true", help="with --backbone-weights: take the checkpoint's averaged weights (ema_state_dict) when it has them")
    ap.add_argument("--init", choices=["default", "kaiming"], default="default",
                    help="default: PyTorch's Conv2d / Linear initialisation, the reference's -- with --backbone yolov1 it does NOT train the 24-layer "
                         "network from scratch (no normalisation layers: the input-dependent part of the activations shrinks by ~0.4 per layer, to "
                         "~1e-8 of the first layer's behind the 20th convolution; the 20-layer classifier stays at ln 4 = 1.3863 over 30 SGD steps "
                         "where He initialisation goes 1.4510 -> 0.6878).  kaiming: He initialisation for LeakyReLU(0.1) with zero biases, the output "
                         "layer as it is (yolo.models.init_kaiming_); applied before --backbone-weights, which then overwrites the 40 trunk tensors "
                         "(the four detection convolutions and FC1 keep it); --backbone resnet50: the head only.  --resume wins over it")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if a.batch_norm and a.backbone != "yolov1":
        ap.error("--batch-norm needs --backbone yolov1 (the ResNet-50 trunk has its BatchNorm layers already)")
    if a.augment != "reference" and a.synthetic:
        ap.error("--augment needs the VOC datasets (synthetic samples are not augmented)")
    if a.backbone_weights and a.backbone != "yolov1":
        ap.error("--backbone-weights needs --backbone yolov1 (a classification checkpoint of pretrain.py holds that trunk)")
    if a.deterministic and a.backbone == "resnet50":
        # (the training loop puts the whole model in train(): there is no eval-mode trunk to ask for here)
        from yolo.models import BN_STATS_NOT_DETERMINISTIC
        ap.error(BN_STATS_NOT_DETERMINISTIC)
    run = cli.begin(ap, a)
    device, rank = run.device, run.rank

    if a.synthetic:
        train_ds, val_ds = SyntheticYOLODataset(a.synthetic, seed=0), SyntheticYOLODataset(max(a.batch_size, a.synthetic // 8), seed=1)
    else:
        train_ds = create_voc_datasets([("2007", "trainval"), ("2012", "train")], augment=True, root=a.voc_root,
                                       device_transform=a.device_augment, recipe=a.augment)     # the reference's splits (src/train.py:106-122)
        val_ds = create_voc_datasets([("2012", "val")], augment=False, root=a.voc_root, device_transform=a.device_augment)
    collate = None
    if a.device_augment:
        if a.synthetic:
            ap.error("--device-augment needs the VOC datasets (synthetic samples are fp32 tensors already)")
        from yolo.augment import collate_u8
        collate = collate_u8
    train_loader, val_loader = cli.make_loaders(a, run, train_ds, val_ds, collate, drop_last=True)

    backbone = (YOLOv1Backbone(batch_norm=True) if a.batch_norm else YOLOv1Backbone()) if a.backbone == "yolov1" else ResNetBackbone(pretrained=not a.no_pretrained, freeze=a.freeze_backbone)
    model = YOLOv1(backbone=backbone, num_classes=20, S=7, B=2)
    if a.init == "kaiming" and not a.resume:
        from yolo.models import init_kaiming_
        init_kaiming_(model if a.backbone == "yolov1" else model.head)
    if a.backbone_weights and not a.resume:          # behind --init: the checkpoint's 40 trunk tensors replace whatever the trunk was given
        ck0 = torch.load(a.backbone_weights, map_location="cpu", weights_only=True)
        if bool(ck0.get("batch_norm", False)) != a.batch_norm:
            ap.error(f"--backbone-weights {a.backbone_weights} records batch_norm={bool(ck0.get('batch_norm', False))}, this run has "
                     f"batch_norm={a.batch_norm} (--batch-norm): the two must agree")
        sd = ck0["ema_state_dict"] if (a.use_ema and "ema_state_dict" in ck0) else ck0["model_state_dict"]
        loaded = backbone.load_pretrained(sd)
        if rank == 0:
            print(f"backbone: loaded {loaded} tensors from {a.backbone_weights}" + (" (averaged weights)" if sd is not ck0["model_state_dict"] else ""))
        del ck0, sd
    model = model.to(device)
    if run.world > 1:
        broadcast_parameters(model)
    criterion = YOLOLoss(S=7, B=2, C=20, lambda_coord=a.lambda_coord, lambda_noobj=a.lambda_noobj)
    optimizer = cli.make_optimizer(a, run, model)
    if device == "cuda":
        if model._fusable():
            # the Linear layers' update runs as a background pass beside the next forward's conv stack (11.40 vs 11.58 ms per step
            # at batch 64: the persistent conv kernels draw their tiles from a queue, so the held CUs cost only their share).  With
            # --accum-steps K > 1 the update stays in the foreground: one step per K batches leaves one forward in K to hide it under, and
            # beside the gradient arena the background form measured slower (13.04 vs 10.53 ms per batch at K = 4)
            optimizer.attach_plan(model.hip_plan(), overlap=a.accum_steps == 1)
        elif hasattr(model.head, "hip_plan"):          # DetectionHead on a ResNet trunk: its Linear layers' bf16 operands
            optimizer.attach_plan(model.head.hip_plan())
        elif a.batch_norm:                             # the default head behind the BatchNorm chain: a plan of its own
            optimizer.attach_plan(model.head_plan())
    scheduler = cli.make_scheduler(a, optimizer)

    ck = cli.load_resume(ap, a, run)
    start_epoch = cli.resume(a, ck, model, optimizer, scheduler)
    best_val, best_map = (ck.get("val_loss"), ck.get("mAP50:95")) if ck is not None else (None, None)
    ema = cli.make_ema(a, run, ck, model, optimizer)

    ckdir = cli.checkpoint_dir(a, run)
    record, extra = cli.record_and_extra(a, {"augment": a.augment} if a.augment != "reference" else None)
    res = training.train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, a.epochs, ckdir,
                         save_frequency=a.save_frequency, compute_map=a.compute_map, start_epoch=start_epoch,
                         best_val_loss_init=best_val, best_map_init=best_map, seed=a.seed, record=record, ema=ema, **extra)
    cli.finish(run, res)


if __name__ == "__main__":
    main()
