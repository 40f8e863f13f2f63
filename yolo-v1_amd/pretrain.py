#!/usr/bin/env python3
"""Classification pretraining of the YOLOv1 trunk -- the stage of the paper (section 2.2) in front of detection training: the first 20
convolutions, an average pool and one fully connected layer as a 224 x 224 classifier.  The reference has no such stage (it downloads
torchvision's ImageNet weights for a ResNet-50); this is what gives ``train.py --backbone yolov1`` features to start from.

    python yolo-v1_amd/pretrain.py --device cuda --data-root /data/imagenet --epochs 90 --optimizer sgd --lr 0.1 --label-smoothing 0.1
    python yolo-v1_amd/pretrain.py --device cuda --synthetic 512 --num-classes 10 --epochs 1
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 yolo-v1_amd/pretrain.py --device cuda --init kaiming \
        --device-augment --accum-steps 2 --data-root /data/imagenet ...
    python yolo-v1_amd/train.py --device cuda --backbone yolov1 --backbone-weights checkpoints_pretrain/yolo_best_top1.pth ...

``--data-root``: ``<root>/{train,val}/<class>/*`` image folders, the classes being the sorted directory names of ``train``.
Several ranks (``torch.distributed.run``: one process per GPU, gradients averaged before every update), ``--accum-steps K`` batches per
update, and ``--device-augment`` (crop, resize, colour jitter, flip and normalisation on the device) work as in train.py: what the two scripts
share is ``yolo.training.cli``.
``--init kaiming``: He initialisation -- the default, the reference's (PyTorch's ``Conv2d`` default), does not train this network from
scratch: behind 20 LeakyReLU(0.1) layers without normalisation the input-dependent part of the activations is ~1e-8 of the first layer's.
"""

from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yolo import SoftmaxCrossEntropy, YOLOv1Classifier  # noqa: E402
from yolo.dataset import ImageFolderClassification, SyntheticClassificationDataset  # noqa: E402
from yolo.models import init_kaiming_  # noqa: E402
from yolo.parallel import broadcast_parameters  # noqa: E402
from yolo.training import classify, cli  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    cli.add_common_arguments(ap, optimizer="sgd", lr=1e-2, epochs=90, lr_decay_epochs="30,60,80", checkpoint_dir="checkpoints_pretrain")
    ap.add_argument("--data-root", default=None, help="<root>/{train,val}/<class>/* image folders")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images of --num-classes classes (no dataset needed)")
    ap.add_argument("--num-classes", type=int, default=None, help="default: the class directories of --data-root, or 10 with --synthetic")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--label-smoothing", type=float, default=0.0)
    ap.add_argument("--init", choices=["default", "kaiming"], default="default",
                    help="default: PyTorch's Conv2d / Linear initialisation, the reference's -- it does NOT train this 20-layer network from scratch "
                         "(no normalisation layers: the input-dependent part of the activations shrinks by ~0.4 per layer, to ~1e-8 of the first "
                         "layer's behind the 20th; 30 SGD steps on 8 images leave the loss at ln 4 = 1.3863).  kaiming: He initialisation for "
                         "LeakyReLU(0.1), zero biases, the logits layer as it is (yolo.models.init_kaiming_; the same 30 steps: 1.4510 -> 0.6878).  "
                         "--resume wins over it")
    ap.add_argument("--device-augment", action="store_true",
                    help="loaders ship decoded uint8 images + sampled parameters; crop / resize / colour jitter / flip / normalise run on the device "
                         "(the same bits as the host path for the same draws).  Works with --synthetic too (its samples are uint8 images)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if bool(a.synthetic) == bool(a.data_root):
        ap.error("give exactly one of --data-root and --synthetic")
    if not 0.0 <= a.label_smoothing < 1.0:
        ap.error("--label-smoothing must lie in [0, 1)")
    if a.image_size < 32 or a.image_size % 32:
        ap.error("--image-size must be a multiple of 32 (the trunk halves the map five times)")
    run = cli.begin(ap, a)
    device = run.device

    u8 = {"device_transform": True} if a.device_augment else {}          # (without the option the datasets are built as before it existed)
    if a.synthetic:
        classes = a.num_classes or 10
        train_ds = SyntheticClassificationDataset(a.synthetic, classes, a.image_size, seed=0, train=True, **u8)
        val_ds = SyntheticClassificationDataset(max(min(a.batch_size, a.synthetic), a.synthetic // 8), classes, a.image_size, seed=1, train=False, **u8)
        val_ds.patterns = train_ds.patterns          # the same classes, other samples
    else:
        train_ds = ImageFolderClassification(a.data_root, "train", a.image_size, **u8)
        val_ds = ImageFolderClassification(a.data_root, "val", a.image_size, classes=train_ds.classes, **u8)
        classes = len(train_ds.classes)
        if a.num_classes is not None and a.num_classes != classes:
            ap.error(f"--num-classes {a.num_classes}, but {a.data_root}/train holds {classes} class directories")
    collate = None
    if a.device_augment:
        import functools

        from yolo.augment import collate_u8
        collate = functools.partial(collate_u8, size=(a.image_size, a.image_size))
    # (a rank's shard smaller than one batch is kept as its one short batch)
    train_loader, val_loader = cli.make_loaders(a, run, train_ds, val_ds, collate, drop_last=lambda per_rank: per_rank >= a.batch_size)

    model = YOLOv1Classifier(num_classes=classes, batch_norm=True) if a.batch_norm else YOLOv1Classifier(num_classes=classes)
    if a.init == "kaiming" and not a.resume:
        init_kaiming_(model)
    model = model.to(device)
    if run.world > 1:
        broadcast_parameters(model)
    criterion = SoftmaxCrossEntropy(label_smoothing=a.label_smoothing)
    optimizer = cli.make_optimizer(a, run, model)
    if device == "cuda":
        # the Linear layer's bf16 operand is refreshed by the pass that updates its master.  The update stays in the foreground, with and without
        # --accum-steps: this Linear layer is 1024 x classes, there is nothing worth hiding beside the next forward (train.py keeps the
        # detector's 822 MB update in the foreground under accumulation for the measured reason given there)
        optimizer.attach_plan(model.head_plan())
    scheduler = cli.make_scheduler(a, optimizer)

    ck = cli.load_resume(ap, a, run)
    if ck is not None and ck.get("num_classes", classes) != classes:
        ap.error(f"--resume {a.resume} was trained with {ck['num_classes']} classes, this run has {classes}")
    start_epoch = cli.resume(a, ck, model, optimizer, scheduler)
    best_top1 = ck.get("val_top1") if ck is not None else None
    ema = cli.make_ema(a, run, ck, model, optimizer)

    ckdir = cli.checkpoint_dir(a, run)
    record, extra = cli.record_and_extra(a, {"num_classes": classes, "image_size": a.image_size})
    res = classify.train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, a.epochs, ckdir, save_frequency=a.save_frequency,
                         start_epoch=start_epoch, best_top1_init=best_top1, seed=a.seed, record=record, ema=ema, **extra)
    cli.finish(run, res)


if __name__ == "__main__":
    main()
