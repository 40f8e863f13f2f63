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
update, and ``--device-augment`` (crop, resize, colour jitter, flip and normalisation on the device) work as in train.py.
``--init kaiming``: He initialisation -- the default, the reference's (PyTorch's ``Conv2d`` default), does not train this network from
scratch: behind 20 LeakyReLU(0.1) layers without normalisation the input-dependent part of the activations is ~1e-8 of the first layer's.
"""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402
from torch.utils.data.distributed import DistributedSampler  # noqa: E402

from yolo import SoftmaxCrossEntropy, YOLOv1Classifier  # noqa: E402
from yolo.dataset import ImageFolderClassification, SyntheticClassificationDataset  # noqa: E402
from yolo.models import init_kaiming_  # noqa: E402
from yolo.parallel import broadcast_parameters  # noqa: E402
from yolo.training import classify as loop  # noqa: E402
from yolo.training.trainer import seed_epoch  # noqa: E402


def _seed_worker(worker_id: int) -> None:
    """DataLoader worker: numpy and ``random`` from the seed torch derived for this worker from the loader's generator"""
    import random

    import numpy as np
    s = torch.initial_seed() % (1 << 31)
    np.random.seed(s)
    random.seed(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--data-root", default=None, help="<root>/{train,val}/<class>/* image folders")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images of --num-classes classes (no dataset needed)")
    ap.add_argument("--num-classes", type=int, default=None, help="default: the class directories of --data-root, or 10 with --synthetic")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--batch-size", type=int, default=64, help="per process")
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=90)
    ap.add_argument("--optimizer", choices=["adam", "sgd", "lars"], default="sgd",
                    help="lars: layer-wise adaptive rate scaling on top of SGD with momentum, for the large effective batches of --accum-steps x ranks "
                         "(yolo.optim.LARS; biases and BatchNorm gamma / beta are neither adapted nor decayed).  Use it with --warmup-steps")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd / lars only")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer sgd only")
    ap.add_argument("--lars-eta", type=float, default=1e-3, help="--optimizer lars only: the trust coefficient")
    ap.add_argument("--warmup-steps", type=int, default=0,
                    help="linear learning-rate warm-up: optimizer step k of the run (from 0) runs at (k + 1) / N of the scheduled rate while k < N; "
                         "--resume continues it.  Default 0: none")
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--lr-decay-epochs", default="30,60,80")
    ap.add_argument("--label-smoothing", type=float, default=0.0)
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights: it is what gets validated, and every checkpoint carries it as "
                         "ema_state_dict (train.py --backbone-weights .. --use-ema).  Default: no EMA")
    ap.add_argument("--ema-tau", type=float, default=0.0, help="warm-up of --ema-decay: decay * (1 - exp(-updates / tau)); 0: none")
    ap.add_argument("--init", choices=["default", "kaiming"], default="default",
                    help="default: PyTorch's Conv2d / Linear initialisation, the reference's -- it does NOT train this 20-layer network from scratch "
                         "(no normalisation layers: the input-dependent part of the activations shrinks by ~0.4 per layer, to ~1e-8 of the first "
                         "layer's behind the 20th; 30 SGD steps on 8 images leave the loss at ln 4 = 1.3863).  kaiming: He initialisation for "
                         "LeakyReLU(0.1), zero biases, the logits layer as it is (yolo.models.init_kaiming_; the same 30 steps: 1.4510 -> 0.6878).  "
                         "--resume wins over it")
    ap.add_argument("--accum-steps", type=int, default=1,
                    help="gradient accumulation: K batches per optimizer step and per all-reduce -- effective batch = batch-size x K x world; a last "
                         "group of an epoch with fewer than K batches is dropped.  Default 1: none")
    ap.add_argument("--device-augment", action="store_true",
                    help="loaders ship decoded uint8 images + sampled parameters; crop / resize / colour jitter / flip / normalise run on the device "
                         "(the same bits as the host path for the same draws).  Works with --synthetic too (its samples are uint8 images)")
    ap.add_argument("--seed", type=int, default=None, help="seed of torch, numpy, random and the loaders (every epoch starts from (seed, epoch))")
    ap.add_argument("--deterministic", action="store_true", help="EngineConfig.DETERMINISTIC: bit-reproducible steps (the new kernels use no atomics anyway)")
    ap.add_argument("--checkpoint-dir", default="checkpoints_pretrain")
    ap.add_argument("--save-frequency", type=int, default=10)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--batch-norm", action="store_true",
                    help="Conv2d(bias=False) + BatchNorm2d + LeakyReLU(0.1) in place of Conv2d + LeakyReLU(0.1) on every convolution of the YOLOv1 network (Darknet's "
                         "batch_normalize=1): trains from the default initialisation.  Recorded in the checkpoint; --resume and --backbone-weights check it")
    ap.add_argument("--factored-fc", action="store_true",
                    help="EngineConfig.FC_FACTORED: the weight gradient of a Linear layer with at least FC_FACTORED_MIN weights (the Linear(50176, 4096) behind "
                         "nn.Flatten) is never stored: the update kernel of --optimizer adam / sgd rebuilds it from its two batch factors, and several ranks "
                         "all-gather 7 MB of factors instead of all-reducing 822 MB.  Not with --optimizer lars, --accum-steps > 1 or --device cpu")
    a = ap.parse_args()
    if bool(a.synthetic) == bool(a.data_root):
        ap.error("give exactly one of --data-root and --synthetic")
    if not 0.0 <= a.label_smoothing < 1.0:
        ap.error("--label-smoothing must lie in [0, 1)")
    if a.accum_steps < 1:
        ap.error("--accum-steps must be at least 1")
    if a.factored_fc:
        if a.optimizer == "lars":
            ap.error("--factored-fc is not supported with --optimizer lars (the trust ratio needs the gradient's per-tensor norm): use adam or sgd")
        if a.accum_steps > 1:
            ap.error("--factored-fc is not supported with --accum-steps > 1 (the sum of K factored gradients is not one product of two factors)")
        if not str(a.device).startswith("cuda"):
            ap.error("--factored-fc is not supported with --device cpu (the factored update runs in the HIP kernels only)")
        from yolo.config import CONFIG as _cfg
        _cfg.FC_FACTORED = True
    if a.optimizer == "lars" and a.nesterov:
        ap.error("--optimizer lars has no Nesterov momentum (--nesterov is --optimizer sgd only)")
    if a.warmup_steps < 0:
        ap.error("--warmup-steps must not be negative")
    if a.image_size < 32 or a.image_size % 32:
        ap.error("--image-size must be a multiple of 32 (the trunk halves the map five times)")
    if a.deterministic and a.batch_norm:
        from yolo.bn_executor import BN_LRELU_NOT_DETERMINISTIC
        ap.error("--deterministic --batch-norm: " + BN_LRELU_NOT_DETERMINISTIC)
    if a.deterministic:
        from yolo.config import CONFIG
        CONFIG.DETERMINISTIC = True
        if a.seed is None:
            a.seed = 0
    gen, worker_init = None, None
    if a.seed is not None:
        seed_epoch(a.seed, 0)                 # parameter initialisation
        gen = torch.Generator()
        gen.manual_seed(a.seed)
        worker_init = _seed_worker

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = a.device
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if device == "cuda":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl" if device == "cuda" else "gloo")

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
    pin = device == "cuda"
    collate = None
    if a.device_augment:
        import functools

        from yolo.augment import collate_u8
        collate = functools.partial(collate_u8, size=(a.image_size, a.image_size))
    sampler = DistributedSampler(train_ds, num_replicas=world, rank=rank) if world > 1 else None
    per_rank = len(train_ds) if sampler is None else len(sampler)
    train_loader = DataLoader(train_ds, batch_size=a.batch_size, shuffle=sampler is None, sampler=sampler, num_workers=a.num_workers, pin_memory=pin,
                              drop_last=per_rank >= a.batch_size, collate_fn=collate, generator=gen, worker_init_fn=worker_init)
    val_loader = DataLoader(val_ds, batch_size=a.batch_size, shuffle=False, num_workers=a.num_workers, pin_memory=pin, collate_fn=collate,
                            worker_init_fn=worker_init)

    model = YOLOv1Classifier(num_classes=classes, batch_norm=True) if a.batch_norm else YOLOv1Classifier(num_classes=classes)
    if a.init == "kaiming" and not a.resume:
        init_kaiming_(model)
    model = model.to(device)
    if world > 1:
        broadcast_parameters(model)
    criterion = SoftmaxCrossEntropy(label_smoothing=a.label_smoothing)
    params = [p for p in model.parameters() if p.requires_grad]
    if device == "cuda":
        from yolo.optim import LARS, SGD, Adam, lars_param_groups     # fused clip(10) + Adam / SGD with momentum / LARS on the HIP kernels
        if a.optimizer == "lars":
            optimizer = LARS(lars_param_groups(model, a.weight_decay), lr=a.lr, momentum=a.momentum, eta=a.lars_eta, max_grad_norm=10.0)
        elif a.optimizer == "sgd":
            optimizer = SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov, max_grad_norm=10.0)
        else:
            optimizer = Adam(params, lr=a.lr, weight_decay=a.weight_decay, max_grad_norm=10.0)
        # the Linear layer's bf16 operand is refreshed by the pass that updates its master.  The update stays in the foreground, with and without
        # --accum-steps: this Linear layer is 1024 x classes, there is nothing worth hiding beside the next forward (train.py keeps the
        # detector's 822 MB update in the foreground under accumulation for the measured reason given there)
        optimizer.attach_plan(model.head_plan())
    elif a.optimizer == "lars":                        # torch has none: the same class, whose CPU parameters take stock torch ops
        from yolo.optim import LARS, lars_param_groups
        optimizer = LARS(lars_param_groups(model, a.weight_decay), lr=a.lr, momentum=a.momentum, eta=a.lars_eta, max_grad_norm=10.0)
    elif a.optimizer == "sgd":
        optimizer = torch.optim.SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov)
    else:
        optimizer = torch.optim.Adam(params, lr=a.lr, weight_decay=a.weight_decay)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(e) for e in a.lr_decay_epochs.split(",")], gamma=0.1)

    start_epoch, best_top1 = 1, None
    if a.resume:
        ck = torch.load(a.resume, map_location=device, weights_only=True)
        if ck.get("num_classes", classes) != classes:
            ap.error(f"--resume {a.resume} was trained with {ck['num_classes']} classes, this run has {classes}")
        if bool(ck.get("batch_norm", False)) != a.batch_norm:
            ap.error(f"--resume {a.resume} records batch_norm={bool(ck.get('batch_norm', False))}, this run has batch_norm={a.batch_norm} "
                     "(--batch-norm): the two must agree")
        model.load_state_dict(ck["model_state_dict"])
        optimizer.load_state_dict(ck["optimizer_state_dict"])
        if "scheduler_state_dict" in ck:
            scheduler.load_state_dict(ck["scheduler_state_dict"])
        start_epoch = ck["epoch"] + 1
        a.init = ck.get("init", "default")          # --resume wins over --init: the weights are the file's, and so is the record of how they began
        best_top1 = ck.get("val_top1")
    ema = None
    if a.ema_decay is not None:
        from yolo.optim import ModelEMA
        ema = ModelEMA(model, decay=a.ema_decay, tau=a.ema_tau, optimizer=optimizer if device == "cuda" else None)
        if a.resume and "ema_state_dict" in ck:
            ema.load_state_dict({"module": ck["ema_state_dict"], "updates": ck.get("ema_updates", 0), "decay": a.ema_decay, "tau": a.ema_tau})

    ckdir = Path(a.checkpoint_dir)
    if rank == 0:
        ckdir.mkdir(parents=True, exist_ok=True)
    record = {"num_classes": classes, "image_size": a.image_size}
    if a.seed is not None:
        record.update(seed=a.seed, deterministic=bool(a.deterministic))
    extra = {}
    if a.accum_steps > 1:          # (1: the call, and the checkpoint's keys, are those of a run without the option)
        record["accum_steps"] = a.accum_steps
        extra["accum_steps"] = a.accum_steps
    if a.init != "default":        # (the default: the checkpoint's keys are those of a run without the option)
        record["init"] = a.init
    if a.batch_norm:               # (likewise)
        record["batch_norm"] = True
    if a.warmup_steps:             # (0: the call is that of a run without the option)
        extra["warmup_steps"] = a.warmup_steps
    res = loop.train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, a.epochs, ckdir, save_frequency=a.save_frequency,
                     start_epoch=start_epoch, best_top1_init=best_top1, seed=a.seed, record=record, ema=ema, **extra)
    if rank == 0:
        print("done:", res)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
