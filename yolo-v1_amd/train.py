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

from yolo import YOLOLoss, YOLOv1, ResNetBackbone, YOLOv1Backbone  # noqa: E402
from yolo import training  # noqa: E402
from yolo.dataset import SyntheticYOLODataset, create_voc_datasets  # noqa: E402
from yolo.parallel import broadcast_parameters  # noqa: E402


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
    ap.add_argument("--backbone", choices=["resnet50", "yolov1"], default="resnet50")
    ap.add_argument("--batch-size", type=int, default=64, help="per process")
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=135)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--optimizer", choices=["adam", "sgd", "lars"], default="adam",
                    help="sgd: the YOLOv1 paper's recipe (SGD with momentum); lars: layer-wise adaptive rate scaling on top of it, for the large "
                         "effective batches of --accum-steps x ranks (yolo.optim.LARS; biases and BatchNorm gamma / beta are neither adapted nor "
                         "decayed).  Use it with --warmup-steps")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd / lars only")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer sgd only")
    ap.add_argument("--lars-eta", type=float, default=1e-3, help="--optimizer lars only: the trust coefficient")
    ap.add_argument("--warmup-steps", type=int, default=0,
                    help="linear learning-rate warm-up: optimizer step k of the run (from 0) runs at (k + 1) / N of the scheduled rate while k < N; "
                         "--resume continues it.  Default 0: none")
    ap.add_argument("--lr-decay-epochs", default="75,105")
    ap.add_argument("--lambda-coord", type=float, default=5.0)
    ap.add_argument("--lambda-noobj", type=float, default=0.5)
    ap.add_argument("--save-frequency", type=int, default=10)
    ap.add_argument("--freeze-backbone", action="store_true")
    ap.add_argument("--no-pretrained", action="store_true", help="random-init ResNet50 (no torchvision / ImageNet weights available)")
    ap.add_argument("--compute-map", action="store_true")
    ap.add_argument("--checkpoint-dir", default="checkpoints")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images (no dataset needed)")
    ap.add_argument("--device-augment", action="store_true",
                    help="VOC only: loaders ship decoded uint8 images + sampled parameters, crop / resize / colour jitter / normalise run on the device")
    ap.add_argument("--augment", choices=["reference", "darknet"], default="reference",
                    help="VOC only, the training augmentation: reference = RandomResizedCrop + ColorJitter; darknet = the YOLOv1 paper's recipe (scaling "
                         "and translation by up to 20 %% past the image border, horizontal flip, exposure and saturation up to x1.5 and hue +-0.1 in "
                         "HSV); with and without --device-augment")
    ap.add_argument("--voc-root", default=None, help="dataset root (default: $VOC_ROOT or ./data)")
    ap.add_argument("--deterministic", action="store_true",
                    help="EngineConfig.DETERMINISTIC: every order-dependent sum of the training step runs order-fixed (bit-reproducible steps and --resume)")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay (e.g. 0.9999): it is what gets validated, and every "
                         "checkpoint carries it as ema_state_dict (evaluate.py / predict.py --use-ema).  Default: no EMA")
    ap.add_argument("--ema-tau", type=float, default=0.0, help="warm-up of --ema-decay: decay * (1 - exp(-updates / tau)); 0: none")
    ap.add_argument("--accum-steps", type=int, default=1,
                    help="gradient accumulation: K batches per optimizer step and per all-reduce -- effective batch = batch-size x K x world; a last "
                         "group of an epoch with fewer than K batches is dropped.  Default 1: none")
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
    ap.add_argument("--seed", type=int, default=None, help="seed of torch, numpy, random and the loaders (every epoch starts from (seed, epoch))")
    ap.add_argument("--batch-norm", action="store_true",
                    help="--backbone yolov1 only: " "Conv2d(bias=False) + BatchNorm2d + LeakyReLU(0.1) in place of Conv2d + LeakyReLU(0.1) on every convolution of the YOLOv1 network (Darknet's "
                         "batch_normalize=1): trains from the default initialisation.  Recorded in the checkpoint; --resume and --backbone-weights check it")
    ap.add_argument("--factored-fc", action="store_true",
                    help="EngineConfig.FC_FACTORED: the weight gradient of a Linear layer with at least FC_FACTORED_MIN weights (the Linear(50176, 4096) behind "
                         "nn.Flatten) is never stored: the update kernel of --optimizer adam / sgd rebuilds it from its two batch factors, and several ranks "
                         "all-gather 7 MB of factors instead of all-reducing 822 MB.  Not with --optimizer lars, --accum-steps > 1 or --device cpu")
    a = ap.parse_args()
    if a.batch_norm and a.backbone != "yolov1":
        ap.error("--batch-norm needs --backbone yolov1 (the ResNet-50 trunk has its BatchNorm layers already)")
    if a.batch_norm and a.deterministic:
        from yolo.bn_executor import BN_LRELU_NOT_DETERMINISTIC
        ap.error("--deterministic --batch-norm: " + BN_LRELU_NOT_DETERMINISTIC)
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
    if a.augment != "reference" and a.synthetic:
        ap.error("--augment needs the VOC datasets (synthetic samples are not augmented)")
    if a.backbone_weights and a.backbone != "yolov1":
        ap.error("--backbone-weights needs --backbone yolov1 (a classification checkpoint of pretrain.py holds that trunk)")
    if a.deterministic:
        if a.backbone == "resnet50":
            # (the training loop puts the whole model in train(): there is no eval-mode trunk to ask for here)
            from yolo.models import BN_STATS_NOT_DETERMINISTIC
            ap.error(BN_STATS_NOT_DETERMINISTIC)
        from yolo.config import CONFIG
        CONFIG.DETERMINISTIC = True
        if a.seed is None:
            a.seed = 0
    gen, worker_init = None, None
    if a.seed is not None:
        from yolo.training.trainer import seed_epoch
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
    sampler = DistributedSampler(train_ds, num_replicas=world, rank=rank) if world > 1 else None
    train_loader = DataLoader(train_ds, batch_size=a.batch_size, shuffle=sampler is None, sampler=sampler, num_workers=a.num_workers,
                              pin_memory=device == "cuda", drop_last=True, collate_fn=collate, generator=gen, worker_init_fn=worker_init)
    val_loader = DataLoader(val_ds, batch_size=a.batch_size, shuffle=False, num_workers=a.num_workers, pin_memory=device == "cuda", collate_fn=collate,
                            worker_init_fn=worker_init)

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
    if world > 1:
        broadcast_parameters(model)
    criterion = YOLOLoss(S=7, B=2, C=20, lambda_coord=a.lambda_coord, lambda_noobj=a.lambda_noobj)
    params = [p for p in model.parameters() if p.requires_grad]
    if device == "cuda":
        from yolo.optim import LARS, SGD, Adam, lars_param_groups     # fused clip(10) + Adam / SGD with momentum / LARS on the HIP kernels
        if a.optimizer == "lars":
            optimizer = LARS(lars_param_groups(model, a.weight_decay), lr=a.lr, momentum=a.momentum, eta=a.lars_eta, max_grad_norm=10.0)
        elif a.optimizer == "sgd":
            optimizer = SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov, max_grad_norm=10.0)
        else:
            optimizer = Adam(params, lr=a.lr, weight_decay=a.weight_decay, max_grad_norm=10.0)
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
    elif a.optimizer == "lars":                        # torch has none: the same class, whose CPU parameters take stock torch ops
        from yolo.optim import LARS, lars_param_groups
        optimizer = LARS(lars_param_groups(model, a.weight_decay), lr=a.lr, momentum=a.momentum, eta=a.lars_eta, max_grad_norm=10.0)
    elif a.optimizer == "sgd":
        optimizer = torch.optim.SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov)
    else:
        optimizer = torch.optim.Adam(params, lr=a.lr, weight_decay=a.weight_decay)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(e) for e in a.lr_decay_epochs.split(",")], gamma=0.1)

    start_epoch, best_val, best_map = 1, None, None
    if a.resume:
        ck = torch.load(a.resume, map_location=device, weights_only=True)
        if bool(ck.get("batch_norm", False)) != a.batch_norm:
            ap.error(f"--resume {a.resume} records batch_norm={bool(ck.get('batch_norm', False))}, this run has batch_norm={a.batch_norm} "
                     "(--batch-norm): the two must agree")
        model.load_state_dict(ck["model_state_dict"])
        optimizer.load_state_dict(ck["optimizer_state_dict"])
        if "scheduler_state_dict" in ck:
            scheduler.load_state_dict(ck["scheduler_state_dict"])
        start_epoch = ck["epoch"] + 1
        a.init = ck.get("init", "default")          # --resume wins over --init: the weights are the file's, and so is the record of how they began
        best_val, best_map = ck.get("val_loss"), ck.get("mAP50:95")
    ema = None
    if a.ema_decay is not None:
        from yolo.optim import ModelEMA
        ema = ModelEMA(model, decay=a.ema_decay, tau=a.ema_tau, optimizer=optimizer if device == "cuda" else None)
        if a.resume and "ema_state_dict" in ck:      # (a file without one: the average starts from the resumed weights, copied just above)
            ema.load_state_dict({"module": ck["ema_state_dict"], "updates": ck.get("ema_updates", 0), "decay": a.ema_decay, "tau": a.ema_tau})

    ckdir = Path(a.checkpoint_dir)
    if rank == 0:
        ckdir.mkdir(parents=True, exist_ok=True)
    record = {"seed": a.seed, "deterministic": bool(a.deterministic)} if a.seed is not None else None
    extra = {}
    if a.accum_steps > 1:          # (1: the call, and the checkpoint's keys, are those of a run without the option)
        record = {**(record or {}), "accum_steps": a.accum_steps}
        extra["accum_steps"] = a.accum_steps
    if a.augment != "reference":          # (the default: the checkpoint's keys are those of a run without the option)
        record = {**(record or {}), "augment": a.augment}
    if a.init != "default":               # (likewise)
        record = {**(record or {}), "init": a.init}
    if a.batch_norm:                      # (likewise)
        record = {**(record or {}), "batch_norm": True}
    if a.warmup_steps:                    # (0: the call is that of a run without the option)
        extra["warmup_steps"] = a.warmup_steps
    res = training.train(model, train_loader, val_loader, criterion, optimizer, scheduler, device, a.epochs, ckdir,
                         save_frequency=a.save_frequency, compute_map=a.compute_map, start_epoch=start_epoch,
                         best_val_loss_init=best_val, best_map_init=best_map, seed=a.seed, record=record, ema=ema, **extra)
    if rank == 0:
        print("done:", res)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
