"""What train.py and pretrain.py share around their ``main()``: the common options and their checks, seeding, the process group, the loaders,
the optimizer and scheduler, ``--resume``, the EMA and the checkpoint record.  Each script keeps its datasets and model, its own options, the
plan it attaches to the optimizer and its final ``train(...)`` call.  (No dataset module and no torchvision is imported here.)"""

from __future__ import annotations

import os
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from .loop import seed_epoch


def add_common_arguments(ap, optimizer: str, lr: float, epochs: int, lr_decay_epochs: str, checkpoint_dir: str) -> None:
    """the options both scripts take; the arguments are the defaults in which they differ"""
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--batch-size", type=int, default=64, help="per process")
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=epochs)
    ap.add_argument("--lr", type=float, default=lr)
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--optimizer", choices=["adam", "sgd", "lars"], default=optimizer,
                    help="sgd: the YOLOv1 paper's recipe (SGD with momentum); lars: layer-wise adaptive rate scaling on top of it, for the large "
                         "effective batches of --accum-steps x ranks (yolo.optim.LARS; biases and BatchNorm gamma / beta are neither adapted nor "
                         "decayed).  Use it with --warmup-steps")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd / lars only")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer sgd only")
    ap.add_argument("--lars-eta", type=float, default=1e-3, help="--optimizer lars only: the trust coefficient")
    ap.add_argument("--warmup-steps", type=int, default=0,
                    help="linear learning-rate warm-up: optimizer step k of the run (from 0) runs at (k + 1) / N of the scheduled rate while k < N; "
                         "--resume continues it.  Default 0: none")
    ap.add_argument("--lr-decay-epochs", default=lr_decay_epochs)
    ap.add_argument("--save-frequency", type=int, default=10)
    ap.add_argument("--checkpoint-dir", default=checkpoint_dir)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--seed", type=int, default=None, help="seed of torch, numpy, random and the loaders (every epoch starts from (seed, epoch))")
    ap.add_argument("--deterministic", action="store_true",
                    help="EngineConfig.DETERMINISTIC: every order-dependent sum of the training step runs order-fixed (bit-reproducible steps and --resume)")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay (e.g. 0.9999): it is what gets validated, and every "
                         "checkpoint carries it as ema_state_dict (evaluate.py / predict.py --use-ema, train.py --backbone-weights .. --use-ema).  "
                         "Default: no EMA")
    ap.add_argument("--ema-tau", type=float, default=0.0, help="warm-up of --ema-decay: decay * (1 - exp(-updates / tau)); 0: none")
    ap.add_argument("--accum-steps", type=int, default=1,
                    help="gradient accumulation: K batches per optimizer step and per all-reduce -- effective batch = batch-size x K x world; a last "
                         "group of an epoch with fewer than K batches is dropped.  Default 1: none")
    ap.add_argument("--batch-norm", action="store_true",
                    help="Conv2d(bias=False) + BatchNorm2d + LeakyReLU(0.1) in place of Conv2d + LeakyReLU(0.1) on every convolution of the YOLOv1 network "
                         "(Darknet's batch_normalize=1; train.py: --backbone yolov1 only): trains from the default initialisation.  Recorded in the "
                         "checkpoint; --resume and --backbone-weights check it")
    ap.add_argument("--factored-fc", action="store_true",
                    help="EngineConfig.FC_FACTORED: the weight gradient of a Linear layer with at least FC_FACTORED_MIN weights (the Linear(50176, 4096) behind "
                         "nn.Flatten) is never stored: the update kernel of --optimizer adam / sgd rebuilds it from its two batch factors, and several ranks "
                         "all-gather 7 MB of factors instead of all-reducing 822 MB.  Not with --optimizer lars, --accum-steps > 1 or --device cpu")


def _seed_worker(worker_id: int) -> None:
    """DataLoader worker: numpy and ``random`` from the seed torch derived for this worker from the loader's generator"""
    import random

    import numpy as np
    s = torch.initial_seed() % (1 << 31)
    np.random.seed(s)
    random.seed(s)


def begin(ap, a):
    """the common checks of the parsed options ``a`` (the script has made its own), then in this order: EngineConfig.FC_FACTORED and
    DETERMINISTIC, the seeding (in front of the model's construction: parameter initialisation), the process group
    -> namespace(device, world, rank, gen, worker_init), ``gen`` / ``worker_init`` being the loaders' generator and worker seeding (None unseeded)"""
    if a.batch_norm and a.deterministic:
        from ..bn_executor import BN_LRELU_NOT_DETERMINISTIC
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
    if a.optimizer == "lars" and a.nesterov:
        ap.error("--optimizer lars has no Nesterov momentum (--nesterov is --optimizer sgd only)")
    if a.warmup_steps < 0:
        ap.error("--warmup-steps must not be negative")
    from ..config import CONFIG
    if a.factored_fc:
        CONFIG.FC_FACTORED = True
    if a.deterministic:
        CONFIG.DETERMINISTIC = True
        if a.seed is None:
            a.seed = 0
    run = SimpleNamespace(device=a.device, world=int(os.environ.get("WORLD_SIZE", "1")), rank=int(os.environ.get("RANK", "0")), gen=None, worker_init=None)
    if a.seed is not None:
        seed_epoch(a.seed, 0)                 # parameter initialisation
        run.gen = torch.Generator()
        run.gen.manual_seed(a.seed)
        run.worker_init = _seed_worker
    if run.world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if run.device == "cuda":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl" if run.device == "cuda" else "gloo")
    return run


def make_loaders(a, run, train_ds, val_ds, collate, drop_last):
    """(train loader, validation loader); several ranks shard the training set.  ``drop_last``: a bool, or a function of the samples per rank"""
    sampler = DistributedSampler(train_ds, num_replicas=run.world, rank=run.rank) if run.world > 1 else None
    if callable(drop_last):
        drop_last = drop_last(len(train_ds) if sampler is None else len(sampler))
    pin = run.device == "cuda"
    train_loader = DataLoader(train_ds, batch_size=a.batch_size, shuffle=sampler is None, sampler=sampler, num_workers=a.num_workers, pin_memory=pin,
                              drop_last=drop_last, collate_fn=collate, generator=run.gen, worker_init_fn=run.worker_init)
    val_loader = DataLoader(val_ds, batch_size=a.batch_size, shuffle=False, num_workers=a.num_workers, pin_memory=pin, collate_fn=collate,
                            worker_init_fn=run.worker_init)
    return train_loader, val_loader


def make_optimizer(a, run, model):
    """the optimizer of ``--optimizer``.  On a device: fused clip(10) + Adam / SGD with momentum / LARS on the HIP kernels (the script attaches
    its plan); on the CPU torch's own Adam and SGD, and for lars -- torch has none -- the same class, whose CPU parameters take stock torch ops"""
    from ..optim import LARS, SGD, Adam, lars_param_groups
    params = [p for p in model.parameters() if p.requires_grad]
    if a.optimizer == "lars":
        return LARS(lars_param_groups(model, a.weight_decay), lr=a.lr, momentum=a.momentum, eta=a.lars_eta, max_grad_norm=10.0)
    if run.device == "cuda":
        if a.optimizer == "sgd":
            return SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov, max_grad_norm=10.0)
        return Adam(params, lr=a.lr, weight_decay=a.weight_decay, max_grad_norm=10.0)
    if a.optimizer == "sgd":
        return torch.optim.SGD(params, lr=a.lr, momentum=a.momentum, weight_decay=a.weight_decay, nesterov=a.nesterov)
    return torch.optim.Adam(params, lr=a.lr, weight_decay=a.weight_decay)


def make_scheduler(a, optimizer):
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(e) for e in a.lr_decay_epochs.split(",")], gamma=0.1)


def load_resume(ap, a, run):
    """the checkpoint of ``--resume`` (None without), its ``batch_norm`` record checked against this run's"""
    if not a.resume:
        return None
    ck = torch.load(a.resume, map_location=run.device, weights_only=True)
    if bool(ck.get("batch_norm", False)) != a.batch_norm:
        ap.error(f"--resume {a.resume} records batch_norm={bool(ck.get('batch_norm', False))}, this run has batch_norm={a.batch_norm} "
                 "(--batch-norm): the two must agree")
    return ck


def resume(a, ck, model, optimizer, scheduler) -> int:
    """model, optimizer and scheduler state from ``ck`` (``load_resume``) -> the epoch to start at (1 without a checkpoint)"""
    if ck is None:
        return 1
    model.load_state_dict(ck["model_state_dict"])
    optimizer.load_state_dict(ck["optimizer_state_dict"])
    if "scheduler_state_dict" in ck:
        scheduler.load_state_dict(ck["scheduler_state_dict"])
    a.init = ck.get("init", "default")          # --resume wins over --init: the weights are the file's, and so is the record of how they began
    return ck["epoch"] + 1


def make_ema(a, run, ck, model, optimizer):
    """the ``ModelEMA`` of ``--ema-decay`` (None without), continued from ``ck`` where it holds one (a file without one: the average starts
    from the resumed weights, which ``resume`` has just loaded)"""
    if a.ema_decay is None:
        return None
    from ..optim import ModelEMA
    ema = ModelEMA(model, decay=a.ema_decay, tau=a.ema_tau, optimizer=optimizer if run.device == "cuda" else None)
    if ck is not None and "ema_state_dict" in ck:
        ema.load_state_dict({"module": ck["ema_state_dict"], "updates": ck.get("ema_updates", 0), "decay": a.ema_decay, "tau": a.ema_tau})
    return ema


def checkpoint_dir(a, run) -> Path:
    ckdir = Path(a.checkpoint_dir)
    if run.rank == 0:
        ckdir.mkdir(parents=True, exist_ok=True)
    return ckdir


def record_and_extra(a, own: dict | None = None):
    """(``record``: the plain entries of the epoch checkpoints, ``own`` first; ``extra``: the keywords of ``train(...)``).  An option left at
    its default adds nothing to either: the call, and the checkpoint's keys, are those of a run without the option"""
    record, extra = dict(own or {}), {}
    if a.seed is not None:
        record.update(seed=a.seed, deterministic=bool(a.deterministic))
    if a.accum_steps > 1:
        record["accum_steps"] = extra["accum_steps"] = a.accum_steps
    if a.init != "default":
        record["init"] = a.init
    if a.batch_norm:
        record["batch_norm"] = True
    if a.warmup_steps:
        extra["warmup_steps"] = a.warmup_steps
    return record or None, extra


def finish(run, res) -> None:
    if run.rank == 0:
        print("done:", res)
    if run.world > 1:
        dist.destroy_process_group()
