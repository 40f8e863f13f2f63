#!/usr/bin/env python3
"""micro-benchmark: images/s of yolo_augment_u8 for a batch of 64 VOC-sized images (sampled crops, all three colour operations) into the stem's
NHWC4 buffer, next to images/s of the host path (_Augment.apply + ToTensor + Normalize on Pillow) on the same images with 1 and 16 worker
processes.  Warm-up, then REPS timed runs of each; median and spread (min .. max) are printed.
--recipe darknet: the same images with parameters from _DarknetAugment.sample (windows past the image border, flips, the HSV operation).
--device-only: skip the host path."""
import argparse, os, statistics, sys, time
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))
import numpy as np
import torch
from PIL import Image
from yolo.augment import collate_u8
from yolo.dataset import RECIPES
from yolo.inference import _Preprocess

N, REPS = 64, 7
SIZES = [(375, 500), (500, 375), (333, 500), (500, 333), (281, 500), (374, 500), (500, 400), (442, 500)]      # (H, W) common in PASCAL VOC


def make(recipe):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    aug = RECIPES[recipe]((448, 448))
    images = [rng.integers(0, 256, size=SIZES[i % len(SIZES)] + (3,), dtype=np.uint8) for i in range(N)]
    return images, [aug.sample(im.shape[1], im.shape[0]) for im in images]


def host_one(job):
    im, p, recipe = job
    torch.set_num_threads(1)
    return _Preprocess()(RECIPES[recipe]((448, 448)).apply(Image.fromarray(im), [], p)[0]).shape[0]


def spread(rates):
    return f"{statistics.median(rates):9.0f} img/s (min {min(rates):.0f} .. max {max(rates):.0f}, {len(rates)} runs)"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--recipe", choices=sorted(RECIPES), default="reference")
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    images, params = make(a.recipe)
    jobs = [(im, p, a.recipe) for im, p in zip(images, params)]
    print(f"recipe {a.recipe}")
    for workers in (() if a.device_only else (1, 16)):
        with Pool(workers) as pool:
            pool.map(host_one, jobs)          # warm-up: imports, Pillow's tables
            rates = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                pool.map(host_one, jobs * 2, chunksize=max(1, 2 * N // (4 * workers)))
                rates.append(2 * N / (time.perf_counter() - t0))
        print(f"host {RECIPES[a.recipe].__name__} + _finish, {workers:2d} worker process(es): {spread(rates)}")
    if not torch.cuda.is_available():
        sys.exit("no GPU: the device path is not measured")
    from yolo.engine import Act
    batch = collate_u8([(torch.from_numpy(im), p, torch.zeros(1)) for im, p, _ in jobs], pin_memory=True)[0]
    dev = batch.to("cuda")
    act = Act(N, 448, 448, 4, 3, dev.device)
    for _ in range(5):
        dev.into_act(act)
    torch.cuda.synchronize()
    rates, inner = [], 50
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            dev.into_act(act)
        e1.record()
        torch.cuda.synchronize()
        rates.append(inner * N / (e0.elapsed_time(e1) / 1e3))
    print(f"yolo_augment_u8 -> NHWC4 bf16, batch {N}:              {spread(rates)}  = {N / statistics.median(rates) * 1e3:.3f} ms per batch")
    rates = []
    for _ in range(REPS):                     # with the host->device copy of the pinned uint8 batch and the descriptor upload
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            batch.to("cuda", non_blocking=True).into_act(act)
        torch.cuda.synchronize()
        rates.append(10 * N / (time.perf_counter() - t0))
    print(f"  + copy of the uint8 batch ({batch.data.numel() / 1e6:.1f} MB) and descriptors:   {spread(rates)}")
