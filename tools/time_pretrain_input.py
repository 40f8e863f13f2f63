#!/usr/bin/env python3
"""images/s of pretrain.py's epoch loop (yolo.training.classify.train_epoch) with the input path on the host and on the device.

    python tools/time_pretrain_input.py --data-root /tmp/folders --make 1024            # once: JPEG files from a seed, then exit
    python tools/time_pretrain_input.py --data-root /tmp/folders [--device-augment] [--pkg OTHER/yolo-v1_amd] [--json out.json]

One process is one configuration: YOLOv1Classifier with the fused SGD of pretrain.py, the loader as pretrain.py builds it (shuffle, pinned memory,
`--workers` worker processes, with --device-augment the uint8 collate), `--epochs` passes over the image folder.  A pass is timed from the
moment batch `--skip` is handed out (the workers have started and delivered their first round) to a device synchronise behind the last step --
the host clock around work that ends in a synchronise.  Decoding stays in the workers either way; what --device-augment moves to the device is
crop, resize, colour jitter, flip, ToTensor and Normalize.

The loader's workers deliver in rounds of `--workers` batches, so a pass should hold many rounds: `--repeat R` lists every file R times
(1024 files x 9 = 144 batches of 64 = 9 rounds of 16).  To compare two trees (the parent commit's host path against this one's), start the
configurations alternately, each in its own process: `--pkg` names the package directory to import.  Needs the GPU: there is no fallback."""
import argparse, functools, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--data-root", required=True)
ap.add_argument("--make", type=int, default=0, help="write this many JPEG files (8 classes, ~500 x 375, both orientations) under <data-root>/train and exit")
ap.add_argument("--pkg", default=None, help="the yolo-v1_amd directory to import (default: this tree's)")
ap.add_argument("--device-augment", action="store_true")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--workers", type=int, default=16)
ap.add_argument("--epochs", type=int, default=2)
ap.add_argument("--skip", type=int, default=16)
ap.add_argument("--repeat", type=int, default=9)
ap.add_argument("--tag", default=None)
ap.add_argument("--json", default=None, help="append the result line there")
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make_one(job):
    import numpy as np
    from PIL import Image
    path, seed = job
    rng = np.random.Generator(np.random.PCG64([5, seed]))
    h, w = (375, 500) if seed % 3 else (500, 375)
    h, w = h + int(rng.integers(-40, 41)), w + int(rng.integers(-40, 41))
    # a photograph's statistics, roughly: smooth structure at a few scales plus mild noise (what the JPEG decoder's time depends on)
    img = np.zeros((h, w, 3), np.float32)
    for cells in (4, 16, 64):
        coarse = rng.uniform(0, 255, (cells, cells, 3)).astype(np.float32)
        img += np.asarray(Image.fromarray(coarse.astype(np.uint8)).resize((w, h), Image.BICUBIC), np.float32) / 3
    img += rng.normal(0, 6, img.shape)
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90)


if a.make:
    from multiprocessing import Pool
    jobs = []
    for i in range(a.make):
        d = os.path.join(a.data_root, "train", f"class{i % 8}")
        os.makedirs(d, exist_ok=True)
        jobs.append((os.path.join(d, f"{i:06d}.jpg"), i))
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        pool.map(_make_one, jobs, chunksize=16)
    print(f"wrote {a.make} files under {a.data_root}/train")
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.pkg) if a.pkg else os.path.join(ROOT, "yolo-v1_amd"))
import torch
from torch.utils.data import DataLoader
from yolo import SoftmaxCrossEntropy, YOLOv1Classifier
from yolo.dataset import ImageFolderClassification
from yolo.optim import SGD
from yolo.training import classify as loop

assert torch.cuda.is_available(), "time_pretrain_input.py measures on the GPU"
torch.manual_seed(0)
ds = ImageFolderClassification(a.data_root, "train", a.size, **({"device_transform": True} if a.device_augment else {}))
ds.samples = ds.samples * a.repeat
collate = None
if a.device_augment:
    from yolo.augment import collate_u8
    collate = functools.partial(collate_u8, size=(a.size, a.size))
loader = DataLoader(ds, batch_size=a.batch, shuffle=True, num_workers=a.workers, pin_memory=True, drop_last=True, collate_fn=collate)
model = YOLOv1Classifier(num_classes=len(ds.classes)).to("cuda")
opt = SGD(model.parameters(), lr=1e-4, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
opt.attach_plan(model.head_plan())
crit = SoftmaxCrossEntropy(0.1)


class Timed:
    """the loader, with the clock started when batch `skip` is handed out"""

    def __init__(self, inner, skip):
        self.inner, self.skip, self.t0 = inner, skip, None

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        for i, b in enumerate(self.inner):
            if i == self.skip:
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
            yield b


assert len(loader) > a.skip, "the pass is shorter than --skip"
rates = []
for epoch in range(1, a.epochs + 1):
    timed = Timed(loader, a.skip)
    loop.train_epoch(model, timed, crit, opt, "cuda", epoch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - timed.t0
    rates.append(round((len(loader) - a.skip) * a.batch / dt, 1))
out = {"tag": a.tag or ("device" if a.device_augment else "host"), "pkg": a.pkg or "this tree", "device_augment": bool(a.device_augment), "batch": a.batch,
       "size": a.size, "workers": a.workers, "batches_timed": len(loader) - a.skip, "images_per_s": rates}
print(json.dumps(out), flush=True)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "a") as f:
        f.write(json.dumps(out) + "\n")
