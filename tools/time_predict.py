#!/usr/bin/env python3
"""Images per second of the prediction surface ("Batched detection") on a folder of synthetic JPEGs in VOC-like mixed
sizes, written here with PIL from a seed:
  (a) the YOLOInference.predict(path) loop,
  (b) predict_batch from the files at batch 16 and 64 (decode threads + device),
  (c) predict_batch from the same images decoded beforehand (device and result assembly alone),
  (d) predict_batch_arrays, which builds no Detection objects, and the host stages on their own (decoding, packing, the objects),
and, per batch of 64 random predictions at conf 0.01, ops.detect_host against ops.postprocess_host (+ classes_to_images, which it
calls under scoring "all") with the per-image record slices both leave to their caller -- the host clock around calls that end in a
device->host copy -- and the device time of the three launches of ops.detect between two events.  Warm-up first; the legs alternate
inside one process; medians and the spread of the repeats go out as one JSON line.  Needs a GPU (no fallback).

    python tools/time_predict.py [--images 1024] [--repeats 5] [--workers 4] [--folder DIR]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "yolo-v1_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

S, B, C = 7, 2, 20
SIZES = [(500, 375), (375, 500), (480, 360), (333, 500), (500, 333), (500, 400), (354, 500), (500, 281)]      # (W, H)


def write_folder(folder: str, n: int) -> list:
    """n JPEGs of smooth noise (a photograph's compression ratio, roughly), sizes in turn"""
    rng = np.random.RandomState(0)
    paths = []
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        coarse = rng.randint(0, 256, (h // 16 + 1, w // 16 + 1, 3)).astype(np.uint8)
        paths.append(os.path.join(folder, f"{i:05d}.jpg"))
        Image.fromarray(coarse).resize((w, h), Image.BICUBIC).save(paths[-1], quality=90)
    return paths


def detector():
    """the default YOLOv1, random weights, a last bias that lets most cells of every image report an object (a few dozen detections
    an image at conf 0.5, so that result assembly is part of what is timed)"""
    from yolo import YOLOv1
    from yolo.inference import YOLOInference
    torch.manual_seed(0)
    model = YOLOv1()
    bias = np.zeros((S, S, 5 * B + C), np.float32)
    cell = np.arange(S * S).reshape(S, S)
    bias[..., 0:2] = bias[..., 5:7] = 0.5
    bias[..., 2:4], bias[..., 7:9] = 0.25, 0.2
    bias[..., 4] = 0.6 + 0.35 * cell / (S * S - 1)
    bias[..., 9] = bias[..., 4] - 0.05
    np.put_along_axis(bias[..., 10:], (cell % C)[..., None], 0.8, -1)
    with torch.no_grad():
        model.head[4].bias.copy_(torch.from_numpy(bias.reshape(-1)))
    return YOLOInference(model.cuda().eval(), device="cuda")


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(values, scale=1.0, digits=1):
    v = [x * scale for x in values]
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def time_legs(legs: dict, repeats: int) -> dict:
    times = {k: [] for k in legs}
    for fn in legs.values():                      # warm-up: code objects, plans of every batch size, allocator, page cache
        fn()
    for _ in range(repeats):
        for k, fn in legs.items():                # the legs alternate
            times[k].append(wall(fn))
    return times


def postprocess_legs(repeats: int, iters: int, conf: float) -> dict:
    from yolo import ops
    pred = torch.rand((64, S, S, 5 * B + C), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    wh = np.array([SIZES[n % len(SIZES)] for n in range(64)], np.float64)
    out = {}
    for scoring in ("argmax", "all"):
        def old():
            return [rec[keep] for rec, keep in ops.postprocess_host(pred, conf, 0.4, ops._hip.NMS_INFERENCE, S, B, C, scoring)]

        def new():
            det, _, off = ops.detect_host(pred, conf, 0.4, S, B, C, scoring)
            return [det[off[n]: off[n + 1]] for n in range(64)]

        def new_pixels():
            det, _, off = ops.detect_host(pred, conf, 0.4, S, B, C, scoring, wh)
            return [det[off[n]: off[n + 1]] for n in range(64)]

        a, b = old(), new()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the two paths must agree before they are compared"
        legs = {"postprocess_host": old, "detect_host": new, "detect_host_pixels": new_pixels}
        t = time_legs({k: (lambda f=f: [f() for _ in range(iters)]) for k, f in legs.items()}, repeats)
        row = {k: summary(v, 1e3 / iters, 4) for k, v in t.items()}
        ev = []
        for _ in range(repeats):                  # device time of decode + NMS + finish, between two events
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                ops.detect(pred, conf, 0.4, S, B, C, scoring, wh)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1) / iters)
        row["detect_device_ms"] = summary(ev, 1.0, 4)
        row["rows"] = int(sum(len(x) for x in b))
        row["bytes_to_host"] = {"postprocess_host": 64 * (C if scoring == "all" else 1) * (S * S * B * (48 + 4) + 8),
                                "detect_host": row["rows"] * 48 + 65 * 4}
        out[scoring] = {"ms_per_batch": row}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window of the post-processing legs")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--conf-threshold", type=float, default=0.01, help="of the post-processing legs; the image legs use predict's default 0.5")
    ap.add_argument("--folder", default=None, help="where the JPEGs go (default: a temporary directory)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_predict.py measures on a GPU"
    with tempfile.TemporaryDirectory() as tmp:
        folder = a.folder or tmp
        os.makedirs(folder, exist_ok=True)
        paths = write_folder(folder, a.images)
        engine = detector()
        arrays = [np.asarray(engine.load_image(p)) for p in paths]
        from yolo.augment import U8Batch
        pinned = torch.empty(max(sum(x.size for x in arrays[i: i + 64]) for i in range(0, len(arrays), 64)), dtype=torch.uint8, pin_memory=True)
        _, cls, score, _, _, xywh = engine.predict_batch_arrays(arrays, batch_size=64, workers=a.workers, normalized=True)
        records = np.concatenate([cls[:, None].astype(np.float64), score[:, None], xywh], 1)
        found = {}
        legs = {
            "a_predict_loop": lambda: found.__setitem__("a", sum(len(engine.predict(p)) for p in paths)),
            "b_files_batch16": lambda: found.__setitem__("b16", sum(map(len, engine.predict_batch(paths, batch_size=16, workers=a.workers)))),
            "b_files_batch64": lambda: found.__setitem__("b64", sum(map(len, engine.predict_batch(paths, batch_size=64, workers=a.workers)))),
            "c_arrays_batch16": lambda: found.__setitem__("c16", sum(map(len, engine.predict_batch(arrays, batch_size=16, workers=a.workers)))),
            "c_arrays_batch64": lambda: found.__setitem__("c64", sum(map(len, engine.predict_batch(arrays, batch_size=64, workers=a.workers)))),
            "d_files_to_arrays_batch64": lambda: engine.predict_batch_arrays(paths, batch_size=64, workers=a.workers),
            "d_arrays_to_arrays_batch64": lambda: engine.predict_batch_arrays(arrays, batch_size=64, workers=a.workers),
            # host stages on their own: decoding, packing a batch into one buffer, one Detection object per row
            "decode_only_pool": lambda: engine._loaded(paths, a.workers),
            "decode_only_one_thread": lambda: [engine.load_image(p) for p in paths],
            "pack_only_batch64": lambda: [U8Batch.from_images(arrays[i: i + 64], buffer=pinned) for i in range(0, len(arrays), 64)],
            "detection_objects_only": lambda: engine._records_to_detections(records, None),
        }
        t = time_legs(legs, a.repeats)
    out = {"device": torch.cuda.get_device_name(0), "images": a.images, "workers": a.workers, "repeats": a.repeats, "detections": found,
           "images_per_s": {k: summary([a.images / x for x in v]) for k, v in t.items()},
           "postprocess_batch64": dict(postprocess_legs(a.repeats, a.iters, a.conf_threshold), conf_threshold=a.conf_threshold)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
