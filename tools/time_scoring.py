#!/usr/bin/env python3
"""Post-processing time per batch of mAPMetric.update for scoring="argmax" and scoring="all" ("Class-specific
scores"): the device stage alone (decode, NMS, ground-truth decode, TP / FP matching and the device->host copies, ended by a
synchronise) and the whole update() with its host-side list building.  The two modes alternate inside one process; the
medians and the spread of the repeats are printed as one JSON line.  Needs a GPU (no fallback).

    python tools/time_scoring.py [--batches 16 64] [--repeats 9] [--iters 20] [--conf-threshold 0.01]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v1_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def inputs(n: int, seed: int):
    """network-like predictions: noise everywhere, the object cells close to the targets (so that NMS and matching have work)"""
    import synth
    rng = np.random.Generator(np.random.PCG64([seed, n]))
    tgt = synth.synth_targets(n, seed=seed)
    pred = rng.uniform(0, 0.35, size=(n, 7, 7, 30)).astype(np.float32)
    obj = tgt[..., 4] > 0
    k = int(obj.sum())
    pred[obj, :5] = tgt[obj, :5] + rng.normal(0, 0.03, size=(k, 5)).astype(np.float32)
    pred[obj, 5:10] = tgt[obj, :5] + rng.normal(0, 0.08, size=(k, 5)).astype(np.float32)
    pred[obj, 10:] = tgt[obj, 10:] * 0.9 + 0.05
    return torch.from_numpy(pred).cuda(), torch.from_numpy(tgt).cuda()


def device_stage(pred, tgt, scoring: str, conf: float):
    """what update() does on the device and over the bus, nothing of its host lists; returns the bytes copied to the host"""
    from yolo import ops
    S, B, C = 7, 2, 20
    N, M = pred.shape[0], S * S * B
    thr = [0.5 + 0.05 * i for i in range(10)]
    if scoring == "all":
        rec, counts = ops.decode_classes(pred, conf, S, B, C)
        rec_g, cnt_g = rec.view(N * C, M, 6), counts.view(N * C)
        keep, kc = ops.nms(rec_g, cnt_g, 0.4, 1)
        grec, gcnt = ops.decode_gt(tgt, S, B, C)
        tp, bucket = ops.map_match(rec_g, keep, kc, grec.repeat_interleave(C, 0), gcnt.repeat_interleave(C), thr, 0.5, (32 / 448) ** 2, (96 / 448) ** 2)
    else:
        rec, counts = ops.decode(pred, conf, S, B, C)
        keep, kc = ops.nms(rec, counts, 0.4, 1)
        grec, gcnt = ops.decode_gt(tgt, S, B, C)
        tp, bucket = ops.map_match(rec, keep, kc, grec, gcnt, thr, 0.5, (32 / 448) ** 2, (96 / 448) ** 2)
    host = [t.cpu() for t in (rec, counts, keep, kc, grec, gcnt, tp, bucket)]
    torch.cuda.synchronize()
    return sum(t.numel() * t.element_size() for t in host), int(kc.sum())


def whole_update(pred, tgt, scoring: str, conf: float):
    from yolo import mAPMetric
    m = mAPMetric(20, conf_threshold=conf, scoring=scoring)
    m.update(pred, tgt)
    torch.cuda.synchronize()
    assert m._dev_images == pred.shape[0]
    return sum(len(p) for p in m.all_predictions)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conf-threshold", type=float, default=0.01)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_scoring.py measures on a GPU"
    out = {"device": torch.cuda.get_device_name(0), "conf_threshold": a.conf_threshold, "iters": a.iters, "repeats": a.repeats}
    for n in a.batches:
        pred, tgt = inputs(n, 7)
        row = {}
        for fn in (device_stage, whole_update):
            times = {"argmax": [], "all": []}
            info = {}
            for s in times:                          # warm-up: code objects, allocator
                for _ in range(3):
                    info[s] = fn(pred, tgt, s, a.conf_threshold)
            for _ in range(a.repeats):
                for s in times:                      # the modes alternate
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        fn(pred, tgt, s, a.conf_threshold)
                    times[s].append((time.perf_counter() - t0) / a.iters * 1e3)
            row[fn.__name__] = {s: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                    "info": info[s]} for s, v in times.items()}
        out[f"batch_{n}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
