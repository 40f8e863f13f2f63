#!/usr/bin/env python3
"""Post-processing time per batch of the two evaluation protocols ("VOC devkit evaluation"), on the input of
tools/time_scoring.py and with its repeat scheme: mAPMetric.update(scoring="all") -- the grid protocol -- beside
VOCMetric.update under scoring "all" and "argmax".  Per leg the device stage alone (the launches, the device->host copies, ended by
a synchronise) and the whole update() with its host-side bookkeeping.  The legs alternate inside one process; medians and the
spread of the repeats are printed as one JSON line.  Needs a GPU (no fallback).

    python tools/time_voc_eval.py [--batches 16 64] [--repeats 9] [--iters 20] [--conf-threshold 0.01]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import time_scoring as TS  # noqa: E402  (puts the package and tests/golden on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

S, B, C, SIZE = 7, 2, 20, 448
LEGS = ("grid_all", "voc_all", "voc_argmax")


def ground_truth(tgt: torch.Tensor):
    """the objects of the grid targets as an annotation table: pixel corners on SIZE x SIZE images, nothing difficult"""
    from yolo import _post_cpu
    from yolo.voc_eval import VOCGroundTruth
    images = []
    for n, t in enumerate(tgt.cpu().numpy()):
        g = _post_cpu.decode_gt(t, S, B)
        x, y, w, h = g[:, 1], g[:, 2], g[:, 3], g[:, 4]
        images.append({"image_id": str(n), "width": SIZE, "height": SIZE, "class_ids": g[:, 0].astype(np.int64), "difficult": np.zeros(len(g), bool),
                       "boxes": np.stack([(x - w / 2) * SIZE, (y - h / 2) * SIZE, (x + w / 2) * SIZE, (y + h / 2) * SIZE], 1)})
    return VOCGroundTruth.from_images(images)


def voc_device_stage(pred, gt, scoring: str, conf: float, state: dict):
    """what VOCMetric.update does on the device and over the bus; returns the bytes copied to the host and the rows"""
    from yolo import ops
    N, M = pred.shape[0], S * S * B
    if scoring == "all":
        rec, counts = ops.decode_classes(pred, conf, S, B, C)
        rec, counts, per_image = rec.view(N * C, M, 6), counts.view(N * C), C
    else:
        rec, counts = ops.decode(pred, conf, S, B, C)
        per_image = 1
    keep, kc = ops.nms(rec, counts, 0.4, 1)
    st = state["staging"] = ops.voc_match(rec, keep, kc, per_image, gt.boxes, gt.cls, gt.difficult, gt.offsets, gt.wh, 0, [0.5], state.get("staging"))
    n = int(st.total.item())
    host = [t[:n].cpu() for t in (st.score, st.cls_img, st.status, st.box)]
    torch.cuda.synchronize()
    return 4 + sum(t.numel() * t.element_size() for t in host), n


def voc_whole_update(pred, gt, scoring: str, conf: float, state: dict):
    from yolo.voc_eval import VOCMetric
    m = state.get("metric")
    if m is None:
        m = state["metric"] = VOCMetric(C, gt, scoring=scoring, conf_threshold=conf)
    m.reset()                                  # the staging buffers stay, as they do from batch to batch of an evaluation
    m.update(pred, 0)
    torch.cuda.synchronize()
    assert m._staging is not None
    return sum(len(s) for s in m._score)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conf-threshold", type=float, default=0.01)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_voc_eval.py measures on a GPU"
    out = {"device": torch.cuda.get_device_name(0), "conf_threshold": a.conf_threshold, "iters": a.iters, "repeats": a.repeats}
    for n in a.batches:
        pred, tgt = TS.inputs(n, 7)
        gt = ground_truth(tgt)
        row = {}
        for stage in ("device_stage", "whole_update"):
            states = {leg: {} for leg in LEGS}
            fns = {
                "grid_all": (lambda: TS.device_stage(pred, tgt, "all", a.conf_threshold)) if stage == "device_stage"
                else (lambda: TS.whole_update(pred, tgt, "all", a.conf_threshold)),
                "voc_all": lambda: (voc_device_stage if stage == "device_stage" else voc_whole_update)(pred, gt, "all", a.conf_threshold, states["voc_all"]),
                "voc_argmax": lambda: (voc_device_stage if stage == "device_stage" else voc_whole_update)(pred, gt, "argmax", a.conf_threshold,
                                                                                                          states["voc_argmax"]),
            }
            times = {leg: [] for leg in LEGS}
            info = {}
            for leg in LEGS:                          # warm-up: code objects, allocator
                for _ in range(3):
                    info[leg] = fns[leg]()
            for _ in range(a.repeats):
                for leg in LEGS:                      # the legs alternate
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        fns[leg]()
                    times[leg].append((time.perf_counter() - t0) / a.iters * 1e3)
            row[stage] = {leg: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "info": info[leg]}
                          for leg, v in times.items()}
        out[f"batch_{n}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
