#!/usr/bin/env python3
"""Run detection on image files (the reference's src/predict.py surface + an additive --backbone flag).

    python yolo-v1_amd/predict.py image.jpg --checkpoint checkpoints/yolo_best.pth --device cuda --backbone yolov1
    python yolo-v1_amd/predict.py photos/ --batch-size 64 --json detections.json --checkpoint ... --backbone yolov1
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from yolo import YOLOv1, ResNetBackbone, YOLOv1Backbone  # noqa: E402
from yolo.inference import YOLOInference  # noqa: E402
from yolo.utils import VOC_CLASSES, draw_detections  # noqa: E402


def load_model(checkpoint_path: str | None, device: str, num_classes: int = 20, backbone: str = "resnet50", use_ema: bool = False,
               batch_norm: bool = False) -> YOLOv1:
    """batch_norm: the BatchNorm variant of --backbone yolov1 when there is no checkpoint; a checkpoint's own ``batch_norm`` record decides otherwise"""
    ck = torch.load(checkpoint_path, map_location=device, weights_only=True) if checkpoint_path else None
    if ck is not None:
        batch_norm = bool(ck.get("batch_norm", False))
    if batch_norm and backbone != "yolov1":
        raise SystemExit("batch_norm (the checkpoint's record, or --batch-norm) needs --backbone yolov1")
    bb = (YOLOv1Backbone(batch_norm=True) if batch_norm else YOLOv1Backbone()) if backbone == "yolov1" else ResNetBackbone(pretrained=False)
    model = YOLOv1(backbone=bb, num_classes=num_classes)
    if checkpoint_path:
        from yolo.training.checkpoints import weights_of
        model.load_state_dict(weights_of(ck, use_ema, checkpoint_path))
    elif use_ema:
        raise SystemExit("--use-ema needs --checkpoint")
    return model.eval().to(device)


IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp")


def expand_inputs(inputs) -> list[str]:
    """files stay as they are; a directory stands for its image files (by suffix, any letter case), sorted, not recursively"""
    out = []
    for p in inputs:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p))
                    if f.lower().endswith(IMAGE_SUFFIXES) and os.path.isfile(os.path.join(p, f))]
        else:
            out.append(p)
    return out


def report(engine, path, dets, a) -> None:
    print(f"{path}: {len(dets)} detections")
    for d in dets:
        print(f"  {d.class_name:12s} {d.confidence:.3f} {d.bbox}")
    if a.output_dir:
        os.makedirs(a.output_dir, exist_ok=True)
        draw_detections(engine.load_image(path), dets, VOC_CLASSES, a.conf_threshold).save(os.path.join(a.output_dir, os.path.basename(path)))


def json_entry(path, width, height, cls, score, box) -> dict:
    """one image of --json: pixel boxes {xmin, ymin, xmax, ymax} clamped to the image"""
    return {"image": path, "width": int(width), "height": int(height),
            "detections": [{"class_id": int(c), "class_name": VOC_CLASSES[int(c)], "confidence": float(s), "bbox": [float(v) for v in b]}
                           for c, s, b in zip(cls, score, box)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="+", help="image files, or directories (their *.jpg, *.jpeg, *.png, *.bmp files, sorted, not recursively)")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--backbone", choices=["resnet50", "yolov1"], default="resnet50")
    ap.add_argument("--conf-threshold", type=float, default=0.5)
    ap.add_argument("--nms-threshold", type=float, default=0.4)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("--use-ema", action="store_true", help="load the averaged weights of a train.py --ema-decay checkpoint (ema_state_dict)")
    ap.add_argument("--scoring", choices=["argmax", "all"], default="argmax",
                    help="argmax: one class per cell, the reference's protocol; all: every box scored for every class and NMS per class, "
                         "the paper's / Darknet's test-time protocol")
    ap.add_argument("--batch-norm", action="store_true",
                    help="--backbone yolov1 without a checkpoint: the BatchNorm variant (a checkpoint's own batch_norm record decides otherwise)")
    ap.add_argument("--batch-size", type=int, default=1, help="images per forward pass; above 1 the files are decoded by --workers threads while "
                                                              "the previous batch runs (YOLOInference.predict_batch)")
    ap.add_argument("--workers", type=int, default=4, help="decoder threads of --batch-size > 1 (1 .. 16)")
    ap.add_argument("--json", default=None, metavar="FILE",
                    help="write per image {image, width, height, detections: [{class_id, class_name, confidence, bbox: [xmin, ymin, xmax, ymax]}]}, "
                         "boxes in pixels")
    a = ap.parse_args()
    if a.batch_size < 1:
        ap.error("--batch-size must be at least 1")
    paths = expand_inputs(a.images)
    engine = YOLOInference(load_model(a.checkpoint, a.device, backbone=a.backbone, use_ema=a.use_ema, batch_norm=a.batch_norm), device=a.device)
    entries = []
    if a.batch_size > 1:
        idx, cls, score, box, sizes, xywh = engine.predict_batch_arrays(paths, conf_threshold=a.conf_threshold, nms_threshold=a.nms_threshold,
                                                                         scoring=a.scoring, batch_size=a.batch_size, workers=a.workers,
                                                                         normalized=True)
        first = np.searchsorted(idx, np.arange(len(paths) + 1))
        for i, path in enumerate(paths):
            rows = slice(first[i], first[i + 1])
            rec = np.concatenate([cls[rows, None].astype(np.float64), score[rows, None], xywh[rows]], 1)
            report(engine, path, engine._records_to_detections(rec, VOC_CLASSES), a)
            entries.append(json_entry(path, sizes[i][0], sizes[i][1], cls[rows], score[rows], box[rows]))
    else:
        from yolo._post_cpu import voc_pixel_boxes
        for path in paths:
            dets = engine.predict(path, conf_threshold=a.conf_threshold, nms_threshold=a.nms_threshold, class_names=VOC_CLASSES, scoring=a.scoring)
            report(engine, path, dets, a)
            if a.json:
                w, h = engine.load_image(path).size
                xywh = [[d.bbox.x, d.bbox.y, d.bbox.width, d.bbox.height] for d in dets]
                entries.append(json_entry(path, w, h, [d.class_id for d in dets], [d.confidence for d in dets], voc_pixel_boxes(xywh, w, h)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(entries, f, indent=1)


if __name__ == "__main__":
    main()
