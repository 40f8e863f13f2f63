#!/usr/bin/env python3
"""mAP evaluation of a checkpoint (the reference's src/evaluate.py surface; defaults batch 16,
conf 0.01, nms 0.4 as in src/evaluate.py:18-95) with an additive --backbone / --synthetic flag and, with --protocol voc,
the PASCAL VOC devkit's evaluation (yolo/voc_eval.py) instead of the reference's."""

from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from yolo import YOLOv1, ResNetBackbone, YOLOv1Backbone, evaluate_model  # noqa: E402
from yolo.dataset import SyntheticYOLODataset, create_voc_datasets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--backbone", choices=["resnet50", "yolov1"], default="resnet50")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--conf-threshold", type=float, default=0.01)
    ap.add_argument("--nms-threshold", type=float, default=0.4)
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--output", default="evaluation_results.txt")
    ap.add_argument("--use-ema", action="store_true", help="evaluate the averaged weights of a train.py --ema-decay checkpoint (ema_state_dict)")
    ap.add_argument("--scoring", choices=["argmax", "all"], default="argmax",
                    help="argmax: one class per cell, the reference's protocol; all: every box scored for every class and NMS per class, "
                         "the paper's / Darknet's test-time protocol")
    ap.add_argument("--batch-norm", action="store_true",
                    help="--backbone yolov1 without a checkpoint: the BatchNorm variant (a checkpoint's own batch_norm record decides otherwise)")
    ap.add_argument("--protocol", choices=["grid", "voc"], default="grid",
                    help="grid: ground truth from the S x S target, the reference's matching; voc: the PASCAL VOC devkit's -- every annotated "
                         "object, difficult flags, pixel overlaps (yolo/voc_eval.py)")
    ap.add_argument("--ap-mode", choices=["voc07", "area"], default="voc07", help="--protocol voc: the 11-point AP of VOC2007 or the area of VOC2010+")
    ap.add_argument("--iou-thresholds", default="0.5", help="--protocol voc: comma-separated IoU thresholds, the first is the one of mAP")
    ap.add_argument("--write-detections", default=None, metavar="DIR", help="--protocol voc: write the devkit's comp4_det_test_<class>.txt files there")
    a = ap.parse_args()
    if a.protocol != "voc" and (a.write_detections or a.ap_mode != "voc07" or a.iou_thresholds != "0.5"):
        ap.error("--ap-mode, --iou-thresholds and --write-detections need --protocol voc")
    ck =torch.load(a.checkpoint, map_location=a.device, weights_only=True) if a.checkpoint else None
    bn = bool(ck.get("batch_norm", False)) if ck is not None else a.batch_norm
    if bn and a.backbone != "yolov1":
        ap.error("batch_norm (the checkpoint's record, or --batch-norm) needs --backbone yolov1")
    ds = SyntheticYOLODataset(a.synthetic, seed=2) if a.synthetic else create_voc_datasets([("2007", "test")], augment=False)
    loader = DataLoader(ds, batch_size=a.batch_size, shuffle=False, num_workers=4)
    bb = (YOLOv1Backbone(batch_norm=True) if bn else YOLOv1Backbone()) if a.backbone == "yolov1" else ResNetBackbone(pretrained=False)
    model = YOLOv1(backbone=bb, num_classes=20)
    if a.checkpoint:
        from yolo.training.checkpoints import weights_of
        model.load_state_dict(weights_of(ck, a.use_ema, a.checkpoint))
    elif a.use_ema:
        ap.error("--use-ema needs --checkpoint")
    model = model.to(a.device)
    if a.protocol == "voc":
        from yolo.voc_eval import evaluate_voc
        res = evaluate_voc(model, ds, a.device, num_classes=20, iou_thresholds=[float(t) for t in a.iou_thresholds.split(",")], ap_mode=a.ap_mode,
                           scoring=a.scoring, conf_threshold=a.conf_threshold, nms_threshold=a.nms_threshold, batch_size=a.batch_size,
                           write_detections=a.write_detections)
    else:
        res = evaluate_model(model, loader, a.device, num_classes=20, conf_threshold=a.conf_threshold, nms_threshold=a.nms_threshold,
                             scoring=a.scoring)
    lines = [f"{k}: {float(v):.6f}" for k, v in res.items()]
    if a.scoring != "argmax":
        lines.append(f"scoring: {a.scoring}")
    if a.protocol == "voc":
        lines += ["protocol: voc", f"ap_mode: {a.ap_mode}"]
    print("\n".join(lines[:12]))
    with open(a.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
