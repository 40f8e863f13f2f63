#!/usr/bin/env python3
"""mAP evaluation of a checkpoint (the reference's src/evaluate.py surface; defaults batch 16,
conf 0.01, nms 0.4 as in src/evaluate.py:18-95) with an additive --backbone / --synthetic flag."""

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
    a = ap.parse_args()
    ck = torch.load(a.checkpoint, map_location=a.device, weights_only=True) if a.checkpoint else None
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
    res = evaluate_model(model, loader, a.device, num_classes=20, conf_threshold=a.conf_threshold, nms_threshold=a.nms_threshold,
                         scoring=a.scoring)
    lines = [f"{k}: {float(v):.6f}" for k, v in res.items()]
    if a.scoring != "argmax":
        lines.append(f"scoring: {a.scoring}")
    print("\n".join(lines[:12]))
    with open(a.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
