"""PASCAL VOC devkit evaluation (not in the reference; DESIGN.md, "VOC devkit evaluation").

``mAPMetric`` takes its ground truth from the S x S target tensor -- one object per cell -- measures IoU on normalised boxes and
knows no ``difficult`` flag.  This module evaluates as the VOC devkit (``VOCevaldet.m`` / ``voc_eval.py``) does: the ground truth
is every annotated object, a detection whose best match is a difficult object is neither a true nor a false positive, difficult
objects are left out of the positive count, overlaps are measured on pixel boxes with the devkit's ``+ 1``, and the AP is the
VOC2007 11-point form or the area form of VOC2010 and later.

On a ROCm tensor ``VOCMetric.update`` is decode (``yolo_decode`` / ``yolo_decode_classes``), NMS (``yolo_nms``) and ONE more
launch, ``yolo_voc_match``, which matches every kept detection against its image's ground truth at all thresholds and compacts the
rows; the host reads the row count (the batch's one synchronisation) and copies exactly that many rows.  Per detection the metric
keeps arrays only -- class, score, image index, status word, pixel corners -- and ``compute`` is one stable argsort per class, the
cumulative sums and the AP in NumPy.  CPU tensors, and a batch beyond the kernel's limits, go through ``_post_cpu.voc_match``.
"""

from __future__ import annotations

import os
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from . import _post_cpu

AP_MODES = ("voc07", "area")
_TINY = float(np.nextafter(0.0, 1.0))          # the smallest positive fp64


class VOCGroundTruth:
    """The annotated objects of a whole split as one ragged table: image n owns rows offsets[n] .. offsets[n+1] - 1."""

    def __init__(self, boxes, cls, difficult, offsets, wh, image_ids):
        self.boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
        self.cls = np.ascontiguousarray(cls, np.int64).reshape(-1)
        self.difficult = np.ascontiguousarray(difficult, bool).reshape(-1)
        self.offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        self.wh = np.ascontiguousarray(wh, np.float64).reshape(-1, 2)
        self.image_ids = [str(i) for i in image_ids]
        n = len(self.image_ids)
        if len(self.offsets) != n + 1 or len(self.wh) != n or self.offsets[0] != 0 or np.any(np.diff(self.offsets) < 0) \
                or not (len(self.boxes) == len(self.cls) == len(self.difficult) == self.offsets[-1]):
            raise ValueError("VOCGroundTruth: offsets / wh / image_ids / rows do not describe one table")

    def __len__(self) -> int:
        return len(self.image_ids)

    @classmethod
    def from_images(cls, images: Sequence[dict]) -> "VOCGroundTruth":
        """``images``: one ``ground_truth`` dict per image (yolo/dataset.py), in the split's order."""
        counts = [len(g["class_ids"]) for g in images]
        cat = lambda key, dtype, shape: np.concatenate([np.zeros(0, dtype).reshape(shape)]                     # noqa: E731
                                                       + [np.asarray(g[key], dtype).reshape(shape) for g in images])
        return cls(cat("boxes", np.float64, (-1, 4)), cat("class_ids", np.int64, (-1,)), cat("difficult", bool, (-1,)),
                   np.concatenate(([0], np.cumsum(counts))), [[g["width"], g["height"]] for g in images], [g["image_id"] for g in images])

    @classmethod
    def from_dataset(cls, ds) -> "VOCGroundTruth":
        return cls.from_images([ds.ground_truth(i) for i in range(len(ds))])


def average_precision(tp: np.ndarray, fp: np.ndarray, npos: int, ap_mode: str) -> float:
    """AP of one class from the 0/1 vectors of its detections in descending score (an ignored detection is 0 in both)."""
    ctp, cfp = np.cumsum(tp, dtype=np.float64), np.cumsum(fp, dtype=np.float64)
    rec = ctp / npos
    prec = ctp / np.maximum(ctp + cfp, _TINY)
    if ap_mode == "voc07":
        ap = 0.0
        for k in range(11):                       # the devkit's np.arange(0, 1.1, 0.1)
            sel = rec >= k * 0.1
            ap = ap + (float(prec[sel].max()) if sel.any() else 0.0) / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


class VOCMetric:
    """PASCAL VOC devkit AP over the annotated ground truth of a split (module docstring)."""

    def __init__(self, num_classes: int, ground_truth: VOCGroundTruth, iou_thresholds=(0.5,), ap_mode: str = "voc07", scoring: str = "all",
                 conf_threshold: float = 0.01, nms_threshold: float = 0.4, S: int = 7, B: int = 2, class_names: Sequence[str] = None):
        if ap_mode not in AP_MODES:
            raise ValueError(f"ap_mode must be one of {AP_MODES}, got {ap_mode!r}")
        self.num_classes, self.gt, self.ap_mode = num_classes, ground_truth, ap_mode
        self.iou_thresholds = [float(iou_thresholds)] if isinstance(iou_thresholds, (int, float)) else [float(t) for t in iou_thresholds]
        if not self.iou_thresholds:
            raise ValueError("VOCMetric needs at least one IoU threshold")
        self.scoring = _post_cpu.check_scoring(scoring)
        self.conf_threshold, self.nms_threshold, self.S, self.B = conf_threshold, nms_threshold, S, B
        if class_names is None:
            from .dataset import VOC_CLASSES
            class_names = VOC_CLASSES if num_classes == len(VOC_CLASSES) else [str(c) for c in range(num_classes)]
        self.class_names = list(class_names)
        self._staging = None
        self.reset()

    def reset(self):
        self._score: List[np.ndarray] = []
        self._cls: List[np.ndarray] = []
        self._img: List[np.ndarray] = []
        self._status: List[np.ndarray] = []
        self._box: List[np.ndarray] = []
        self._seen = np.zeros(len(self.gt), bool)

    # ------------------------------------------------------------------ accumulation
    def _append(self, score, cls, img, status, box):
        self._score.append(np.asarray(score, np.float64))
        self._cls.append(np.asarray(cls, np.int32))
        self._img.append(np.asarray(img, np.int32))
        self._status.append(np.asarray(status, np.uint32))
        self._box.append(np.asarray(box, np.float64).reshape(-1, 4))

    def _fits_kernel(self, M: int, first: int, N: int) -> bool:
        from . import ops
        most = int(np.diff(self.gt.offsets[first: first + N + 1]).max()) if N else 0
        return len(self.iou_thresholds) <= ops.VOC_MAX_THRESHOLDS and M <= ops.VOC_MAX_PER_GROUP and most <= ops.VOC_MAX_GT

    def update(self, predictions: torch.Tensor, first_index: int):
        """predictions (batch, S, S, 5B+C): the network's output for samples first_index, first_index + 1, ... of the split."""
        N = predictions.shape[0]
        if first_index < 0 or first_index + N > len(self.gt):
            raise IndexError(f"samples {first_index} .. {first_index + N - 1} are not in a ground truth of {len(self.gt)} images")
        self._seen[first_index: first_index + N] = True
        if N == 0:
            return
        C = predictions.shape[-1] - 5 * self.B
        M = self.S * self.S * self.B
        if predictions.is_cuda and self._fits_kernel(M, first_index, N):
            return self._update_device(predictions, first_index, N, C, M)
        # host: CPU tensors, and device batches beyond the kernel's limits (decode and NMS still run where the tensor lives)
        if predictions.is_cuda:
            from . import ops
            per_img = [r[k] for r, k in ops.postprocess_host(predictions, self.conf_threshold, self.nms_threshold, ops._hip.NMS_METRICS, self.S, self.B, C,
                                                             self.scoring)]
        else:
            per_img = []
            for i in range(N):
                p = predictions[i].detach().numpy()
                if self.scoring == "all":
                    rec, keep = _post_cpu.nms_classes(_post_cpu.decode_classes(p, self.conf_threshold, self.S, self.B), self.nms_threshold, _post_cpu.METRICS)
                else:
                    rec = _post_cpu.decode(p, self.conf_threshold, self.S, self.B)
                    keep = _post_cpu.nms(rec, self.nms_threshold, _post_cpu.METRICS)
                per_img.append(rec[keep])
        for i, kept in enumerate(per_img):
            n = first_index + i
            a, b = self.gt.offsets[n], self.gt.offsets[n + 1]
            status, box = _post_cpu.voc_match(kept, self.gt.wh[n, 0], self.gt.wh[n, 1], self.gt.boxes[a:b], self.gt.cls[a:b], self.gt.difficult[a:b],
                                              self.iou_thresholds)
            self._append(kept[:, 1], kept[:, 0], np.full(len(kept), n), status, box)

    def _update_device(self, predictions, first: int, N: int, C: int, M: int):
        from . import ops
        if self.scoring == "all":
            rec, counts = ops.decode_classes(predictions, self.conf_threshold, self.S, self.B, C)
            rec, counts, per_image = rec.view(N * C, M, 6), counts.view(N * C), C
        else:
            rec, counts = ops.decode(predictions, self.conf_threshold, self.S, self.B, C)
            per_image = 1
        keep, kc = ops.nms(rec, counts, self.nms_threshold, ops._hip.NMS_METRICS)
        a, b = self.gt.offsets[first], self.gt.offsets[first + N]
        st = self._staging = ops.voc_match(rec, keep, kc, per_image, self.gt.boxes[a:b], self.gt.cls[a:b], self.gt.difficult[a:b],
                                           self.gt.offsets[first: first + N + 1] - a, self.gt.wh[first: first + N], first, self.iou_thresholds,
                                           self._staging)
        n = int(st.total.item())                          # 4 bytes: the batch's one synchronisation
        ci = st.cls_img[:n].cpu().numpy()
        self._append(st.score[:n].cpu().numpy(), ci[:, 0], ci[:, 1], st.status[:n].cpu().numpy().view(np.uint32), st.box[:n].cpu().numpy())

    # ------------------------------------------------------------------ results
    def _arrays(self):
        cat = lambda parts, dtype, tail: np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)   # noqa: E731
        return (cat(self._score, np.float64, ()), cat(self._cls, np.int32, ()), cat(self._img, np.int32, ()), cat(self._status, np.uint32, ()),
                cat(self._box, np.float64, (4,)))

    def compute(self) -> Dict[str, float]:
        """mAP, AP_class_<c>, npos_class_<c>, num_detections, num_ignored at the first threshold; with several thresholds also mAP@<t>."""
        score, cls, _img, status, _box = self._arrays()
        seen_rows = np.repeat(self._seen, np.diff(self.gt.offsets))
        counted = seen_rows & ~self.gt.difficult
        npos = [int(np.count_nonzero(counted & (self.gt.cls == c))) for c in range(self.num_classes)]
        order = []
        for c in range(self.num_classes):
            idx = np.nonzero(cls == c)[0]
            order.append(idx[np.argsort(-score[idx], kind="stable")])    # ties keep image order, then list order
        per_thr = []
        for ti in range(len(self.iou_thresholds)):
            aps = []
            for c in range(self.num_classes):
                if npos[c] == 0:
                    aps.append(float("nan"))
                    continue
                st = (status[order[c]] >> np.uint32(2 * ti)) & np.uint32(3)
                aps.append(average_precision(st == _post_cpu.VOC_TP, st == _post_cpu.VOC_FP, npos[c], self.ap_mode))
            per_thr.append(aps)
        mean = lambda aps: float(np.mean([a for a in aps if not np.isnan(a)])) if any(not np.isnan(a) for a in aps) else float("nan")  # noqa: E731
        out: Dict[str, float] = {"mAP": mean(per_thr[0])}
        if len(self.iou_thresholds) > 1:
            for t, aps in zip(self.iou_thresholds, per_thr):
                out[f"mAP@{t:g}"] = mean(aps)
        for c in range(self.num_classes):
            out[f"AP_class_{c}"] = per_thr[0][c]
        for c in range(self.num_classes):
            out[f"npos_class_{c}"] = npos[c]
        out["num_detections"] = int(len(score))
        out["num_ignored"] = int(np.count_nonzero((status & np.uint32(3)) == _post_cpu.VOC_IGNORED))
        return out

    def write_detections(self, directory: str, prefix: str = "comp4_det_test_") -> List[str]:
        """The devkit's / the evaluation server's detection files: ``<prefix><class name>.txt``, one line
        ``image_id score xmin ymin xmax ymax`` per detection, corners 1-based (Darknet's print_yolo_detections: + 1 on all four)."""
        score, cls, img, _status, box = self._arrays()
        os.makedirs(directory, exist_ok=True)
        paths = []
        for c in range(self.num_classes):
            path = os.path.join(directory, f"{prefix}{self.class_names[c]}.txt")
            idx = np.nonzero(cls == c)[0]
            with open(path, "w") as f:
                f.write("".join("%s %f %f %f %f %f\n" % (self.gt.image_ids[i], s, x1 + 1, y1 + 1, x2 + 1, y2 + 1)
                                for i, s, (x1, y1, x2, y2) in zip(img[idx].tolist(), score[idx].tolist(), box[idx].tolist())))
            paths.append(path)
        return paths


class _Indexed(torch.utils.data.Dataset):
    """(image, index) samples of a detection dataset: the loop needs to know which images a batch holds, not their grid targets"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, idx):
        return self.ds[idx][0], idx


def evaluate_voc(model: nn.Module, dataset, device: str, num_classes: int = 20, iou_thresholds=(0.5,), ap_mode: str = "voc07", scoring: str = "all",
                 conf_threshold: float = 0.01, nms_threshold: float = 0.4, S: int = 7, B: int = 2, batch_size: int = 16, num_workers: int = 4,
                 write_detections: str = None, ground_truth: VOCGroundTruth = None) -> Dict[str, float]:
    """Run ``model`` over ``dataset`` (unshuffled) and return ``VOCMetric.compute()``; ``write_detections``: a directory for the devkit's files."""
    model.eval()
    gt = ground_truth if ground_truth is not None else VOCGroundTruth.from_dataset(dataset)
    metric = VOCMetric(num_classes, gt, iou_thresholds=iou_thresholds, ap_mode=ap_mode, scoring=scoring, conf_threshold=conf_threshold,
                       nms_threshold=nms_threshold, S=S, B=B, class_names=getattr(dataset, "class_names", None))
    loader = DataLoader(_Indexed(dataset), batch_size=batch_size, shuffle=False, num_workers=num_workers)
    with torch.no_grad():
        for images, idx in loader:
            first = int(idx[0])
            assert idx.tolist() == list(range(first, first + len(idx))), "evaluate_voc needs the split in order"
            metric.update(model(images.to(device)), first)
    if write_detections:
        metric.write_detections(write_detections)
    return metric.compute()
