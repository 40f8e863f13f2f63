"""Host (numpy, float64) decode / IoU / NMS used when the tensors live on the CPU.

This is the reference's ``--device cpu`` behaviour for post-processing (Python-float arithmetic on
fp32 values widened by ``.item()``: src/yolo/inference.py:170-317, src/yolo/metrics.py:185-341),
written array-wise.  It is selected by the tensor's device, never as a substitute for a missing HIP
library: device tensors always go through yolo_decode / yolo_nms (postprocess.hip).
"""

from __future__ import annotations

import numpy as np

INFERENCE, METRICS = 0, 1


def decode(pred: np.ndarray, conf_thr: float, S: int, B: int) -> np.ndarray:
    """(S,S,5B+C) fp32 -> (n,6) float64 rows [class_id, conf*prob, x, y, w, h] in (i,j,b) scan order."""
    p = np.asarray(pred, dtype=np.float32).reshape(S, S, -1)
    cls = p[..., B * 5:].argmax(-1)                              # first maximum, like torch.argmax
    prob = np.take_along_axis(p[..., B * 5:], cls[..., None], -1)[..., 0].astype(np.float64)
    boxes = p[..., : B * 5].reshape(S, S, B, 5).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    rec = np.empty((S, S, B, 6), np.float64)
    rec[..., 0] = cls[..., None]
    rec[..., 1] = boxes[..., 4] * prob[..., None]
    rec[..., 2] = (jj[..., None] + boxes[..., 0]) / S
    rec[..., 3] = (ii[..., None] + boxes[..., 1]) / S
    rec[..., 4] = boxes[..., 2]
    rec[..., 5] = boxes[..., 3]
    rec = rec.reshape(-1, 6)
    return rec[rec[:, 1] > conf_thr]


def decode_gt(tgt: np.ndarray, S: int, B: int) -> np.ndarray:
    """(S,S,5B+C) fp32 -> (n,5) float64 rows [class_id, x, y, w, h]; a cell holds an object iff conf0 > 0."""
    t = np.asarray(tgt, dtype=np.float32).reshape(S, S, -1)
    jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    rec = np.empty((S, S, 5), np.float64)
    rec[..., 0] = t[..., B * 5:].argmax(-1)
    rec[..., 1] = (jj + t[..., 0].astype(np.float64)) / S
    rec[..., 2] = (ii + t[..., 1].astype(np.float64)) / S
    rec[..., 3] = t[..., 2]
    rec[..., 4] = t[..., 3]
    return rec[t[..., 4] > 0]


def iou_one_to_many(a: np.ndarray, b: np.ndarray, variant: int) -> np.ndarray:
    """IoU of box a (4,) against boxes b (m,4), centre format, float64, a is the first argument."""
    ax1, ay1, ax2, ay2 = a[0] - a[2] / 2, a[1] - a[3] / 2, a[0] + a[2] / 2, a[1] + a[3] / 2
    bx1, by1 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2
    bx2, by2 = b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    dw = np.where(bx2 < ax2, bx2, ax2) - np.where(bx1 > ax1, bx1, ax1)
    dh = np.where(by2 < ay2, by2, ay2) - np.where(by1 > ay1, by1, ay1)
    inter = np.where(dw > 0, dw, 0.0) * np.where(dh > 0, dh, 0.0)
    a1, a2 = a[2] * a[3], b[:, 2] * b[:, 3]
    if variant == INFERENCE:
        return inter / (a1 + a2 - inter + 1e-6)
    union = a1 + a2 - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union == 0, 0.0, inter / np.where(union == 0, 1.0, union))


def iou_scalar(a, b, variant: int) -> float:
    return float(iou_one_to_many(np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(1, 4), variant)[0])


def nms(rec: np.ndarray, thr: float, variant: int) -> np.ndarray:
    """Greedy NMS over (n,6) records -> kept indices in the reference's output order
    (variant INFERENCE: confidence order; METRICS: grouped by class in first-appearance order)."""
    n = len(rec)
    if n == 0:
        return np.zeros(0, np.int32)
    order = np.argsort(-rec[:, 1], kind="stable")            # ties keep scan order
    cls, box = rec[order, 0], rec[order, 2:6]
    alive = np.ones(n, bool)
    kept = []
    for a in range(n):
        if not alive[a]:
            continue
        kept.append(a)
        later = np.nonzero(alive[a + 1:] & (cls[a + 1:] == cls[a]))[0] + a + 1
        if len(later):
            alive[later[~(iou_one_to_many(box[a], box[later], variant) < thr)]] = False
    kept = np.asarray(kept, np.int64)
    if variant == METRICS:
        first = {}
        for pos, c in enumerate(cls):
            first.setdefault(c, pos)
        kept = kept[np.argsort([first[cls[k]] for k in kept], kind="stable")]
    return order[kept].astype(np.int32)


# ------------------------------------------------------------------------------------------------
# class-specific scoring (YOLOv1 paper section 2; Darknet get_detection_boxes + do_nms_sort): every box is a candidate of
# every class with score conf_b * prob_c; each class is thresholded and NMS-filtered on its own
# ------------------------------------------------------------------------------------------------
SCORINGS = ("argmax", "all")


def check_scoring(scoring: str) -> str:
    if scoring not in SCORINGS:
        raise ValueError(f"scoring must be one of {SCORINGS}, got {scoring!r}")
    return scoring


def decode_classes(pred: np.ndarray, conf_thr: float, S: int, B: int) -> list:
    """(S,S,5B+C) fp32 -> C arrays (n_c,6) float64 of rows [c, conf_b*prob_c, x, y, w, h], each in (i,j,b) scan order."""
    p = np.asarray(pred, dtype=np.float32).reshape(S, S, -1)
    C = p.shape[-1] - B * 5
    probs = p[..., B * 5:].astype(np.float64)                     # (S,S,C)
    boxes = p[..., : B * 5].reshape(S, S, B, 5).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    rec = np.empty((S, S, B, 6), np.float64)
    rec[..., 2] = (jj[..., None] + boxes[..., 0]) / S
    rec[..., 3] = (ii[..., None] + boxes[..., 1]) / S
    rec[..., 4] = boxes[..., 2]
    rec[..., 5] = boxes[..., 3]
    out = []
    for c in range(C):
        rec[..., 0] = c
        rec[..., 1] = boxes[..., 4] * probs[..., c, None]
        r = rec.reshape(-1, 6)
        out.append(r[r[:, 1] > conf_thr])                          # boolean indexing copies
    return out


def nms_classes(groups: list, thr: float, variant: int):
    """Per-class NMS over the lists of ``decode_classes`` -> (rec, keep) of one image: ``rec`` is the groups one behind the
    other (class ascending, scan order), ``keep`` indexes it in the result order.  METRICS: classes ascending, inside a
    class the NMS output (confidence) order.  INFERENCE: all kept detections by confidence descending, stable over that."""
    rec = np.concatenate(groups) if len(groups) else np.zeros((0, 6))
    keep, off = [], 0
    for g in groups:
        keep.append(nms(g, thr, variant).astype(np.int64) + off)
        off += len(g)
    keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    if variant == INFERENCE:
        keep = keep[np.argsort(-rec[keep, 1], kind="stable")]
    return rec.reshape(-1, 6), keep.astype(np.int32)


# ------------------------------------------------------------------------------------------------
# PASCAL VOC devkit matching ("VOC devkit evaluation"): what yolo_voc_match does on the device, array-wise per
# (image, class) group -- the same float64 operations in the same order
# ------------------------------------------------------------------------------------------------
VOC_FP, VOC_TP, VOC_IGNORED = 0, 1, 2


def voc_pixel_boxes(xywh: np.ndarray, W: float, H: float) -> np.ndarray:
    """(n,4) normalised centre boxes -> (n,4) pixel corners of a W x H image, clamped to it."""
    x, y, w, h = (np.asarray(xywh, np.float64).reshape(-1, 4)[:, k] for k in range(4))
    W, H = np.float64(W), np.float64(H)
    out = np.stack([(x - w / 2) * W, (y - h / 2) * H, (x + w / 2) * W, (y + h / 2) * H], 1)
    for col, lim in ((0, W), (1, H), (2, W), (3, H)):
        v = out[:, col]
        v[v < 0] = 0.0
        v[v > lim] = lim
    return out


def voc_match(kept: np.ndarray, W: float, H: float, gt_box: np.ndarray, gt_cls: np.ndarray, gt_difficult: np.ndarray, thresholds):
    """One image.  ``kept`` (n,6): its kept records in metrics-NMS order (inside a class: score-descending).  Returns the status
    words (n,) uint32 -- 2 bits per threshold: 0 FP, 1 TP, 2 ignored -- and the clamped pixel boxes (n,4)."""
    kept = np.asarray(kept, np.float64).reshape(-1, 6)
    box = voc_pixel_boxes(kept[:, 2:6], W, H)
    status = np.zeros(len(kept), np.uint32)
    thr = np.asarray(thresholds, np.float64)
    shifts = (2 * np.arange(len(thr))).astype(np.uint32)
    dcls = kept[:, 0].astype(np.int64)
    for c in np.unique(dcls):
        gi = np.nonzero(gt_cls == c)[0]
        if len(gi) == 0:
            continue                                                      # no candidate: FP at every threshold
        di = np.nonzero(dcls == c)[0]
        d, g, dif = box[di], gt_box[gi], gt_difficult[gi]
        iw = np.where(g[None, :, 2] < d[:, None, 2], g[None, :, 2], d[:, None, 2]) - np.where(g[None, :, 0] > d[:, None, 0], g[None, :, 0], d[:, None, 0]) + 1
        ih = np.where(g[None, :, 3] < d[:, None, 3], g[None, :, 3], d[:, None, 3]) - np.where(g[None, :, 1] > d[:, None, 1], g[None, :, 1], d[:, None, 1]) + 1
        darea = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)
        garea = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
        inter = iw * ih
        part = (iw > 0) & (ih > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ov = np.where(part, inter / (darea[:, None] + garea[None, :] - inter), -np.inf)
        jmax = ov.argmax(1)                                               # first of the largest
        ovmax = ov[np.arange(len(di)), jmax]
        taken = np.zeros((len(gi), len(thr)), bool)
        for k in range(len(di)):                                          # the greedy walk, all thresholds at once
            j = jmax[k]
            hit = ovmax[k] >= thr
            if dif[j]:
                st = np.where(hit, VOC_IGNORED, VOC_FP)
            else:
                tp = hit & ~taken[j]
                taken[j] |= tp
                st = np.where(tp, VOC_TP, VOC_FP)
            status[di[k]] = np.bitwise_or.reduce(st.astype(np.uint32) << shifts)
    return status, box
