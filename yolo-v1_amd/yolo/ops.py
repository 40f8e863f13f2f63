"""Tensor-level wrappers over the C ABI (include/yolo_hip.h).  Device tensors in, device tensors out;
nothing here synchronises except the explicit ``*_host`` helpers, which do ONE device->host copy
where the reference does hundreds of ``.item()`` syncs (src/yolo/inference.py:184-191,
src/yolo/metrics.py:200-208, src/yolo/loss.py:165-169)."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _hip
from ._hip import check, lib, ptr, stream

# ------------------------------------------------------------------------------------------------
# decode / IoU / NMS
# ------------------------------------------------------------------------------------------------


def _as_f32_dev(t: torch.Tensor) -> torch.Tensor:
    _hip.require_cuda(t)
    return t.detach().to(torch.float32).contiguous()


@_hip.device_guard
def decode(pred: torch.Tensor, conf_thr: float, S: int, B: int, C: int):
    """(N,S,S,5B+C) fp32 -> rec (N,S*S*B,6) f64 {cls,conf,x,y,w,h}, counts (N,) i32.
    Replaces src/yolo/inference.py:170-210 / src/yolo/metrics.py:185-218."""
    pred = _as_f32_dev(pred)
    N = pred.shape[0]
    rec = torch.empty((N, S * S * B, 6), dtype=torch.float64, device=pred.device)
    counts = torch.empty((N,), dtype=torch.int32, device=pred.device)
    check(lib().yolo_decode(ptr(pred), N, S, B, C, float(conf_thr), ptr(rec), ptr(counts), stream()), "yolo_decode")
    return rec, counts


@_hip.device_guard
def decode_classes(pred: torch.Tensor, conf_thr: float, S: int, B: int, C: int):
    """(N,S,S,5B+C) fp32 -> rec (N,C,S*S*B,6) f64 {c,conf_b*prob_c,x,y,w,h}, counts (N,C) i32: every box scored for every
    class (YOLOv1 paper section 2).  ``rec.view(N*C, S*S*B, 6)`` / ``counts.view(N*C)`` are what ``nms`` and ``map_match`` take."""
    pred = _as_f32_dev(pred)
    N = pred.shape[0]
    rec = torch.empty((N, C, S * S * B, 6), dtype=torch.float64, device=pred.device)
    counts = torch.empty((N, C), dtype=torch.int32, device=pred.device)
    check(lib().yolo_decode_classes(ptr(pred), N, S, B, C, float(conf_thr), ptr(rec), ptr(counts), stream()), "yolo_decode_classes")
    return rec, counts


@_hip.device_guard
def decode_gt(tgt: torch.Tensor, S: int, B: int, C: int):
    """(N,S,S,5B+C) fp32 -> rec (N,S*S,5) f64 {cls,x,y,w,h}, counts.  Replaces src/yolo/metrics.py:232-256."""
    tgt = _as_f32_dev(tgt)
    N = tgt.shape[0]
    rec = torch.empty((N, S * S, 5), dtype=torch.float64, device=tgt.device)
    counts = torch.empty((N,), dtype=torch.int32, device=tgt.device)
    check(lib().yolo_decode_gt(ptr(tgt), N, S, B, C, ptr(rec), ptr(counts), stream()), "yolo_decode_gt")
    return rec, counts


@_hip.device_guard
def nms(rec: torch.Tensor, counts: torch.Tensor, thr: float, variant: int):
    """rec (N,M,6) f64 + counts -> keep (N,M) i32 (reference output order), keep_counts (N,).
    Replaces src/yolo/inference.py:298-317 (variant 0) / src/yolo/metrics.py:270-296 (variant 1)."""
    _hip.require_cuda(rec, counts)
    assert rec.dtype == torch.float64 and rec.is_contiguous() and counts.dtype == torch.int32
    N, M, _ = rec.shape
    keep = torch.empty((N, M), dtype=torch.int32, device=rec.device)
    kc = torch.empty((N,), dtype=torch.int32, device=rec.device)
    check(lib().yolo_nms(ptr(rec), ptr(counts), N, M, float(thr), int(variant), ptr(keep), ptr(kc), stream()), "yolo_nms")
    return keep, kc


@_hip.device_guard
def pairwise_iou(a: torch.Tensor, b: torch.Tensor, variant: int) -> torch.Tensor:
    """a (na,4), b (nb,4) f64 (x,y,w,h) -> (na,nb) f64.  src/yolo/inference.py:229-249 / metrics.py:313-341."""
    _hip.require_cuda(a, b)
    a = a.to(torch.float64).contiguous()
    b = b.to(torch.float64).contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    check(lib().yolo_pairwise_iou(ptr(a), a.shape[0], ptr(b), b.shape[0], int(variant), ptr(out), stream()), "yolo_pairwise_iou")
    return out


@_hip.device_guard
def map_match(rec: torch.Tensor, keep: torch.Tensor, kc: torch.Tensor, grec: torch.Tensor, gcnt: torch.Tensor, thresholds, extra_thr: float,
              small_area: float, medium_area: float):
    """TP bits of every kept prediction (see yolo_map_match) + the size bucket of every ground truth, on the device.
    Replaces the matching loops of src/yolo/metrics.py:343-442, 444-491, 568-651."""
    import ctypes
    _hip.require_cuda(rec, keep, kc, grec, gcnt)
    N, M, _ = rec.shape
    G = grec.shape[1]
    tp = torch.zeros((N, M), dtype=torch.int64, device=rec.device)
    bucket = torch.zeros((N, G), dtype=torch.int32, device=rec.device)
    thr = (ctypes.c_double * len(thresholds))(*[float(t) for t in thresholds])
    check(lib().yolo_map_match(ptr(rec), ptr(keep), ptr(kc), N, M, ptr(grec), ptr(gcnt), G, thr, len(thresholds), float(extra_thr), float(small_area),
                               float(medium_area), ptr(tp), ptr(bucket), stream()), "yolo_map_match")
    return tp, bucket


VOC_MAX_THRESHOLDS, VOC_MAX_GT, VOC_MAX_PER_GROUP = 16, 256, 1024      # the limits of yolo_voc_match (include/yolo_hip.h)


class VocStaging:
    """The five output buffers of ``yolo_voc_match`` for the worst case of one batch shape, kept by the caller across batches."""

    def __init__(self, rows: int, device):
        self.rows, self.device = rows, device
        self.score = torch.empty((rows,), dtype=torch.float64, device=device)
        self.cls_img = torch.empty((rows, 2), dtype=torch.int32, device=device)
        self.status = torch.empty((rows,), dtype=torch.int32, device=device)         # the uint32 status words, bit for bit
        self.box = torch.empty((rows, 4), dtype=torch.float64, device=device)
        self.total = torch.empty((1,), dtype=torch.int32, device=device)


@_hip.device_guard
def voc_match(rec: torch.Tensor, keep: torch.Tensor, kc: torch.Tensor, groups_per_image: int, gt_box: np.ndarray, gt_cls: np.ndarray,
              gt_difficult: np.ndarray, gt_off: np.ndarray, img_wh: np.ndarray, image_base: int, thresholds, staging: VocStaging = None):
    """PASCAL VOC devkit matching of the kept detections of ``nms`` (metrics variant) on the device (see yolo_voc_match).
    rec (n_groups, M, 6), keep (n_groups, M), kc (n_groups,) device tensors; the batch's slice of the ground-truth table as
    HOST arrays -- gt_box (G,4) f64 pixel corners, gt_cls (G,), gt_difficult (G,), gt_off (images+1,) starting at 0, img_wh
    (images,2) -- uploaded here in one copy.  Launches without synchronising; returns the staging buffers (``staging`` if it
    is given and large enough), whose ``total`` says how many leading rows are valid."""
    _hip.require_cuda(rec, keep, kc)
    assert rec.dtype == torch.float64 and rec.is_contiguous() and keep.dtype == torch.int32 and keep.is_contiguous() and kc.dtype == torch.int32
    n_groups, M, _ = rec.shape
    gt_off = np.ascontiguousarray(gt_off, np.int32)
    n_img, G = len(gt_off) - 1, int(gt_off[-1])
    if n_img * groups_per_image != n_groups or gt_off[0] != 0 or len(gt_box) != G or len(gt_cls) != G or len(gt_difficult) != G or len(img_wh) != n_img:
        raise RuntimeError(f"voc_match: {n_groups} groups of {groups_per_image} per image do not fit a ground-truth slice of {n_img} images, {G} rows")
    max_gt = int(np.diff(gt_off).max()) if n_img else 0
    # one upload: the f64 parts first, then the int32 parts, then the bytes (every part stays aligned to its type)
    f64 = np.concatenate([np.asarray(gt_box, np.float64).reshape(-1), np.asarray(img_wh, np.float64).reshape(-1)])
    i32 = np.concatenate([np.asarray(gt_cls, np.int32).reshape(-1), gt_off])
    blob = np.concatenate([f64.view(np.uint8), i32.view(np.uint8), np.asarray(gt_difficult, np.uint8).reshape(-1), np.zeros(8, np.uint8)])
    dev = torch.from_numpy(blob).to(rec.device)
    p0 = dev.data_ptr()
    p_box, p_wh = p0, p0 + 32 * G
    p_cls = p0 + 8 * len(f64)
    p_off = p_cls + 4 * G
    p_dif = p_cls + 4 * len(i32)
    if staging is None or staging.rows < n_groups * M or staging.device != rec.device:
        staging = VocStaging(max(n_groups * M, 1), rec.device)
    thr = (ctypes.c_double * len(thresholds))(*[float(t) for t in thresholds])
    vp = ctypes.c_void_p
    check(lib().yolo_voc_match(ptr(rec), ptr(keep), ptr(kc), n_groups, M, int(groups_per_image), vp(p_box), vp(p_cls), vp(p_dif), vp(p_off), vp(p_wh),
                               max_gt, int(image_base), thr, len(thresholds), ptr(staging.score), ptr(staging.cls_img), ptr(staging.status),
                               ptr(staging.box), ptr(staging.total), stream()), "yolo_voc_match")
    staging.upload = dev          # the kernel reads it: it must outlive the launch
    return staging


def classes_to_images(rec_h, counts_h, keep_h, kc_h, variant: int, extra=None):
    """Host arrays of ``decode_classes`` + grouped ``nms`` -> per image (rec, keep) like ``_post_cpu.nms_classes``: the valid rows
    of the image's C groups one behind the other, and the kept indices into them in the result order of ``variant``.
    ``extra`` (N,C,M), e.g. the TP bits of ``map_match``: its kept entries in that order come third."""
    N, C, M, _ = rec_h.shape
    slot = np.arange(M)
    out = []
    for n in range(N):
        valid = slot[None, :] < counts_h[n][:, None]                       # (C,M), row-major == class ascending, scan order
        kvalid = slot[None, :] < kc_h[n][:, None]
        off = np.concatenate(([0], np.cumsum(counts_h[n][:-1]))).astype(np.int64)
        rec = rec_h[n][valid]
        keep = (keep_h[n].astype(np.int64) + off[:, None])[kvalid]
        ex = None if extra is None else extra[n][kvalid]
        if variant == _hip.NMS_INFERENCE:
            order = np.argsort(-rec[keep, 1], kind="stable")
            keep = keep[order]
            ex = None if ex is None else ex[order]
        out.append((rec, keep.astype(np.int32)) if extra is None else (rec, keep.astype(np.int32), ex))
    return out


def postprocess_host(pred: torch.Tensor, conf_thr: float, nms_thr: float, variant: int, S: int, B: int, C: int, scoring: str = "argmax"):
    """decode + NMS on the device for a batch, ONE device->host copy.
    Returns per image (rec[n] as a (cnt,6) float64 numpy array, kept indices int32 numpy array).
    scoring="all": class-specific scores, NMS per (image, class) group by the same ``yolo_nms``; rec[n] holds the image's
    C groups one behind the other."""
    from ._post_cpu import check_scoring
    if check_scoring(scoring) == "all":
        rec, counts = decode_classes(pred, conf_thr, S, B, C)
        N = rec.shape[0]
        keep, kc = nms(rec.view(N * C, S * S * B, 6), counts.view(N * C), nms_thr, variant)
        return classes_to_images(rec.cpu().numpy(), counts.cpu().numpy(), keep.view(N, C, -1).cpu().numpy(), kc.view(N, C).cpu().numpy(), variant)
    rec, counts = decode(pred, conf_thr, S, B, C)
    keep, kc = nms(rec, counts, nms_thr, variant)
    rec_h, counts_h, keep_h, kc_h = rec.cpu().numpy(), counts.cpu().numpy(), keep.cpu().numpy(), kc.cpu().numpy()
    return [(rec_h[n, : counts_h[n]], keep_h[n, : kc_h[n]]) for n in range(rec_h.shape[0])]


def _groups(pred: torch.Tensor, conf_thr: float, nms_thr: float, variant: int, S: int, B: int, C: int, scoring: str):
    """decode + NMS of a batch as ``yolo_voc_match`` / ``yolo_detect_finish`` take them: rec (n_groups, M, 6), keep (n_groups, M),
    keep counts (n_groups,), groups per image (C under scoring "all", else 1)"""
    from ._post_cpu import check_scoring
    if check_scoring(scoring) == "all":
        rec, counts = decode_classes(pred, conf_thr, S, B, C)
        rec, counts, gpi = rec.view(-1, S * S * B, 6), counts.view(-1), C
    else:
        (rec, counts), gpi = decode(pred, conf_thr, S, B, C), 1
    keep, kc = nms(rec, counts, nms_thr, variant)
    return rec, keep, kc, gpi


@_hip.device_guard
def detect_finish(rec: torch.Tensor, keep: torch.Tensor, kc: torch.Tensor, groups_per_image: int, img_wh=None):
    """The kept detections of ``nms`` (inference variant) as dense per-image lists in result order (see yolo_detect_finish).
    ``img_wh`` (images, 2) {W, H}, array or tensor: pixel corners clamped to the image; None: the records' x, y, w, h.
    Returns device tensors det (rows, 6) f64, image (rows,) i32, off (images + 1,) i32 sized for the worst case: the first
    ``off[-1]`` rows are valid, the rest is not written."""
    _hip.require_cuda(rec, keep, kc)
    assert rec.dtype == torch.float64 and rec.is_contiguous() and keep.dtype == torch.int32 and keep.is_contiguous() and kc.dtype == torch.int32
    n_groups, M, _ = rec.shape
    if groups_per_image < 1 or n_groups % groups_per_image:
        raise RuntimeError(f"detect_finish: {n_groups} groups are not a multiple of {groups_per_image} per image")
    n_img = n_groups // groups_per_image
    if img_wh is not None:
        img_wh = torch.as_tensor(img_wh, dtype=torch.float64).to(rec.device).contiguous()
        if tuple(img_wh.shape) != (n_img, 2):
            raise RuntimeError(f"detect_finish: img_wh {tuple(img_wh.shape)} must be ({n_img}, 2)")
    det = torch.empty((max(n_groups * M, 1), 6), dtype=torch.float64, device=rec.device)
    image = torch.empty((max(n_groups * M, 1),), dtype=torch.int32, device=rec.device)
    off = torch.empty((n_img + 1,), dtype=torch.int32, device=rec.device)
    check(lib().yolo_detect_finish(ptr(rec), ptr(keep), ptr(kc), n_groups, M, int(groups_per_image), ptr(img_wh), ptr(det), ptr(image), ptr(off),
                                   stream()), "yolo_detect_finish")
    return det, image, off


def detect(pred: torch.Tensor, conf_thr: float, nms_thr: float, S: int, B: int, C: int, scoring: str = "argmax", img_wh=None):
    """Batched detection on the device: decode, NMS (inference variant) and ``detect_finish`` as three launches, no
    synchronisation.  Returns the device tensors (det, image, off) of ``detect_finish``."""
    rec, keep, kc, gpi = _groups(pred, conf_thr, nms_thr, _hip.NMS_INFERENCE, S, B, C, scoring)
    return detect_finish(rec, keep, kc, gpi, img_wh)


def rows_to_host(det: torch.Tensor, off: torch.Tensor):
    """(det, off) of ``detect_finish`` as NumPy arrays in two small copies: ``off`` first, then exactly ``off[-1]`` rows"""
    off_h = off.cpu().numpy()
    return det[: int(off_h[-1])].cpu().numpy(), off_h


def detect_host(pred: torch.Tensor, conf_thr: float, nms_thr: float, S: int, B: int, C: int, scoring: str = "argmax", img_wh=None):
    """``detect`` with the result on the host: (det (total, 6) f64, image (total,) i32, off (images + 1,) i32) as NumPy arrays.
    Two small device->host copies -- ``off``, then exactly ``total`` rows; ``image`` is ``off`` spelled out per row."""
    det, _, off = detect(pred, conf_thr, nms_thr, S, B, C, scoring, img_wh)
    det_h, off_h = rows_to_host(det, off)
    return det_h, np.repeat(np.arange(len(off_h) - 1, dtype=np.int32), np.diff(off_h)), off_h


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------


@_hip.device_guard
def loss_fwd_bwd(pred: torch.Tensor, tgt: torch.Tensor, S: int, B: int, C: int, lambda_coord: float, lambda_noobj: float,
                 want_grad: bool = True):
    """Fused loss forward+backward (src/yolo/loss.py:87-212).  Returns (out8 fp32 device tensor, dpred or None)."""
    pred = _as_f32_dev(pred)
    tgt = _as_f32_dev(tgt)
    N = pred.shape[0]
    if pred.dim() != 4 or tuple(pred.shape) != (N, S, S, 5 * B + C) or tgt.shape != pred.shape:
        # the kernel cannot know the buffers' extents: e.g. YOLOLoss(S=14) on S=7 predictions would read out of bounds
        raise RuntimeError(f"YOLOLoss: predictions {tuple(pred.shape)} / targets {tuple(tgt.shape)} must both be (N, {S}, {S}, {5 * B + C})")
    out = torch.empty((8,), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    work = torch.empty((N * 8,), dtype=torch.float64, device=pred.device)
    check(lib().yolo_loss_fwd_bwd(ptr(pred), ptr(tgt), N, S, B, C, float(lambda_coord), float(lambda_noobj),
                                  ptr(out), ptr(dpred), ptr(work), stream()), "yolo_loss_fwd_bwd")
    return out, dpred


@_hip.device_guard
def loss_iou(b1: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """YOLOLoss.compute_iou (src/yolo/loss.py:174-212) with broadcasting done here."""
    b1, b2 = torch.broadcast_tensors(b1, b2)
    b1 = _as_f32_dev(b1)
    b2 = _as_f32_dev(b2)
    out = torch.empty(b1.shape[:-1], dtype=torch.float32, device=b1.device)
    check(lib().yolo_loss_iou(ptr(b1), ptr(b2), out.numel(), ptr(out), stream()), "yolo_loss_iou")
    return out
