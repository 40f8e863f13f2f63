"""Inference pipeline with the reference's single-image surface (src/yolo/inference.py:12-317), and batches of images.

``predict`` = load -> resize/normalise -> model -> decode -> NMS.  On a ROCm device the model runs on
the HIP engine and decode + NMS run as two kernel launches with ONE device->host copy, instead of
~880 ``.item()`` syncs per image (inference.py:184-191).

``predict_batch`` / ``predict_batch_arrays`` take a list of files, PIL images or decoded arrays of any sizes (DESIGN.md,
"Batched detection"): a thread pool decodes batch k + 1 while batch k runs, a batch is uploaded as one packed uint8 buffer
(``yolo.augment.U8Batch``) and resized on the device, and decode + NMS + ``yolo_detect_finish`` leave the per-image result lists
on the device, so the copy back is the detections alone.
"""

from __future__ import annotations

import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn as nn
from PIL import Image

from . import _post_cpu
from .schemas import BoundingBox, Detection

EPSILON = 1e-6  # in the IoU denominator of this variant (reference inference.py:9,248)

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


class _Preprocess:
    """Resize((448,448)) -> ToTensor -> Normalize(ImageNet) without torchvision.
    PIL's bilinear ``resize`` is what torchvision's ``Resize`` calls for PIL inputs."""

    def __init__(self, size=(448, 448), mean=_MEAN, std=_STD):
        self.size = size
        self.mean_t, self.std_t = tuple(mean), tuple(std)
        self.mean = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)

    def __call__(self, image: Image.Image) -> torch.Tensor:
        img = image.resize((self.size[1], self.size[0]), Image.BILINEAR)
        arr = np.asarray(img, dtype=np.uint8)
        if arr.ndim == 2:
            arr = arr[:, :, None]
        t = torch.from_numpy(arr.copy()).permute(2, 0, 1).to(torch.float32).div_(255.0)
        return (t - self.mean) / self.std


def _clamp_workers(workers: int) -> int:
    """decoder threads of ``predict_batch``: what the caller asks for within 1 .. 16, never the machine's CPU count"""
    return max(1, min(16, int(workers)))


def _default_device() -> str:
    if torch.backends.mps.is_available():
        return "mps"
    return "cuda" if torch.cuda.is_available() else "cpu"


class YOLOInference:
    """Inference engine: ``device`` / ``model`` / ``transform`` attributes and the methods of the reference."""

    def __init__(self, model: nn.Module, device: str | None = None) -> None:
        self.device = _default_device() if device is None else device
        self.model = model.to(self.device)
        self.model.eval()
        self.transform = _Preprocess()

    # ------------------------------------------------------------------ image handling
    def load_image(self, image_path: str) -> Image.Image:
        return Image.open(image_path).convert("RGB")

    def preprocess_image(self, image: Image.Image) -> torch.Tensor:
        if self._on_gpu() and isinstance(self.transform, _Preprocess) and image.mode == "RGB":
            # device path: ship the decoded uint8 pixels (3 B each, not 12) and resize + normalise there --
            # bit-identical to the host transform (yolo/preprocess.py)
            from .preprocess import preprocess_u8
            u8 = torch.from_numpy(np.asarray(image, dtype=np.uint8).copy()).unsqueeze(0).to(self.device)
            out, _ = preprocess_u8(u8, self.transform.size, self.transform.mean_t, self.transform.std_t)
            return out
        return self.transform(image).unsqueeze(0).to(self.device)

    def _on_gpu(self) -> bool:
        return torch.device(self.device).type == "cuda"

    # ------------------------------------------------------------------ pipeline
    def predict(self, image_path: str, conf_threshold: float = 0.5, nms_threshold: float = 0.4,
                class_names: list[str] | None = None, scoring: str = "argmax") -> list[Detection]:
        """scoring="all": the paper's test-time protocol -- every box scored for every class, NMS per class, the kept detections
        of all classes by confidence (a box may come out under several classes)."""
        _post_cpu.check_scoring(scoring)
        return self._predict_loaded(self.load_image(image_path), conf_threshold, nms_threshold, class_names, scoring)

    def _predict_loaded(self, image: Image.Image, conf_threshold: float, nms_threshold: float, class_names, scoring: str) -> list[Detection]:
        """``predict`` behind ``load_image``"""
        x = self.preprocess_image(image)
        with torch.no_grad():
            pred = self.model(x)
        if pred.is_cuda:
            from . import ops
            S, B = self.model.S, self.model.B
            C = pred.shape[-1] - 5 * B
            (rec, keep), = ops.postprocess_host(pred[:1], conf_threshold, nms_threshold, ops._hip.NMS_INFERENCE, S, B, C, scoring)
            dets = self._records_to_detections(rec, class_names)   # validates every decoded box like the reference
            return [dets[k] for k in keep]
        if scoring == "all":
            groups = _post_cpu.decode_classes(pred[0].detach().numpy(), conf_threshold, self.model.S, self.model.B)
            rec, keep = _post_cpu.nms_classes(groups, nms_threshold, _post_cpu.INFERENCE)
            dets = self._records_to_detections(rec, class_names)
            return [dets[k] for k in keep]
        dets = self.parse_predictions(pred[0], conf_threshold, class_names)
        return self.non_max_suppression(dets, nms_threshold)

    @staticmethod
    def _records_to_detections(rec: np.ndarray, class_names) -> list[Detection]:
        out = []
        for c, conf, x, y, w, h in rec.tolist():
            cid = int(c)
            out.append(Detection(class_id=cid, class_name=class_names[cid] if class_names else f"class_{cid}",
                                 confidence=conf, bbox=BoundingBox(x=x, y=y, width=w, height=h)))
        return out

    # ------------------------------------------------------------------ batches
    def predict_batch(self, images, conf_threshold: float = 0.5, nms_threshold: float = 0.4, class_names: list[str] | None = None,
                      scoring: str = "argmax", batch_size: int = 64, workers: int = 4) -> list[list[Detection]]:
        """``predict`` for many images -- paths, PIL images or uint8 (H, W, 3) arrays in any mix, of any sizes: per image, in input
        order, the detections ``predict`` would return.  On a device the files are decoded by ``workers`` threads while the previous
        batch runs, a batch travels as one packed uint8 buffer, and decode + NMS + the per-image result lists are three launches whose
        output -- the detections and nothing else -- is all that is copied back.  A CPU model takes the images one by one."""
        _post_cpu.check_scoring(scoring)
        images = list(images)
        if not self._on_gpu():
            return [self._predict_loaded(im, conf_threshold, nms_threshold, class_names, scoring) for im in self._loaded(images, workers)]
        out = []
        for det, off, _ in self._device_batches(images, conf_threshold, nms_threshold, scoring, batch_size, workers, pixels=False):
            dets = self._records_to_detections(det, class_names)     # validates every box like the reference
            out += [dets[off[n]: off[n + 1]] for n in range(len(off) - 1)]
        return out

    def predict_batch_arrays(self, images, conf_threshold: float = 0.5, nms_threshold: float = 0.4, class_names: list[str] | None = None,
                             scoring: str = "argmax", batch_size: int = 64, workers: int = 4, normalized: bool = False):
        """``predict_batch`` for bulk callers: (image_index (n,) int32, class_id (n,) int32, score (n,) f64, pixel_boxes (n, 4) f64
        {xmin, ymin, xmax, ymax} clamped to the image, sizes (images, 2) int32 {W, H}), rows in input order of the images and
        result order inside an image.  ``normalized``: a sixth array (n, 4), the boxes as ``predict`` reports them {x, y, w, h}.
        ``class_names`` is accepted for the common signature and not used."""
        _post_cpu.check_scoring(scoring)
        images = list(images)
        det, norm, idx, sizes = [np.zeros((0, 6))], [np.zeros((0, 4))], [np.zeros(0, np.int32)], [np.zeros((0, 2), np.int32)]
        if not self._on_gpu():
            for i, im in enumerate(self._loaded(images, workers)):
                ds = self._predict_loaded(im, conf_threshold, nms_threshold, None, scoring)
                box = np.array([[d.bbox.x, d.bbox.y, d.bbox.width, d.bbox.height] for d in ds], np.float64).reshape(-1, 4)
                head = np.array([[d.class_id, d.confidence] for d in ds], np.float64).reshape(-1, 2)
                det.append(np.concatenate([head, _post_cpu.voc_pixel_boxes(box, im.width, im.height)], 1))
                norm.append(box)
                idx.append(np.full(len(ds), i, np.int32))
                sizes.append(np.array([[im.width, im.height]], np.int32))
        else:
            base = 0
            for d, off, wh, *xywh in self._device_batches(images, conf_threshold, nms_threshold, scoring, batch_size, workers, pixels=True,
                                                          both=normalized):
                det.append(d)
                norm += xywh
                idx.append(np.repeat(np.arange(base, base + len(wh), dtype=np.int32), np.diff(off)))
                sizes.append(wh)
                base += len(wh)
        det = np.concatenate(det)
        res = (np.concatenate(idx), det[:, 0].astype(np.int32), det[:, 1].copy(), det[:, 2:6].copy(), np.concatenate(sizes))
        return res + (np.concatenate(norm),) if normalized else res

    @staticmethod
    def _decoded(item):
        """path -> RGB PIL image (the caller's ``load_image``); PIL image -> RGB; uint8 (H, W, 3) array or tensor -> itself"""
        if isinstance(item, Image.Image):
            return item if item.mode == "RGB" else item.convert("RGB")
        if isinstance(item, torch.Tensor):
            item = item.detach().cpu().numpy()
        if isinstance(item, np.ndarray):
            if item.dtype != np.uint8 or item.ndim != 3 or item.shape[2] != 3:
                raise ValueError(f"predict_batch takes uint8 images of shape (H, W, 3), got {item.dtype} {item.shape}")
            return item
        return None

    def _load_one(self, item):
        """one input of ``predict_batch`` decoded: a PIL RGB image or a uint8 (H, W, 3) array; runs in a worker thread"""
        got = self._decoded(item)
        if got is not None:
            return got
        try:
            return self.load_image(item)
        except Exception as e:
            raise RuntimeError(f"predict_batch: cannot read image {str(item)!r}: {e}") from e

    def _loaded(self, images, workers: int):
        """CPU path: every input as a PIL RGB image, decoded by the pool ahead of the loop; the pool is gone when this returns"""
        with ThreadPoolExecutor(max_workers=_clamp_workers(workers)) as pool:
            futures = [pool.submit(self._load_one, im) for im in images]
            try:
                return [im if isinstance(im, Image.Image) else Image.fromarray(im) for im in (f.result() for f in futures)]
            except BaseException:
                pool.shutdown(wait=True, cancel_futures=True)
                raise

    def _device_batches(self, images, conf_threshold, nms_threshold, scoring, batch_size, workers, pixels: bool, both: bool = False):
        """The host pipeline of ``predict_batch`` on a device; yields per batch (det (rows, 6), off (images + 1,), sizes (images, 2)
        {W, H}[, xywh (rows, 4) if ``both``]) as NumPy arrays; det holds pixel corners if ``pixels`` else the records' x, y, w, h.
        At most two batches are in flight: batch k + 1 is decoded by the pool while batch k runs.  The packed images go through two
        page-locked staging buffers in turn, each rewritten only after an event recorded behind its upload has completed; uploads and
        kernels share the current stream."""
        from . import ops
        from .augment import U8Batch
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        model, dev = self.model, torch.device(self.device)
        S, B = model.S, model.B
        fused = hasattr(model, "_fusable") and model._fusable()
        size = self.transform.size if isinstance(self.transform, _Preprocess) else (448, 448)
        chunks = [images[i: i + batch_size] for i in range(0, len(images), batch_size)]
        staging, uploaded = [None, None], [None, None]
        pool = ThreadPoolExecutor(max_workers=_clamp_workers(workers))
        try:
            submit = lambda chunk: [pool.submit(self._load_one, im) for im in chunk]
            pending = submit(chunks[0]) if chunks else None
            for k in range(len(chunks)):
                following = submit(chunks[k + 1]) if k + 1 < len(chunks) else None      # decoded while batch k runs
                arrays = [np.asarray(im, dtype=np.uint8) for im in (f.result() for f in pending)]
                pending = following
                slot, need = k % 2, sum(a.size for a in arrays)
                if uploaded[slot] is not None:
                    uploaded[slot].synchronize()
                if staging[slot] is None or staging[slot].numel() < need:
                    staging[slot] = torch.empty(need + need // 4, dtype=torch.uint8, pin_memory=True)
                with torch.cuda.device(dev), torch.no_grad():
                    batch = U8Batch.from_images(arrays, size, buffer=staging[slot]).to(dev, non_blocking=True)
                    uploaded[slot] = torch.cuda.Event()
                    uploaded[slot].record()
                    pred = model(batch if fused else batch.to_tensor())
                    wh = np.array([[a.shape[1], a.shape[0]] for a in arrays], np.int32)
                    rec, keep, kc, gpi = ops._groups(pred, conf_threshold, nms_threshold, ops._hip.NMS_INFERENCE, S, B, pred.shape[-1] - 5 * B, scoring)
                    first = ops.detect_finish(rec, keep, kc, gpi, wh if pixels else None)
                    second = ops.detect_finish(rec, keep, kc, gpi, None) if pixels and both else None
                    det, off = ops.rows_to_host(first[0], first[2])
                    out = (det, off, wh) + ((second[0][: len(det), 2:6].cpu().numpy(),) if second is not None else ())
                yield out          # (outside the no_grad / device scopes: they must not stay entered while the caller runs)
        finally:
            pool.shutdown(wait=True, cancel_futures=True)

    def parse_predictions(self, pred: torch.Tensor, conf_threshold: float, class_names: list[str] | None = None,
                          scoring: str = "argmax") -> list[Detection]:
        """(S,S,5B+C) -> Detections with conf*prob > threshold, (row, col, box) scan order.
        scoring="all": conf_b*prob_c of every class c, the lists of the classes one behind the other (classes ascending)."""
        S, B = self.model.S, self.model.B
        if _post_cpu.check_scoring(scoring) == "all":
            if pred.is_cuda:
                from . import ops
                rec, cnt = ops.decode_classes(pred.unsqueeze(0), conf_threshold, S, B, pred.shape[-1] - 5 * B)
                rec, cnt = rec[0].cpu().numpy(), cnt[0].cpu().numpy()
                rec = rec[np.arange(rec.shape[1])[None, :] < cnt[:, None]]
            else:
                rec = np.concatenate(_post_cpu.decode_classes(pred.detach().numpy(), conf_threshold, S, B))
            return self._records_to_detections(rec, class_names)
        if pred.is_cuda:
            from . import ops
            rec, cnt = ops.decode(pred.unsqueeze(0), conf_threshold, S, B, pred.shape[-1] - 5 * B)
            rec = rec[0, : int(cnt[0])].cpu().numpy()
        else:
            rec = _post_cpu.decode(pred.detach().numpy(), conf_threshold, S, B)
        return self._records_to_detections(rec, class_names)

    def iou(self, bbox1: BoundingBox, bbox2: BoundingBox) -> float:
        """IoU of two boxes with +EPSILON in the denominator (Python-float arithmetic)."""
        ax1, ay1, ax2, ay2 = bbox1.to_corners()
        bx1, by1, bx2, by2 = bbox2.to_corners()
        iw = max(0, min(ax2, bx2) - max(ax1, bx1))
        ih = max(0, min(ay2, by2) - max(ay1, by1))
        inter = iw * ih
        return inter / (bbox1.area + bbox2.area - inter + EPSILON)

    def non_max_suppression(self, detections: list[Detection], nms_threshold: float = None, iou_threshold: float = None) -> list[Detection]:
        """Greedy per-class NMS; a box survives a kept one iff its class differs or IoU < threshold.
        ``iou_threshold`` is the deprecated spelling and wins when given."""
        if iou_threshold is not None:
            warnings.warn("Parameter 'iou_threshold' is deprecated, use 'nms_threshold' instead.", DeprecationWarning, stacklevel=2)
            thr = iou_threshold
        elif nms_threshold is not None:
            thr = nms_threshold
        else:
            thr = 0.4
        if len(detections) == 0:
            return []
        rec = np.array([[d.class_id, d.confidence, d.bbox.x, d.bbox.y, d.bbox.width, d.bbox.height] for d in detections], np.float64)
        if self._on_gpu():
            # a GPU model never takes a host loop silently: the device kernels cover up to 1024 boxes per image
            # (S = 14, B = 3 -> 588); a longer list is refused by yolo_nms and that error propagates
            from . import ops
            cap = 128 if len(rec) <= 128 else max(len(rec), 129)
            rec_d = torch.zeros((1, cap, 6), dtype=torch.float64, device=self.device)
            rec_d[0, : len(rec)] = torch.from_numpy(rec)
            cnt = torch.tensor([len(rec)], dtype=torch.int32, device=self.device)
            keep, kc = ops.nms(rec_d, cnt, thr, ops._hip.NMS_INFERENCE)
            keep = keep[0, : int(kc[0])].cpu().numpy()
        else:
            keep = _post_cpu.nms(rec, thr, _post_cpu.INFERENCE)
        return [detections[k] for k in keep]
