"""Training / validation input path on the device (libyolo_hip.so: yolo_augment_u8).

The reference augments every training sample on the host, one PIL image at a time (src/yolo/dataset.py:288-319
RandomResizedCrop + ColorJitter, 325-409 the transform calls of ``__getitem__``), and ships fp32.  Here the host decodes the
file and draws the random parameters (``yolo.dataset._Augment.sample``); a batch travels as ONE packed uint8 buffer of images of
different sizes plus one descriptor per image (``U8Batch``), and two kernel launches do crop -> Pillow-exact resize -> colour
operations in the sampled order -> ToTensor -> Normalize, into the stem's NHWC4 bf16 buffer (``Plan.forward``) or an NCHW fp32
tensor (``U8Batch.to_tensor``).  The result is bit-identical to the host path (``_Augment.apply`` + ``_Preprocess``) for the
same parameters: tests/test_gpu_augment.py.  The Darknet recipe (``_DarknetAugment``: ``JitterParams`` entries) goes through the same two
launches -- window with edge replication, flip, one HSV operation -- and may share a batch with ``AugParams`` entries:
tests/test_gpu_darknet_augment.py.  The classification pretraining (``dataset._ClassifyTransform``) sends ``AugParams`` with its ``flip``
set, into ``YOLOv1Classifier``'s trunk plan: tests/test_gpu_pretrain_scale.py.

    ds = create_voc_datasets(..., device_transform=True)
    loader = DataLoader(ds, batch_size=64, collate_fn=collate_u8, pin_memory=True)
    for images, targets in loader:              # images: U8Batch
        pred = model(images.to("cuda", non_blocking=True))
"""

from __future__ import annotations

import ctypes
import math
from typing import Sequence

import numpy as np
import torch
from PIL import Image

from . import _hip
from .dataset import AugParams, JitterParams, _Augment, _DarknetAugment
from .preprocess import MEAN, STD, bilinear_tables

# (in_size, out_size, device index) -> (int32 device tensor [out][2 + k]: first input index, count, k weights; k).  Never evicted:
# descriptors of batches in flight hold raw pointers into these tensors, and crop sizes are integers in a narrow range.
_TABLES: dict = {}


def _device_table(in_size: int, out_size: int, dev: torch.device):
    key = (in_size, out_size, dev.index)
    hit = _TABLES.get(key)
    if hit is None:
        b, c, k = bilinear_tables(in_size, out_size)
        hit = _TABLES[key] = (torch.from_numpy(np.concatenate([b, c], axis=1)).to(dev), k)
    return hit


class U8Batch:
    """N decoded RGB images of different sizes, packed HWC into one uint8 buffer, with the parameters of their crop and colour
    operations: one ``AugParams`` (reference recipe, crop inside the image) or ``JitterParams`` (Darknet recipe, a window that may
    leave the image) per image, in any mix.  Stands for the (N, 3, H, W) fp32 batch the host path would have produced: ``shape``, ``is_cuda``, ``device``,
    ``to`` and ``pin_memory`` behave as a tensor's do, so loaders and training loops pass it along unchanged."""

    requires_grad = False

    def __init__(self, data: torch.Tensor, sizes: Sequence, params: Sequence, size=(448, 448), mean=MEAN, std=STD):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("U8Batch expects a flat uint8 buffer")
        if len(sizes) != len(params) or not sizes:
            raise ValueError("U8Batch needs one (H, W) and one AugParams / JitterParams per image, and at least one image")
        self.data, self.sizes, self.params = data, [tuple(int(v) for v in s) for s in sizes], list(params)
        self.size, self.mean, self.std = (int(size[0]), int(size[1])), tuple(mean), tuple(std)
        self.offsets, off = [], 0
        for (h, w), p in zip(self.sizes, self.params):
            if isinstance(p, JitterParams):          # only this recipe's window may leave the image; it still has to meet it
                if not (p.ch > 0 and p.cw > 0 and p.top < h and p.top + p.ch > 0 and p.left < w and p.left + p.cw > 0):
                    raise ValueError(f"window {tuple(p[:4])} misses its {h} x {w} image")
                if not (0.0 <= p.saturation < math.inf and 0.0 <= p.exposure < math.inf):
                    raise ValueError("saturation and exposure must be finite and >= 0")
            else:
                if not (0 <= p.top and 0 <= p.left and p.ch > 0 and p.cw > 0 and p.top + p.ch <= h and p.left + p.cw <= w):
                    raise ValueError(f"crop {tuple(p[:4])} outside its {h} x {w} image")
                if len(p.ops) > 3:
                    raise ValueError("at most 3 colour operations")
            self.offsets.append(off)
            off += h * w * 3
        if off != data.numel():
            raise ValueError(f"buffer holds {data.numel()} bytes, the images need {off}")
        self._descs = self._descs_dev = None
        self._tmp_bytes = 0

    @classmethod
    def from_images(cls, images: Sequence, size=(448, 448), buffer: torch.Tensor = None) -> "U8Batch":
        """The inference transform of decoded images of any sizes (uint8 (H, W, 3) arrays or tensors): the whole image as the
        crop, no colour operation, no flip -- Resize(size) + ToTensor + Normalize, what ``YOLOInference.preprocess_image`` does.
        ``buffer``: a flat uint8 host tensor (e.g. page-locked) at least as large as the images together; they are packed into
        its head instead of a fresh buffer."""
        arrays = [im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im) for im in images]
        for a in arrays:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"U8Batch.from_images expects uint8 images of shape (H, W, 3), got {a.dtype} {tuple(a.shape)}")
        total = sum(a.size for a in arrays)
        if buffer is None:
            buffer = torch.empty(total, dtype=torch.uint8)
        elif buffer.dtype != torch.uint8 or buffer.dim() != 1 or buffer.is_cuda or not buffer.is_contiguous() or buffer.numel() < total:
            raise ValueError(f"buffer must be a flat uint8 host tensor of at least {total} bytes")
        flat, off = buffer.numpy(), 0            # (shares the buffer's memory; the images may be read-only arrays)
        for a in arrays:
            flat[off: off + a.size] = a.reshape(-1)
            off += a.size
        sizes = [(a.shape[0], a.shape[1]) for a in arrays]
        return cls(buffer[:total], sizes, [AugParams(0, 0, h, w) for h, w in sizes], size)

    # ------------------------------------------------------------------ tensor-like surface
    def __len__(self) -> int:
        return len(self.sizes)

    @property
    def shape(self) -> torch.Size:
        return torch.Size((len(self.sizes), 3, self.size[0], self.size[1]))

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    def requires_grad_(self, requires_grad: bool = True):
        if requires_grad:
            raise RuntimeError("a U8Batch has no input gradient: the uint8 pixels are not differentiable; call .to_tensor() and ask "
                               "for the gradient of that fp32 tensor")
        return self

    def pin_memory(self):
        return U8Batch(self.data.pin_memory(), self.sizes, self.params, self.size, self.mean, self.std)

    def to(self, device, non_blocking: bool = False):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.data.device:
            return self
        out = U8Batch(self.data.to(device, non_blocking=non_blocking), self.sizes, self.params, self.size, self.mean, self.std)
        if device.type == "cuda":
            out._build_descriptors()
        return out

    def cuda(self, non_blocking: bool = False):
        return self.to("cuda", non_blocking=non_blocking)

    def cpu(self):
        return self.to("cpu")

    def image(self, i: int) -> torch.Tensor:
        """decoded image i as a (H, W, 3) view of the buffer"""
        h, w = self.sizes[i]
        return self.data[self.offsets[i]: self.offsets[i] + h * w * 3].view(h, w, 3)

    # ------------------------------------------------------------------ device side
    def _build_descriptors(self) -> None:
        """the yolo_augment_desc array of this batch for the device the buffer lies on: tables from the per-device cache (only
        sizes not seen before are uploaded), the ragged layout of the horizontal pass's scratch, one small upload"""
        dev = self.data.device
        Ho, Wo = self.size
        descs = (_hip.AugmentDesc * len(self.sizes))()
        tmp = 0
        with torch.cuda.device(dev):
            for d, (h, w), off, p in zip(descs, self.sizes, self.offsets, self.params):
                d.src_off, d.Hs, d.Ws = off, h, w
                d.top, d.left, d.ch, d.cw = p.top, p.left, p.ch, p.cw
                if p.cw != Wo:
                    t, d.hk = _device_table(p.cw, Wo, dev)
                    d.htab = t.data_ptr()
                    d.tmp_off = tmp
                    tmp += p.ch * Wo * 3
                if p.ch != Ho:
                    t, d.vk = _device_table(p.ch, Ho, dev)
                    d.vtab = t.data_ptr()
                if isinstance(p, JitterParams):
                    inside = 0 <= p.top and 0 <= p.left and p.top + p.ch <= h and p.left + p.cw <= w
                    d.flags = (_hip.AUG_F_FLIP if p.flip else 0) | (0 if inside else _hip.AUG_F_EDGE)
                    d.n_ops, d.ops[0] = 1, _hip.AUG_HSV
                    d.brightness, d.saturation, d.hue_shift = p.exposure, p.saturation, int(p.hue * 255)
                    continue
                d.flags = _hip.AUG_F_FLIP if p.flip else 0          # (the classification transform's; the kernel mirrors the columns of stage 1)
                d.n_ops = len(p.ops)
                for i, op in enumerate(p.ops):
                    d.ops[i] = op
                d.brightness, d.saturation, d.hue_shift = p.brightness, p.saturation, int(p.hue * 255)
            self._descs, self._tmp_bytes = descs, tmp
            self._descs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)

    def _run(self, act=None, nchw=None, u8=None) -> None:
        _hip.require_cuda(self.data, nchw, u8)
        if self._descs is None:
            self._build_descriptors()
        dev = self.data.device
        with torch.cuda.device(dev):
            tmp = torch.empty(self._tmp_bytes, dtype=torch.uint8, device=dev) if self._tmp_bytes else None
            m3, s3 = (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std)
            _hip.check(_hip.lib().yolo_augment_u8(_hip.ptr(self.data), self.data.numel(), self._descs, _hip.ptr(self._descs_dev), len(self.sizes), self.size[0],
                                                  self.size[1], _hip.ptr(tmp), self._tmp_bytes, m3, s3, act.p if act is not None else None,
                                                  act.halo if act is not None else 0, _hip.ptr(nchw), _hip.ptr(u8), _hip.stream()), "yolo_augment_u8")

    def into_act(self, act) -> None:
        """augment + normalise into an existing NHWC4 bf16 activation buffer (the stem's input)"""
        if (act.N, act.H, act.W, act.C) != (len(self.sizes), self.size[0], self.size[1], 4):
            raise ValueError("activation buffer does not match the batch / target size")
        self._run(act=act)

    def to_uint8(self) -> torch.Tensor:
        """the augmented images before ToTensor, uint8 (N, H, W, 3) -- on the device through the kernel, on the CPU through PIL"""
        if self.is_cuda:
            out = torch.empty((len(self.sizes), self.size[0], self.size[1], 3), dtype=torch.uint8, device=self.device)
            self._run(u8=out)
            return out
        return torch.stack([torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()) for im in self._host_images()])

    def to_tensor(self) -> torch.Tensor:
        """the (N, 3, H, W) fp32 batch this object stands for: on the device through yolo_augment_u8, on the CPU through the host
        path (``_Augment.apply`` / ``_DarknetAugment.apply`` on PIL + ToTensor + Normalize) -- the same bits either way"""
        if self.is_cuda:
            out = torch.empty(tuple(self.shape), dtype=torch.float32, device=self.device)
            self._run(nchw=out)
            return out
        from .inference import _Preprocess
        finish = _Preprocess(self.size, self.mean, self.std)
        return torch.stack([finish(im) for im in self._host_images()])

    def _host_images(self):
        ref, dark = _Augment(self.size), _DarknetAugment(self.size)
        return [(dark if isinstance(p, JitterParams) else ref).apply(Image.fromarray(self.image(i).numpy()), [], p)[0] for i, p in enumerate(self.params)]


def collate_u8(samples, size=(448, 448), pin_memory: bool = False):
    """collate function for datasets in ``device_transform`` mode: [(uint8 HWC tensor, AugParams or JitterParams, target), ...] ->
    (U8Batch, stacked targets).  ``pin_memory``: pack straight into page-locked memory (a DataLoader with ``pin_memory=True`` pins
    the batch by itself through ``U8Batch.pin_memory``)."""
    images = [s[0] for s in samples]
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("collate_u8 expects uint8 images of shape (H, W, 3)")
    total = sum(im.numel() for im in images)
    buf = torch.empty(total, dtype=torch.uint8, pin_memory=pin_memory)
    off = 0
    for im in images:
        buf[off: off + im.numel()] = im.reshape(-1)
        off += im.numel()
    batch = U8Batch(buf, [im.shape[:2] for im in images], [s[1] for s in samples], size)
    return batch, torch.stack([s[2] for s in samples])
