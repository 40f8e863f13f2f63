"""Data side of the reference's surface (src/yolo/dataset.py), without torchvision.

``VOCDetectionYOLO`` / ``CombinedVOCDataset`` / ``create_voc_datasets`` keep the reference's constructor arguments,
attributes (``S, B, C, class_names, class_to_idx, augment, target_size``) and return types; what the reference delegates
to ``torchvision.datasets.VOCDetection`` and ``torchvision.transforms.v2`` (un-vendored dependencies) is restated here:

  * the VOC directory layout ``<root>/[<Kaggle split dir>/]VOCdevkit/VOC<year>/{JPEGImages, Annotations,
    ImageSets/Main/<image_set>.txt}`` and the XML -> nested-dict conversion of ``VOCDetection.parse_voc_xml`` (the
    annotation dicts passed to ``_extract_bboxes_from_annotation`` have torchvision's shape, dataset.py:411-467);
  * evaluation transform = Resize (PIL bilinear) -> ToTensor -> Normalize, i.e. ``yolo.inference._Preprocess``
    (bit-identical to the reference's v2 pipeline for PIL inputs, tests/test_preprocess_cpu.py);
  * training augmentation = box-aware RandomResizedCrop(scale (0.8, 1.2), ratio (0.8, 1.2)) + ColorJitter(brightness 0.5,
    saturation 0.5, hue 0.1) (dataset.py:288-319), same distributions, drawn from ``torch``'s global RNG -- the random
    STREAM differs from torchvision's, so augmented samples are "parity unpinned" (statistics, not bits);
  * ``recipe="darknet"`` (additive): the YOLOv1 paper's augmentation instead -- scaling and translation by up to 20 % of the
    image size past the image border (edge replication), a horizontal flip, exposure and saturation scaled by up to 1.5 and
    the hue shifted by up to 0.1 in HSV (``_DarknetAugment``);
  * ``download=True`` (kagglehub) is not available offline and raises.

``encode_target`` restates ``_encode_target`` (dataset.py:487-532); ``SyntheticYOLODataset`` feeds benchmarks and tests.
"""

from __future__ import annotations

import math
import os
import xml.etree.ElementTree as ET
from pathlib import Path
from typing import List, NamedTuple, Tuple

import numpy as np
import torch
from PIL import Image, ImageEnhance
from torch.utils.data import Dataset

VOC_CLASSES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
               "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]


def encode_target(bboxes, class_ids, S: int = 7, B: int = 2, C: int = 20) -> torch.Tensor:
    """Boxes (x_center, y_center, w, h in [0,1]) + class ids -> (S, S, 5B+C) target.
    The first object that lands in a cell owns it; only box slot 0 is filled; class is one-hot."""
    t = torch.zeros((S, S, 5 * B + C))
    for (xc, yc, w, h), cid in zip(bboxes, class_ids):
        i = min(int(S * yc), S - 1)
        j = min(int(S * xc), S - 1)
        if t[i, j, 4] == 0:
            t[i, j, 0] = S * xc - j
            t[i, j, 1] = S * yc - i
            t[i, j, 2] = w
            t[i, j, 3] = h
            t[i, j, 4] = 1.0
            t[i, j, 5 * B + cid] = 1.0
    return t


class SyntheticYOLODataset(Dataset):
    """Random 448x448 images ~N(0,1) with 0..max_obj encoded objects (the benchmark input of SURVEY.md 8d)."""

    def __init__(self, length: int = 256, S: int = 7, B: int = 2, C: int = 20, max_obj: int = 3, seed: int = 0, size: int = 448):
        self.length, self.S, self.B, self.C, self.max_obj, self.seed, self.size = length, S, B, C, max_obj, seed, size

    def __len__(self) -> int:
        return self.length

    def __getitem__(self, idx: int):
        rng = np.random.Generator(np.random.PCG64([self.seed, idx]))
        img = torch.from_numpy(rng.standard_normal((3, self.size, self.size), dtype=np.float32))
        k = int(rng.integers(0, self.max_obj + 1))
        boxes = [(*rng.uniform(0, 1, 2), *rng.uniform(0.05, 0.9, 2)) for _ in range(k)]
        cids = [int(rng.integers(0, self.C)) for _ in range(k)]
        return img, encode_target(boxes, cids, self.S, self.B, self.C)

    def ground_truth(self, idx: int) -> dict:
        """The sample's objects as an annotation would list them (yolo/voc_eval.py): ALL k boxes of ``__getitem__``'s generator, also
        those ``encode_target`` drops because their cell is taken, as pixel corners of a size x size image; nothing is difficult."""
        rng = np.random.Generator(np.random.PCG64([self.seed, idx]))
        rng.standard_normal((3, self.size, self.size), dtype=np.float32)          # the image's draws come first
        k = int(rng.integers(0, self.max_obj + 1))
        boxes = [(*rng.uniform(0, 1, 2), *rng.uniform(0.05, 0.9, 2)) for _ in range(k)]
        cids = [int(rng.integers(0, self.C)) for _ in range(k)]
        size = float(self.size)
        pix = [[(xc - w / 2) * size, (yc - h / 2) * size, (xc + w / 2) * size, (yc + h / 2) * size] for xc, yc, w, h in boxes]
        return {"image_id": f"{idx:06d}", "width": self.size, "height": self.size, "boxes": np.array(pix, np.float64).reshape(-1, 4),
                "class_ids": np.array(cids, np.int64), "difficult": np.zeros(k, bool)}


# ------------------------------------------------------------------------------------------------------------------
# PASCAL VOC on disk
# ------------------------------------------------------------------------------------------------------------------
def parse_voc_xml(node: ET.Element) -> dict:
    """XML element -> nested dict with the shape torchvision's ``VOCDetection.parse_voc_xml`` gives: a tag that repeats
    under one parent becomes a list, ``annotation["object"]`` is ALWAYS a list (empty without objects), leaves are the
    stripped text."""
    children = list(node)
    if not children:
        return {node.tag: (node.text or "").strip()}
    grouped: dict = {}
    for child in children:
        for k, v in parse_voc_xml(child).items():
            grouped.setdefault(k, []).append(v)
    inner = {k: (v[0] if len(v) == 1 else v) for k, v in grouped.items()}
    if node.tag == "annotation":
        inner["object"] = grouped.get("object", [])
    return {node.tag: inner}


OP_BRIGHTNESS, OP_SATURATION, OP_HUE, OP_HSV = 0, 1, 2, 4      # = YOLO_AUG_* of include/yolo_hip.h (3 is not assigned)


class _AugFields(NamedTuple):
    top: int
    left: int
    ch: int
    cw: int
    ops: Tuple[int, ...] = ()
    brightness: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0


class AugParams(_AugFields):
    """What ``_Augment.sample`` draws for one image: the crop, the colour operations in the order they are applied, their factors
    (``hue`` is the fraction of the hue circle; the H byte moves by ``int(hue * 255)``).  The host path (``_Augment.apply``) and
    the device path (yolo/augment.py -> yolo_augment_u8) both take it.

    ``flip`` (last argument, default False): the output is mirrored left to right.  ``_Augment.sample`` never draws one; the classification
    transform (``_ClassifyTransform.sample``) does.  It is an attribute beside the eight tuple entries, not a ninth: the tuple -- what
    iteration, ``len`` and ``tuple(p)`` give -- stays the crop and the colour parameters; ``==``, ``hash``, ``repr``, ``_replace`` and
    pickling carry the flip along.  The colour operations are per-pixel, so mirroring behind them (the host path) and in front of them
    (the kernel) give the same bytes."""
    flip = False

    def __new__(cls, top, left, ch, cw, ops=(), brightness=1.0, saturation=1.0, hue=0.0, flip=False):
        self = super().__new__(cls, top, left, ch, cw, ops, brightness, saturation, hue)
        if flip:
            self.flip = True          # (kept in the instance's __dict__, which is also what pickle ships as its state)
        return self

    def _replace(self, **kwargs):
        flip = kwargs.pop("flip", self.flip)
        return AugParams(*super()._replace(**kwargs), flip=flip)

    def __eq__(self, other):
        same = tuple.__eq__(self, other)
        return same if same is NotImplemented else (same and self.flip == getattr(other, "flip", False))

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self), self.flip))

    def __repr__(self):
        return super().__repr__()[:-1] + f", flip={self.flip})"


def crop_boxes(boxes, p: AugParams, size) -> List[List[float]]:
    """pixel-space XYXY boxes shifted into the crop, clamped to it and scaled with it to ``size`` = (H, W) (and mirrored with ``p.flip``)"""
    sx, sy = size[1] / p.cw, size[0] / p.ch
    out = []
    for x0, y0, x1, y1 in boxes:
        x0, x1 = min(max(x0 - p.left, 0.0), p.cw) * sx, min(max(x1 - p.left, 0.0), p.cw) * sx
        y0, y1 = min(max(y0 - p.top, 0.0), p.ch) * sy, min(max(y1 - p.top, 0.0), p.ch) * sy
        if p.flip:
            x0, x1 = size[1] - x1, size[1] - x0
        out.append([x0, y0, x1, y1])
    return out


class JitterParams(NamedTuple):
    """What ``_DarknetAugment.sample`` draws for one image: the window (it may extend past any border of the image), the flip, the hue
    shift (fraction of the hue circle; the H byte moves by ``int(hue * 255)``) and the factors of the S and V bytes.  The host path
    (``_DarknetAugment.apply``) and the device path (yolo/augment.py -> yolo_augment_u8) both take it."""
    top: int
    left: int
    ch: int
    cw: int
    flip: bool = False
    hue: float = 0.0
    saturation: float = 1.0
    exposure: float = 1.0


def jitter_boxes(boxes, p: JitterParams, size) -> Tuple[List[List[float]], List[int]]:
    """pixel-space XYXY boxes shifted into the window, scaled with it to ``size`` = (H, W), clamped to the output and mirrored with
    it; a box whose clamped width is below 1e-3 W or whose clamped height is below 1e-3 H is dropped (Darknet's rule).  Returns the
    boxes that stay and their indices in ``boxes``."""
    H, W = size
    sx, sy = W / p.cw, H / p.ch
    out, kept = [], []
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        x0, x1 = min(max((x0 - p.left) * sx, 0.0), W), min(max((x1 - p.left) * sx, 0.0), W)
        y0, y1 = min(max((y0 - p.top) * sy, 0.0), H), min(max((y1 - p.top) * sy, 0.0), H)
        if p.flip:
            x0, x1 = W - x1, W - x0
        if x1 - x0 < 1e-3 * W or y1 - y0 < 1e-3 * H:
            continue
        out.append([x0, y0, x1, y1])
        kept.append(i)
    return out, kept


def _uniform(a: float, b: float) -> float:
    return float(torch.empty(1).uniform_(a, b).item())


class _Augment:
    """RandomResizedCrop(size, scale=(0.8, 1.2), ratio=(0.8, 1.2)) + ColorJitter(brightness 0.5, saturation 0.5, hue 0.1),
    applied to a PIL image and its pixel-space XYXY boxes (torchvision.transforms.v2 semantics: the crop is sampled by
    area fraction x log-uniform aspect ratio, 10 tries, else the central crop at the clamped ratio; boxes are shifted,
    clamped to the crop and scaled with it; the colour operations run in a random order)."""

    def __init__(self, size: Tuple[int, int], scale=(0.8, 1.2), ratio=(0.8, 1.2), brightness=0.5, saturation=0.5, hue=0.1):
        self.size, self.scale, self.ratio = size, scale, ratio
        self.brightness, self.saturation, self.hue = brightness, saturation, hue

    def _crop_params(self, w: int, h: int):
        area = w * h
        log_r = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = area * _uniform(*self.scale)
            ar = math.exp(_uniform(*log_r))
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                top = int(torch.randint(0, h - ch + 1, (1,)).item())
                left = int(torch.randint(0, w - cw + 1, (1,)).item())
                return top, left, ch, cw
        in_ratio = w / h
        if in_ratio < self.ratio[0]:
            cw, ch = w, int(round(w / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            ch, cw = h, int(round(h * self.ratio[1]))
        else:
            cw, ch = w, h
        return (h - ch) // 2, (w - cw) // 2, ch, cw

    @staticmethod
    def _hue(img: Image.Image, delta: float) -> Image.Image:
        hsv = np.array(img.convert("HSV"), dtype=np.uint8)
        hsv[..., 0] = (hsv[..., 0].astype(np.int16) + int(delta * 255)) % 256
        return Image.fromarray(hsv, "HSV").convert("RGB")

    def sample(self, w: int, h: int) -> AugParams:
        """Draw the parameters for a w x h image from torch's global generator: crop tries, brightness, saturation, hue,
        then the order of the colour operations."""
        top, left, ch, cw = self._crop_params(w, h)
        ops, b, s, hu = [], 1.0, 1.0, 0.0
        if self.brightness:
            b = _uniform(max(0.0, 1 - self.brightness), 1 + self.brightness)
            ops.append(OP_BRIGHTNESS)
        if self.saturation:
            s = _uniform(max(0.0, 1 - self.saturation), 1 + self.saturation)
            ops.append(OP_SATURATION)
        if self.hue:
            hu = _uniform(-self.hue, self.hue)
            ops.append(OP_HUE)
        order = tuple(ops[k] for k in torch.randperm(len(ops)).tolist())
        return AugParams(top, left, ch, cw, order, b, s, hu)

    def apply(self, image: Image.Image, boxes: List[List[float]], p: AugParams):
        """The host path: crop, PIL bilinear resize, the colour operations of ``p`` in its order and its flip; boxes go with the crop."""
        image = image.crop((p.left, p.top, p.left + p.cw, p.top + p.ch)).resize((self.size[1], self.size[0]), Image.BILINEAR)
        for op in p.ops:
            if op == OP_BRIGHTNESS:
                image = ImageEnhance.Brightness(image).enhance(p.brightness)
            elif op == OP_SATURATION:
                image = ImageEnhance.Color(image).enhance(p.saturation)
            else:
                image = self._hue(image, p.hue)
        if p.flip:
            image = image.transpose(Image.FLIP_LEFT_RIGHT)
        return image, crop_boxes(boxes, p, self.size)

    def __call__(self, image: Image.Image, boxes: List[List[float]]):
        return self.apply(image, boxes, self.sample(*image.size))


class _DarknetAugment:
    """The training augmentation of the YOLOv1 paper (section 2.2) and Darknet's yolov1.cfg: a window displaced by up to ``jitter`` of
    the image size on every side -- it may extend past the image, whose border pixels are then replicated, as Darknet's crop does --
    resized to ``size``, a horizontal flip with probability ``flip``, and one round trip through HSV with the hue shifted by up to
    ``hue`` and saturation and exposure (S and V) scaled by up to ``saturation`` / ``exposure`` or their inverses.  H, S and V are
    Pillow's 8-bit channels (``convert("HSV")``), not Darknet's floats.  Shaped like ``_Augment``: ``sample`` / ``apply``."""

    def __init__(self, size: Tuple[int, int], jitter=0.2, hue=0.1, saturation=1.5, exposure=1.5, flip=0.5):
        self.size, self.jitter, self.hue, self.saturation, self.exposure, self.flip = size, jitter, hue, saturation, exposure, flip

    @staticmethod
    def _scale(k: float) -> float:
        s = _uniform(1.0, k)
        return 1.0 / s if float(torch.rand(1).item()) < 0.5 else s

    def sample(self, w: int, h: int) -> JitterParams:
        """Draw the parameters for a w x h image from torch's global generator, in this order: the integers pleft, pright in
        [-int(w * jitter), int(w * jitter)] (one ``randint`` of two), ptop, pbot in [-int(h * jitter), int(h * jitter)] (likewise), the
        flip (one ``rand``), the hue (uniform in +-hue), then the saturation and then the exposure, each a uniform s in [1, k]
        followed by one ``rand`` that inverts it (1 / s) with probability 1/2.  The window is left = pleft, top = ptop,
        cw = w - pleft - pright, ch = h - ptop - pbot."""
        dw, dh = int(w * self.jitter), int(h * self.jitter)
        pleft, pright = torch.randint(-dw, dw + 1, (2,)).tolist()
        ptop, pbot = torch.randint(-dh, dh + 1, (2,)).tolist()
        flip = float(torch.rand(1).item()) < self.flip
        hue = _uniform(-self.hue, self.hue)
        sat = self._scale(self.saturation)
        exp = self._scale(self.exposure)
        return JitterParams(ptop, pleft, h - ptop - pbot, w - pleft - pright, flip, hue, sat, exp)

    @staticmethod
    def _window(image: Image.Image, p: JitterParams) -> Image.Image:
        """pixel (y, x) of the window = source pixel (clamp(top + y, 0, h - 1), clamp(left + x, 0, w - 1))"""
        a = np.asarray(image, dtype=np.uint8)
        ys = np.clip(np.arange(p.top, p.top + p.ch), 0, a.shape[0] - 1)
        xs = np.clip(np.arange(p.left, p.left + p.cw), 0, a.shape[1] - 1)
        return Image.fromarray(np.ascontiguousarray(a[ys][:, xs]))

    @staticmethod
    def _hsv(img: Image.Image, hue: float, saturation: float, exposure: float) -> Image.Image:
        hsv = np.array(img.convert("HSV"), dtype=np.uint8)
        hsv[..., 0] = (hsv[..., 0].astype(np.int16) + int(hue * 255)) % 256
        for c, f in ((1, saturation), (2, exposure)):
            hsv[..., c] = np.minimum(np.float32(255), np.trunc(hsv[..., c].astype(np.float32) * np.float32(f))).astype(np.uint8)
        return Image.fromarray(hsv, "HSV").convert("RGB")

    def geometry(self, image: Image.Image, p: JitterParams) -> Image.Image:
        """window, PIL bilinear resize, flip"""
        image = self._window(image, p).resize((self.size[1], self.size[0]), Image.BILINEAR)
        return image.transpose(Image.FLIP_LEFT_RIGHT) if p.flip else image

    def apply(self, image: Image.Image, boxes: List[List[float]], p: JitterParams):
        """The host path: window, PIL bilinear resize, flip, the HSV round trip; boxes go with the window and the flip (the ones
        ``jitter_boxes`` keeps)."""
        image = self._hsv(self.geometry(image, p), p.hue, p.saturation, p.exposure)
        return image, jitter_boxes(boxes, p, self.size)[0]

    def __call__(self, image: Image.Image, boxes: List[List[float]]):
        return self.apply(image, boxes, self.sample(*image.size))


RECIPES = {"reference": _Augment, "darknet": _DarknetAugment}


class VOCDetectionYOLO(Dataset):
    """PASCAL VOC detection samples as (image tensor (3, H, W), target (S, S, 5B+C)); reference dataset.py:16-588."""

    VOC_CLASSES = VOC_CLASSES
    split_paths = {
        "2007": {"trainval": "VOCtrainval_06-Nov-2007", "test": "VOCtest_06-Nov-2007", "train": "VOCtrainval_06-Nov-2007",
                 "val": "VOCtrainval_06-Nov-2007"},
        "2012": {"trainval": "VOCtrainval_11-May-2012", "test": "VOCtest_11-May-2012", "train": "VOCtrainval_11-May-2012",
                 "val": "VOCtrainval_11-May-2012"},
    }

    @staticmethod
    def download_from_kaggle(year: str = "2007", verbose: bool = True):
        raise ImportError("download_from_kaggle needs kagglehub and a network connection; place the dataset under `root` "
                          "(VOCdevkit/VOC<year>/...) and pass download=False")

    def __init__(self, root: str | Path = None, year: str = "2007", image_set: str = "train", download: bool = False, S: int = 7, B: int = 2,
                 transform=None, target_size: Tuple[int, int] = (448, 448), augment: bool = True, device_transform: bool = False,
                 recipe: str = "reference"):
        self.S, self.B = S, B
        # recipe: the training augmentation -- "reference" (_Augment, the reference's) or "darknet" (_DarknetAugment, the paper's)
        if recipe not in RECIPES:
            raise ValueError(f"recipe must be one of {sorted(RECIPES)}, not {recipe!r}")
        self.recipe = recipe
        # device_transform: __getitem__ returns (decoded uint8 HWC tensor, AugParams or JitterParams, target) for yolo.augment.collate_u8 -- the crop,
        # resize, colour jitter and normalisation then run on the device (yolo_augment_u8) with the very parameters drawn here
        if device_transform and transform is not None:
            raise ValueError("device_transform=True cannot run a custom `transform` on the device")
        self.device_transform = device_transform
        self.C = len(self.VOC_CLASSES)
        self.target_size = target_size
        self.augment = augment and image_set == "train"            # only the training split is augmented (dataset.py:190)
        self.class_to_idx = {n: i for i, n in enumerate(self.VOC_CLASSES)}
        self.class_names = self.VOC_CLASSES
        if download:
            self.download_from_kaggle(year.split("-")[0])
        if root is None:
            raise FileNotFoundError("VOCDetectionYOLO needs `root` (the dataset cannot be downloaded offline)")
        base_year = year.split("-")[0]
        root = Path(root)
        cands = [root / self.split_paths[base_year][image_set] / "VOCdevkit" / f"VOC{base_year}", root / "VOCdevkit" / f"VOC{base_year}",
                 root / f"VOC{base_year}", root]
        self.voc_dir = next((c for c in cands if (c / "ImageSets" / "Main" / f"{image_set}.txt").is_file()), None)
        if self.voc_dir is None:
            raise FileNotFoundError(f"no ImageSets/Main/{image_set}.txt for VOC{base_year} under {root} (looked in: "
                                    + ", ".join(str(c) for c in cands) + ")")
        with open(self.voc_dir / "ImageSets" / "Main" / f"{image_set}.txt") as f:
            self.ids = [ln.split()[0] for ln in f if ln.strip()]
        if transform is not None:
            self.transform = transform
        elif self.augment:
            self.transform = self._get_augmentation_transforms()
        else:
            from .inference import _Preprocess
            self.transform = _Preprocess(size=target_size)
        from .inference import _Preprocess
        self._finish = _Preprocess(size=target_size)                # ToTensor + Normalize (the resize is a no-op after the crop)

    def _get_augmentation_transforms(self):
        return RECIPES[self.recipe](self.target_size)

    def __len__(self) -> int:
        return len(self.ids)

    def _load(self, idx: int):
        name = self.ids[idx]
        image = Image.open(self.voc_dir / "JPEGImages" / f"{name}.jpg").convert("RGB")
        annotation = parse_voc_xml(ET.parse(self.voc_dir / "Annotations" / f"{name}.xml").getroot())
        return image, annotation

    def _augmented_target(self, annotation: dict, w: int, h: int, p) -> torch.Tensor:
        """target of a training sample whose image is cropped by ``p`` (the host and the device path alike); under ``JitterParams`` the
        boxes that ``jitter_boxes`` drops lose their class ids too"""
        bboxes, class_ids = self._extract_bboxes_from_annotation(annotation)
        pix = [[(x - bw / 2) * w, (y - bh / 2) * h, (x + bw / 2) * w, (y + bh / 2) * h] for x, y, bw, bh in bboxes]
        if isinstance(p, JitterParams):
            pix, kept = jitter_boxes(pix, p, self.target_size)
            class_ids = [class_ids[i] for i in kept]
        else:
            pix = crop_boxes(pix, p, self.target_size)
        H, W = self.target_size
        norm = []
        for x0, y0, x1, y1 in pix:
            clamp = lambda v: max(0, min(1, v))   # noqa: E731
            norm.append([clamp(((x0 + x1) / 2) / W), clamp(((y0 + y1) / 2) / H), clamp((x1 - x0) / W), clamp((y1 - y0) / H)])
        return self._encode_target(norm, class_ids)

    def __getitem__(self, idx: int):
        image, annotation = self._load(idx)
        w, h = image.size
        augmented = self.augment and isinstance(self.transform, (_Augment, _DarknetAugment))
        if self.device_transform:
            p = self.transform.sample(w, h) if augmented else AugParams(0, 0, h, w)
            target = self._augmented_target(annotation, w, h, p) if augmented else self._parse_voc_annotation(annotation)
            return torch.from_numpy(np.asarray(image, dtype=np.uint8).copy()), p, target
        if augmented:
            p = self.transform.sample(w, h)
            image, _ = self.transform.apply(image, [], p)
            return self._finish(image), self._augmented_target(annotation, w, h, p)
        return self.transform(image), self._parse_voc_annotation(annotation)

    # ---- annotation handling: same names / arguments / results as the reference (dataset.py:411-532)
    def _extract_bboxes_from_annotation(self, annotation: dict):
        size = annotation["annotation"]["size"]
        iw, ih = float(size["width"]), float(size["height"])
        objects = annotation["annotation"].get("object", [])
        if not isinstance(objects, list):
            objects = [objects]
        bboxes, class_ids = [], []
        for obj in objects:
            if obj["name"] not in self.class_to_idx:
                continue
            bb = obj["bndbox"]
            xmin, ymin, xmax, ymax = float(bb["xmin"]), float(bb["ymin"]), float(bb["xmax"]), float(bb["ymax"])
            vals = [((xmin + xmax) / 2.0) / iw, ((ymin + ymax) / 2.0) / ih, (xmax - xmin) / iw, (ymax - ymin) / ih]
            bboxes.append([max(0, min(1, v)) for v in vals])
            class_ids.append(self.class_to_idx[obj["name"]])
        return bboxes, class_ids

    def _parse_voc_annotation(self, annotation: dict) -> torch.Tensor:
        return self._encode_target(*self._extract_bboxes_from_annotation(annotation))

    def _encode_target(self, bboxes: list, class_ids: list) -> torch.Tensor:
        return encode_target(bboxes, class_ids, self.S, self.B, self.C)

    def ground_truth(self, idx: int) -> dict:
        """What the annotation file says, for the devkit's evaluation (yolo/voc_eval.py): every object with a known class name -- also the
        ones that share a grid cell, which the target tensor cannot hold -- as pixel corners, with its ``difficult`` flag (0 where the tag
        is missing).  Reads the XML only; the image is not opened."""
        root = ET.parse(self.voc_dir / "Annotations" / f"{self.ids[idx]}.xml").getroot()
        size = root.find("size")
        boxes, class_ids, difficult = [], [], []
        for obj in root.iter("object"):
            name = (obj.findtext("name") or "").strip()
            if name not in self.class_to_idx:
                continue
            bb = obj.find("bndbox")
            boxes.append([float(bb.findtext(k)) for k in ("xmin", "ymin", "xmax", "ymax")])
            class_ids.append(self.class_to_idx[name])
            difficult.append(int((obj.findtext("difficult") or "0").strip() or 0) != 0)
        return {"image_id": self.ids[idx], "width": int(float(size.findtext("width"))), "height": int(float(size.findtext("height"))),
                "boxes": np.array(boxes, np.float64).reshape(-1, 4), "class_ids": np.array(class_ids, np.int64),
                "difficult": np.array(difficult, bool)}

    def visualize_sample(self, idx: int) -> dict:
        image, annotation = self._load(idx)
        bboxes, class_ids = self._extract_bboxes_from_annotation(annotation)
        return {"image_path": str(self.voc_dir / "JPEGImages" / f"{self.ids[idx]}.jpg"), "image_size": image.size, "bboxes": bboxes,
                "class_ids": class_ids, "class_names": [self.class_names[c] for c in class_ids], "num_objects": len(bboxes)}


class CombinedVOCDataset(Dataset):
    """Concatenation of several VOCDetectionYOLO datasets with identical S / B / C (dataset.py:590-659)."""

    def __init__(self, datasets: list):
        self.datasets = datasets
        self.lengths = [len(ds) for ds in datasets]
        self.cumulative_lengths = np.cumsum([0] + self.lengths).tolist()
        if datasets:
            first = datasets[0]
            self.S, self.B, self.C = first.S, first.B, first.C
            self.class_names, self.class_to_idx = first.class_names, first.class_to_idx
            for ds in datasets[1:]:
                assert ds.S == self.S, f"All datasets must have same S (grid size): {self.S} != {ds.S}"
                assert ds.B == self.B, f"All datasets must have same B (boxes per cell): {self.B} != {ds.B}"
                assert ds.C == self.C, f"All datasets must have same C (num classes): {self.C} != {ds.C}"

    def __len__(self) -> int:
        return sum(self.lengths)

    def __getitem__(self, idx: int):
        if idx < 0 or idx >= len(self):
            raise IndexError(f"Index {idx} out of range for dataset of size {len(self)}")
        k = int(np.searchsorted(self.cumulative_lengths, idx, side="right")) - 1
        return self.datasets[k][idx - self.cumulative_lengths[k]]

    def ground_truth(self, idx: int) -> dict:
        if idx < 0 or idx >= len(self):
            raise IndexError(f"Index {idx} out of range for dataset of size {len(self)}")
        k = int(np.searchsorted(self.cumulative_lengths, idx, side="right")) - 1
        return self.datasets[k].ground_truth(idx - self.cumulative_lengths[k])


def create_voc_datasets(years_and_splits: list, download: bool = True, S: int = 7, B: int = 2, target_size: Tuple[int, int] = (448, 448),
                        augment: bool = True, root: str | Path = None, device_transform: bool = False, recipe: str = "reference") -> Dataset:
    """One VOCDetectionYOLO, or their concatenation, for [(year, image_set), ...] (dataset.py:662-730).  Offline, ``download``
    is honoured only as "the data must already lie under root" (default root: $VOC_ROOT or ./data)."""
    if root is None:
        root = os.environ.get("VOC_ROOT", "data")
    datasets = [VOCDetectionYOLO(root=root, year=y, image_set=s, download=False, S=S, B=B, target_size=target_size, augment=augment,
                                 device_transform=device_transform, recipe=recipe)
                for y, s in years_and_splits]
    return datasets[0] if len(datasets) == 1 else CombinedVOCDataset(datasets)


# ------------------------------------------------------------------------------------------------------------------
# Classification pretraining (pretrain.py): image folders and a synthetic stand-in.  Extension of the reference surface.
# ------------------------------------------------------------------------------------------------------------------
IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".ppm", ".webp")


class _ClassifyTransform:
    """PIL image -> normalised (3, size, size) tensor.  Training: the geometry and colour of ``_Augment`` (no boxes) and a horizontal flip with
    probability 1/2, all drawn from torch's global generator; validation: the Resize of ``inference._Preprocess``.  Split like ``_Augment``:
    ``sample`` draws an ``AugParams`` (the flip in its ``flip`` field), ``apply`` is the host path, and the device path
    (``device_transform=True`` datasets -> ``yolo.augment.collate_u8`` -> yolo_augment_u8) takes the same parameters."""

    def __init__(self, size: int, train: bool):
        from .inference import _Preprocess
        self.train = train
        self.augment = _Augment((size, size)) if train else None
        self.finish = _Preprocess(size=(size, size))          # Resize (a no-op behind the crop) + ToTensor + Normalize

    def sample(self, w: int, h: int) -> AugParams:
        """training: ``_Augment.sample`` and then one ``rand`` for the flip; validation: the whole image, no operation, nothing drawn"""
        if not self.train:
            return AugParams(0, 0, h, w)
        p = self.augment.sample(w, h)
        return p._replace(flip=float(torch.rand(1).item()) < 0.5)

    def apply(self, image: Image.Image, p: AugParams) -> torch.Tensor:
        if self.train:
            image, _ = self.augment.apply(image, [], p)
        return self.finish(image)

    def __call__(self, image: Image.Image) -> torch.Tensor:
        return self.apply(image, self.sample(*image.size))


def _u8_sample(transform: _ClassifyTransform, image: Image.Image, label: int):
    """a ``device_transform`` sample for ``yolo.augment.collate_u8``: (decoded uint8 HWC tensor, AugParams, label tensor)"""
    return torch.from_numpy(np.asarray(image, dtype=np.uint8).copy()), transform.sample(*image.size), torch.tensor(label, dtype=torch.int64)


class ImageFolderClassification(Dataset):
    """``<root>/<split>/<class>/*`` image folders: the classes are the sorted directory names of the split, a sample is
    (normalised (3, size, size) tensor, class index).  Pillow only.  ``classes``: the class list of another split (the validation split of a
    training run uses the training split's indices; a directory it does not name is an error).  ``device_transform=True``: a sample is
    (decoded uint8 HWC tensor, AugParams, label tensor) for ``yolo.augment.collate_u8(samples, size=(size, size))`` -- crop, resize, colour
    jitter, flip and normalisation then run on the device with the very parameters drawn here."""

    def __init__(self, root: str | Path, split: str = "train", size: int = 224, train: bool | None = None, classes: List[str] | None = None,
                 device_transform: bool = False):
        self.device_transform = device_transform
        self.dir = Path(root) / split
        if not self.dir.is_dir():
            raise FileNotFoundError(f"no directory {self.dir}: expected <root>/{split}/<class>/<image files>")
        found = sorted(d.name for d in self.dir.iterdir() if d.is_dir())
        if not found:
            raise FileNotFoundError(f"{self.dir} holds no class directories")
        self.classes = list(classes) if classes is not None else found
        self.class_to_idx = {n: i for i, n in enumerate(self.classes)}
        unknown = [n for n in found if n not in self.class_to_idx]
        if unknown:
            raise ValueError(f"{self.dir}: class directories {unknown[:5]} are not among the given classes")
        self.samples = [(p, self.class_to_idx[n]) for n in found for p in sorted((self.dir / n).iterdir())
                        if p.suffix.lower() in IMAGE_EXTENSIONS]
        if not self.samples:
            raise FileNotFoundError(f"{self.dir} holds no images ({', '.join(IMAGE_EXTENSIONS)})")
        self.transform = _ClassifyTransform(size, split == "train" if train is None else train)

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, idx: int):
        path, label = self.samples[idx]
        image = Image.open(path).convert("RGB")
        if self.device_transform:
            return _u8_sample(self.transform, image, label)
        return self.transform(image), label


class SyntheticClassificationDataset(Dataset):
    """``length`` images of ``num_classes`` learnable classes without a dataset on disk: sample ``idx`` has class ``idx % num_classes``, and an image is
    its class's fixed low-resolution colour pattern (8 x 8 blocks, drawn once from ``seed``) plus per-sample noise (from ``(seed, idx)``), as
    uint8 RGB through the same Pillow transforms as the folder dataset -- or, with ``device_transform=True``, as the folder dataset's
    (uint8 HWC tensor, AugParams, label tensor) samples."""

    def __init__(self, length: int = 256, num_classes: int = 10, size: int = 224, seed: int = 0, train: bool = False, noise: float = 24.0,
                 device_transform: bool = False):
        self.device_transform = device_transform
        self.length, self.num_classes, self.size, self.seed, self.noise = length, num_classes, size, seed, noise
        rng = np.random.Generator(np.random.PCG64([seed, 1 << 20]))
        self.patterns = rng.integers(32, 224, (num_classes, 8, 8, 3)).astype(np.float32)
        self.transform = _ClassifyTransform(size, train)

    def __len__(self) -> int:
        return self.length

    def image(self, idx: int) -> Image.Image:
        rng = np.random.Generator(np.random.PCG64([self.seed, idx]))
        rep = -(-self.size // 8)
        base = np.kron(self.patterns[idx % self.num_classes], np.ones((rep, rep, 1), dtype=np.float32))[: self.size, : self.size]
        arr = base + rng.standard_normal(base.shape, dtype=np.float32) * self.noise
        return Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8), "RGB")

    def __getitem__(self, idx: int):
        if self.device_transform:
            return _u8_sample(self.transform, self.image(idx), idx % self.num_classes)
        return self.transform(self.image(idx)), idx % self.num_classes
