"""MI355X-native YOLOv1: the module surface of mattiaskvist/yolo-v1's ``src/yolo`` package
(``__all__`` = reference ``yolo/__init__.py:3-31``) on hand-written gfx950 HIP kernels."""

from .dataset import CombinedVOCDataset, VOCDetectionYOLO, create_voc_datasets
from .loss import YOLOLoss
from .metrics import evaluate_model, mAPMetric
from .models import YOLOv1, Backbone, DetectionHead, ResNetBackbone, YOLOv1Backbone
from .optim import ModelEMA  # noqa: F401  (weight EMA for training; the reference keeps none, so it stays out of __all__)
from .optim import GradAccumulator  # noqa: F401  (K micro-batches per optimizer step; likewise)
from .classify import GlobalAvgPool, SoftmaxCrossEntropy, YOLOv1Classifier  # noqa: F401  (classification pretraining of the trunk; likewise)
from .voc_eval import VOCGroundTruth, VOCMetric, evaluate_voc  # noqa: F401  (the VOC devkit's evaluation protocol; likewise)
from .schemas import BoundingBox, Detection

# north_star spellings as aliases of the reference's names
YoloLoss = YOLOLoss
from .compat import cellboxes_to_boxes, mean_average_precision, non_max_suppression  # noqa: E402,F401

__all__ = [
    "Backbone",
    "BoundingBox",
    "CombinedVOCDataset",
    "Detection",
    "DetectionHead",
    "ResNetBackbone",
    "VOCDetectionYOLO",
    "YOLOLoss",
    "YOLOv1",
    "YOLOv1Backbone",
    "create_voc_datasets",
    "evaluate_model",
    "mAPMetric",
]
