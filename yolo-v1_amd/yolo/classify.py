"""Classification pretraining of the YOLOv1 trunk: the stage the paper runs before detection training (section 2.2: the first 20
convolutions, an average pool and one fully connected layer, trained as a 224 x 224 classifier).

The reference (mattiaskvist/yolo-v1) has no such stage -- it loads torchvision's ImageNet weights into a ResNet-50 -- so this module extends
its surface: ``GlobalAvgPool``, ``SoftmaxCrossEntropy`` (shaped like ``YOLOLoss``: ``forward(logits, labels) -> (loss, parts)``) and
``YOLOv1Classifier``, whose ``features.N.*`` state-dict keys are ``YOLOv1Backbone``'s (``YOLOv1Backbone.load_pretrained`` takes them over).

Device tensors run on libyolo_hip.so (classify.hip): the pool and the loss are one autograd node each, the two conv / Linear stacks around
the pool are ordinary engine plans.  CPU tensors take stock torch ops -- an explicit device choice, never a fallback.
"""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip, engine
from ._hip import check, lib, ptr, stream
from .loss import _COPY_STREAMS, LossParts
from .models import YOLOv1Backbone, _BNFeatures, _load_features, _PlanOwner

TRUNK_CONVS = 20             # convolutions of YOLOv1Backbone that the classifier shares with the detector (the paper's count)
_KEYS = ("total", "top1", "top5")
_BAD_LABEL = "label out of bounds: a label lies outside [0, num_classes) (stock F.cross_entropy raises IndexError there)"


# ------------------------------------------------------------------------------------------------ global average pool
@_hip.device_guard
def gap_fwd(x: torch.Tensor) -> torch.Tensor:
    """(N, C, H, W) fp32 on the device -> (N, C, 1, 1): yolo_gap_fwd"""
    _hip.require_cuda(x)
    x = x.detach()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    N, C, H, W = x.shape
    y = torch.empty((N, C, 1, 1), dtype=torch.float32, device=x.device)
    check(lib().yolo_gap_fwd(ptr(x), N, C, H * W, ptr(y), stream()), "yolo_gap_fwd")
    return y


@_hip.device_guard
def gap_bwd(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """gradient (N, C, 1, 1) of the pooled map -> (N, C, H, W): yolo_gap_bwd"""
    _hip.require_cuda(dy)
    dy = dy.detach()
    if dy.dtype != torch.float32 or not dy.is_contiguous():
        dy = dy.float().contiguous()
    N, C = dy.shape[0], dy.shape[1]
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    check(lib().yolo_gap_bwd(ptr(dy), N, C, H * W, ptr(dx), stream()), "yolo_gap_bwd")
    return dx


class _GapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[2], x.shape[3])
        ctx.in_dtype = x.dtype
        return gap_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return gap_bwd(dy, *ctx.hw).to(ctx.in_dtype)


class GlobalAvgPool(nn.Module):
    """``x.mean((2, 3), keepdim=True)``: (N, C, H, W) -> (N, C, 1, 1).  Device tensors: one autograd node on yolo_gap_fwd / yolo_gap_bwd."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4:
            raise RuntimeError(f"GlobalAvgPool expects (N, C, H, W), got {tuple(x.shape)}")
        if x.is_cuda:
            return _GapFn.apply(x)
        return x.mean((2, 3), keepdim=True)


# ------------------------------------------------------------------------------------------------ softmax cross-entropy
@_hip.device_guard
def softmax_xent_fwd_bwd(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float, want_grad: bool = True):
    """Fused loss, gradient and top-1 / top-5 hits (yolo_softmax_xent_fwd_bwd).  Returns (out [2] fp32 = {mean loss, error flag},
    dlogits or None, hits (N, 2) int32), all on the device."""
    _hip.require_cuda(logits, labels)
    logits = logits.detach().to(torch.float32).contiguous()
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
        # the kernel cannot know the buffers' extents
        raise RuntimeError(f"SoftmaxCrossEntropy: logits {tuple(logits.shape)} / labels {tuple(labels.shape)} must be (N, K) and (N,)")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise RuntimeError(f"SoftmaxCrossEntropy: labels must be class indices, got {labels.dtype}")
    labels = labels.detach().to(torch.int64).contiguous()
    N, K = logits.shape
    dev = logits.device
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits) if want_grad else None
    hits = torch.empty((N, 2), dtype=torch.int32, device=dev)
    work = torch.empty((max(N, 1),), dtype=torch.float64, device=dev)
    check(lib().yolo_softmax_xent_fwd_bwd(ptr(logits), ptr(labels), N, K, float(label_smoothing), ptr(out), ptr(dlogits), ptr(hits), ptr(work),
                                          stream()), "yolo_softmax_xent_fwd_bwd")
    return out, dlogits, hits


def topk_hits(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """(N, 2) int32 {top-1, top-5} in stock torch ops, the kernel's rule: a hit at k = fewer than k logits of the row are strictly greater
    than the label's.  A label outside [0, K) never hits."""
    K = logits.shape[1]
    valid = (labels >= 0) & (labels < K)
    xy = logits.gather(1, labels.clamp(0, K - 1).unsqueeze(1))
    above = (logits > xy).sum(1)
    return torch.stack([(above < 1) & valid, (above < 5) & valid], 1).to(torch.int32)


class _HipXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, eps):
        out, dlogits, hits = softmax_xent_fwd_bwd(logits, labels, eps, want_grad=ctx.needs_input_grad[0])
        ctx.dlogits = dlogits
        ctx.in_dtype = logits.dtype
        ctx.mark_non_differentiable(out, hits)
        return out[0].clone(), out, hits

    @staticmethod
    def backward(ctx, g_total, _g_out, _g_hits):
        d = ctx.dlogits
        ctx.dlogits = None
        if d is None:
            return None, None, None
        return (d * g_total).to(ctx.in_dtype), None, None


class ClassifyParts(LossParts):
    """``{"total", "top1", "top5"}`` as Python floats (the mean loss and the top-1 / top-5 accuracy of the batch), fetched when first READ:
    the mechanism of ``yolo.loss.LossParts`` -- a side stream copies the kernel's results to pinned host memory behind the loss kernel, reading
    waits for that copy only.  A label outside [0, num_classes) raises RuntimeError at that first read; ``device_flag`` is the kernel's error
    word on the device (one float32), which ``optimizer.skip_if`` takes so that such a step updates nothing."""

    def __init__(self, event, host_out, host_hits, device_flag=None):
        dict.__init__(self, ((k, None) for k in _KEYS))
        self._pending = (event, (host_out, host_hits))
        self.device_flag = device_flag

    def _fetch(self):
        if self._pending is not None:
            event, (host_out, host_hits) = self._pending
            self._pending = None
            if event is not None:
                event.synchronize()
            total, flag = host_out.tolist()
            if flag != 0.0:
                raise RuntimeError(_BAD_LABEL)
            n = max(host_hits.shape[0], 1)
            top = host_hits.sum(0).tolist()
            dict.update(self, {"total": total, "top1": top[0] / n, "top5": top[1] / n})
        return self

    def done(self) -> bool:
        return self._pending is None or self._pending[0] is None or self._pending[0].query()


class SoftmaxCrossEntropy(nn.Module):
    """``F.cross_entropy(logits, labels, label_smoothing=e)`` (mean over the batch) with the surface of ``YOLOLoss``:
    ``forward(logits, labels) -> (loss, parts)``, ``parts`` = ``{"total", "top1", "top5"}`` + ``device_flag`` (``ClassifyParts``).

    Device tensors: loss, gradient and hits come from ONE launch pair of yolo_softmax_xent_fwd_bwd, one autograd node, no host
    synchronisation inside ``forward``.  A row whose label lies outside [0, K) contributes nothing and raises the flag.
    CPU tensors: ``F.cross_entropy`` plus the same hit rule (``topk_hits``) and the same treatment of such rows."""

    def __init__(self, label_smoothing: float = 0.0):
        super().__init__()
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
        self.label_smoothing = float(label_smoothing)
        self._last_parts = None

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        if not logits.is_cuda:
            return self._forward_cpu(logits, labels)
        prev, self._last_parts = self._last_parts, None
        if prev is not None and prev._pending is not None and prev.done():
            prev._fetch()              # a dict nobody read: its error flag must not get lost (no wait: the copy has landed)
        total, out, hits = _HipXentFn.apply(logits, labels, self.label_smoothing)
        dev = out.device
        cs = _COPY_STREAMS.get(dev.index)
        if cs is None:
            cs = _COPY_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
        cs.wait_stream(torch.cuda.current_stream(dev))          # behind the loss kernel; nothing of the backward pass is queued yet
        host_out = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        host_hits = torch.empty(hits.shape, dtype=hits.dtype, pin_memory=True)
        with torch.cuda.stream(cs):
            host_out.copy_(out, non_blocking=True)
            host_hits.copy_(hits, non_blocking=True)
            event = torch.cuda.Event()
            event.record(cs)
        out.record_stream(cs)
        hits.record_stream(cs)
        parts = ClassifyParts(event, host_out, host_hits, out[1:2])
        self._last_parts = parts
        return total, parts

    def _forward_cpu(self, logits: torch.Tensor, labels: torch.Tensor):
        N, K = logits.shape
        valid = (labels >= 0) & (labels < K)
        if bool(valid.all()):
            total = F.cross_entropy(logits, labels, label_smoothing=self.label_smoothing)
        else:
            rows = F.cross_entropy(logits, labels.clamp(0, K - 1), label_smoothing=self.label_smoothing, reduction="none")
            total = (rows * valid.to(rows.dtype)).sum() / N
        flag = torch.tensor([0.0 if bool(valid.all()) else 1.0], dtype=torch.float32)
        host_out = torch.stack([total.detach().float(), flag[0]])
        return total, ClassifyParts(None, host_out, topk_hits(logits.detach(), labels), flag)


# ------------------------------------------------------------------------------------------------ the classifier
def trunk_cut(features, convs: int = TRUNK_CONVS) -> int:
    """number of leading modules of ``features`` up to and including the [BatchNorm2d and] LeakyReLU behind its ``convs``-th Conv2d"""
    seen = 0
    for i, m in enumerate(features):
        if isinstance(m, nn.Conv2d):
            seen += 1
            if seen == convs:
                j = i + 1
                if j < len(features) and isinstance(features[j], nn.BatchNorm2d):
                    j += 1
                return j + 1 if (j < len(features) and isinstance(features[j], nn.LeakyReLU)) else j
    raise ValueError(f"features hold {seen} convolutions, fewer than {convs}")


class YOLOv1Classifier(_PlanOwner, nn.Module):
    """The pretraining network of the YOLOv1 paper: the first 20 convolutions of ``YOLOv1Backbone`` (same modules, same indices:
    ``features.N.*``), a global average pool and ``Linear(1024, num_classes)``.  (N, 3, H, W) -> (N, num_classes) logits; H and W are
    free (224 in the paper).

    Device tensors: two engine plans -- the conv / pool trunk and [Flatten, Linear] -- with the ``GlobalAvgPool`` node between them;
    ``hip_plans()`` lists them in forward order, which is how ``parallel.make_grad_reducer`` and ``yolo.optim.GradAccumulator`` find them."""

    def __init__(self, num_classes: int = 1000, batch_norm: bool = False):
        super().__init__()
        self.num_classes = num_classes
        self.batch_norm = bool(batch_norm)
        full = (YOLOv1Backbone(batch_norm=True) if self.batch_norm else YOLOv1Backbone()).features
        self.features = nn.Sequential(*list(full)[:trunk_cut(full)])
        self._bn = _BNFeatures(self.features) if self.batch_norm else None
        self.pool = GlobalAvgPool()
        self.fc = nn.Linear(1024, num_classes)
        self._flatten = nn.Flatten()
        self._trunk_plan: engine.Plan | None = None
        self._plan: engine.Plan | None = None        # the plan with the Linear layer: the one _PlanOwner.__deepcopy__ waits for

    def trunk_plan(self) -> engine.Plan:
        """the plan of the plain trunk; with batch_norm=True, of the trunk with its BatchNorm layers folded in (inference)"""
        if self.batch_norm:
            mods, fresh = self._bn.folded()
            if self._trunk_plan is None or fresh:
                self._trunk_plan = engine.Plan.from_modules(mods, 3, True)
            return self._own(self._trunk_plan)
        if self._trunk_plan is None:
            self._trunk_plan = engine.Plan.from_modules(self.features, 3, True)
        return self._own(self._trunk_plan)

    def head_plan(self) -> engine.Plan:
        if self._plan is None:
            self._plan = engine.Plan.from_modules([self._flatten, self.fc], 1024, False)
        return self._own(self._plan)

    def hip_plans(self) -> list:
        """the plans a training step updates; a BatchNorm trunk is none of them: its parameters travel through autograd (engine.BNPlan)"""
        if self.batch_norm:
            return [self.head_plan()]
        return [self.trunk_plan(), self.head_plan()]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (N, 3, H, W) fp32 images, or a ``yolo.augment.U8Batch`` (decoded uint8 images + crop / colour / flip parameters): on the device
        it is augmented straight into the trunk plan's stem input buffer, as ``YOLOv1.forward`` does; on the CPU its fp32 tensor is taken"""
        if x.is_cuda:
            if self.batch_norm and self._bn.wants_train_path(self.training):
                f = engine.run_bn_plan(self._bn.train_plan(), x, self.training)
            else:
                f = engine.run_plan(self.trunk_plan(), x, self.training and not self.batch_norm)
            return engine.run_plan(self.head_plan(), self.pool(f), self.training)
        if not isinstance(x, torch.Tensor):
            x = x.to_tensor()
        return self.fc(self._flatten(self.pool(self.features(x))))
