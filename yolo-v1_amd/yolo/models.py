"""Model surface of the reference (src/yolo/models.py) with the HIP engine underneath.

Module classes, constructor signatures, attribute names and ``state_dict`` keys are the reference's
(SURVEY.md 8b): the fp32 parameters live in ordinary ``nn.Conv2d`` / ``nn.Linear`` children
(``backbone.features.N``, ``head.1`` / ``head.4``, ``head.conv_layers.N`` / ``head.fc_layers.N``) so
checkpoints written by the reference load unchanged.  What differs is ``forward``:

  * device tensors never reach those children -- a whole conv/pool/FC stack runs as ONE autograd node
    on libyolo_hip.so (engine.Plan): zero-haloed NHWC bf16 activations, MFMA implicit-GEMM convs with
    fused bias + LeakyReLU(0.1), fp32 accumulation;
  * CPU tensors take the stock ``torch.nn`` path -- the reference's own ``--device cpu`` behaviour
    (an explicit device choice, not a fallback: a device tensor without the HIP library raises).
"""

from __future__ import annotations

import copy
import weakref

import torch
import torch.nn as nn

from . import engine
from .config import CONFIG
from .conv_bn import _ConvBNBase


BN_STATS_NOT_DETERMINISTIC = ("EngineConfig.DETERMINISTIC does not cover the ResNet trunk in training mode: its BatchNorm batch statistics are summed with "
                              "fp64 atomics (bn.hip, the bn_stats epilogues of the conv kernels).  Put the trunk in eval() mode (running statistics; the "
                              "DetectionHead behind it is covered), or use --backbone yolov1")


class _PlanOwner:
    """mix-in of the modules that own an engine plan: the plan knows its owner (hooks of yolo.optim.Adam.attach_plan(overlap=True)),
    and a deep copy of the module first waits for a background update of its Linear layers still running on a second stream
    (the copy reads every parameter on the current stream)."""

    def _own(self, plan: "engine.Plan") -> "engine.Plan":
        plan.owner = weakref.ref(self)
        return plan

    def __deepcopy__(self, memo):
        plan = self.__dict__.get("_plan")
        if isinstance(plan, engine.Plan):
            plan.params_ready.wait(keep=True)
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__(copy.deepcopy(self.__dict__, memo))       # what copy.deepcopy does for an nn.Module without this method
        return new


@torch.no_grad()
def init_kaiming_(module: nn.Module) -> int:
    """He initialisation for the LeakyReLU(0.1) stacks of this file, in place: every ``nn.Conv2d`` and every ``nn.Linear`` of ``module`` gets
    ``kaiming_normal_(a=0.1, mode="fan_in", nonlinearity="leaky_relu")`` and a zero bias -- except the module's LAST Linear (the logits, the
    detection output), which keeps what it has: nothing follows it, so its scale does not compound.  The draws come from torch's global
    generator in ``module.modules()`` order.  Returns the number of tensors written.

    Why: PyTorch's default (``kaiming_uniform_(a=sqrt(5))``, the reference's initialisation) scales the signal by about 0.4 per
    conv + LeakyReLU(0.1) layer, and these networks have no normalisation layers: behind 20 layers the input-dependent part of the activations
    is ~1e-8 of the first layer's, far below the bf16 resolution of the bias term it rides on, and nothing is learnt (DESIGN.md,
    "Classification pretraining").  Extension of the reference surface; call it before the model moves to its device."""
    linears = [m for m in module.modules() if isinstance(m, nn.Linear)]
    last = linears[-1] if linears else None
    written = 0
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)) and m is not last:
            nn.init.kaiming_normal_(m.weight, a=0.1, mode="fan_in", nonlinearity="leaky_relu")
            written += 1
            if m.bias is not None:
                nn.init.zeros_(m.bias)
                written += 1
    return written


class Backbone(nn.Module):
    """Abstract feature extractor: subclasses map (N,3,H,W) images to (N,C,H',W') features."""

    def __init__(self):
        super().__init__()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("Subclasses must implement forward method")


def _conv_act(cin: int, cout: int, k: int, stride: int = 1, pad: int = 0, bn: bool = False) -> list[nn.Module]:
    if bn:          # Darknet's batch_normalize=1: the conv has no bias, BatchNorm's shift takes its place
        return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.1)]
    return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad), nn.LeakyReLU(0.1)]


class _BNFeatures:
    """How a ``features`` stack with BatchNorm layers runs on the device (``YOLOv1Backbone(batch_norm=True)``, ``YOLOv1Classifier(.., batch_norm=True)``):
    with gradients, the training executor ``engine.BNPlan`` (batch statistics in train(), running statistics in eval()); without, the BatchNorm layers
    folded into plain ``[Conv2d(bias), LeakyReLU, MaxPool2d]`` modules that the ordinary ``engine.Plan`` runs -- same shapes, same launch table as the
    plain network.  The folded modules are shadows outside the module tree (no state-dict keys); they are refreshed when a parameter's or buffer's
    ``_version`` changes, as the folded operands of ``ResNetPlan.forward`` are."""

    def __init__(self, features: nn.Sequential):
        self.features = features
        self.bn_plan: "engine.BNPlan | None" = None
        self._shadow: list | None = None         # the folded plain modules, in order
        self._pairs: list = []                   # (conv, bn, shadow conv)
        self._ver = None

    def wants_train_path(self, training: bool) -> bool:
        """train(): batch statistics, whether or not gradients are recorded; eval(): only a forward that records gradients needs the kept z"""
        return training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.features.parameters()))

    def train_plan(self) -> "engine.BNPlan":
        if self.bn_plan is None:
            self.bn_plan = engine.BNPlan.from_modules(self.features)
        return self.bn_plan

    def folded(self) -> tuple[list, bool]:
        """(the folded plain modules with the current parameters and running statistics, whether the module objects are new)"""
        mods = list(self.features)
        dev = mods[0].weight.device
        fresh = self._shadow is None or self._pairs[0][2].weight.device != dev
        if fresh:
            self._shadow, self._pairs, self._ver = [], [], None
            i = 0
            while i < len(mods):
                m = mods[i]
                if isinstance(m, nn.Conv2d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d):
                    sh = nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, bias=True, device="meta")
                    sh = sh.to_empty(device=dev).requires_grad_(False)
                    self._pairs.append((m, mods[i + 1], sh))
                    self._shadow.append(sh)
                    i += 2
                else:
                    self._shadow.append(m)
                    i += 1
        ver = tuple(int(t._version) for t in self.features.parameters()) + tuple(int(b._version) for b in self.features.buffers())
        if ver != self._ver:
            with torch.no_grad():
                for conv, bn, sh in self._pairs:
                    w, b = _ConvBNBase._fold(conv, bn)
                    sh.weight.copy_(w)
                    sh.bias.copy_(b)
            self._ver = ver
        return self._shadow, fresh


def _load_features(module: nn.Module, state_dict, what: str) -> int:
    """copy every ``features.*`` entry of ``state_dict`` into the parameter or buffer of that name; all or nothing"""
    own = dict(module.named_parameters())
    own.update(dict(module.named_buffers()))
    todo = []
    for key, src in state_dict.items():
        if not key.startswith("features."):
            continue
        dst = own.get(key)
        if dst is None:
            raise KeyError(f"load_pretrained: {key} is not a parameter or buffer of {what}")
        if tuple(dst.shape) != tuple(src.shape):
            raise ValueError(f"load_pretrained: {key} has shape {tuple(src.shape)} in the checkpoint, the backbone expects {tuple(dst.shape)}")
        todo.append((dst, src))
    for dst, src in todo:          # nothing is copied unless everything fits
        dst.copy_(src)
    return len(todo)


class YOLOv1Backbone(_PlanOwner, Backbone):
    """The 24-convolution network of the YOLOv1 paper: 448x448x3 -> 7x7x1024.

    Layer list = src/yolo/models.py:47-84 of the reference (indices inside ``features`` are part of
    the checkpoint contract)."""

    def __init__(self, batch_norm: bool = False):
        super().__init__()
        self.batch_norm = bool(batch_norm)
        if self.batch_norm:
            self._init_bn()
            return
        mods: list[nn.Module] = []
        mods += _conv_act(3, 64, 7, 2, 3) + [nn.MaxPool2d(2, 2)]
        mods += _conv_act(64, 192, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += _conv_act(192, 128, 1) + _conv_act(128, 256, 3, 1, 1) + _conv_act(256, 256, 1) + _conv_act(256, 512, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += self._make_conv_block(512, 256, 512, 4)
        mods += _conv_act(512, 512, 1) + _conv_act(512, 1024, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += self._make_conv_block(1024, 512, 1024, 2)
        mods += _conv_act(1024, 1024, 3, 1, 1) + _conv_act(1024, 1024, 3, 2, 1)
        mods += _conv_act(1024, 1024, 3, 1, 1) + _conv_act(1024, 1024, 3, 1, 1)
        self.features = nn.Sequential(*mods)
        self._plan: engine.Plan | None = None

    def _init_bn(self):
        """the same 24 convolutions with ``Conv2d(bias=False), BatchNorm2d, LeakyReLU(0.1)`` in place of ``Conv2d, LeakyReLU(0.1)`` (Darknet's
        yolov1.cfg: batch_normalize=1 on every convolution); the pools stay where they are.  Extension of the reference surface."""
        ca = lambda *a: _conv_act(*a, bn=True)      # noqa: E731
        mods: list[nn.Module] = []
        mods += ca(3, 64, 7, 2, 3) + [nn.MaxPool2d(2, 2)]
        mods += ca(64, 192, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += ca(192, 128, 1) + ca(128, 256, 3, 1, 1) + ca(256, 256, 1) + ca(256, 512, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += self._make_conv_block(512, 256, 512, 4, True)
        mods += ca(512, 512, 1) + ca(512, 1024, 3, 1, 1) + [nn.MaxPool2d(2, 2)]
        mods += self._make_conv_block(1024, 512, 1024, 2, True)
        mods += ca(1024, 1024, 3, 1, 1) + ca(1024, 1024, 3, 2, 1)
        mods += ca(1024, 1024, 3, 1, 1) + ca(1024, 1024, 3, 1, 1)
        self.features = nn.Sequential(*mods)
        self._plan = None
        self._bn = _BNFeatures(self.features)

    def _make_conv_block(self, in_channels: int, mid_channels: int, out_channels: int, num_blocks: int, bn: bool = False) -> list[nn.Module]:
        """``num_blocks`` x [1x1 reduce -> 3x3 expand], each followed by LeakyReLU(0.1)."""
        out: list[nn.Module] = []
        for _ in range(num_blocks):
            out += _conv_act(in_channels, mid_channels, 1, bn=bn) + _conv_act(mid_channels, out_channels, 3, 1, 1, bn=bn)
            in_channels = out_channels
        return out

    def hip_plan(self) -> engine.Plan:
        """the plan of the plain stack; with batch_norm=True, of the stack with its BatchNorm layers folded in (inference)"""
        if self.batch_norm:
            mods, fresh = self._bn.folded()
            if self._plan is None or fresh:
                self._plan = engine.Plan.from_modules(mods, 3, True)
            return self._own(self._plan)
        if self._plan is None:
            self._plan = engine.Plan.from_modules(self.features, 3, True)
        return self._own(self._plan)

    @torch.no_grad()
    def load_pretrained(self, state_dict) -> int:
        """Take over the trunk of a classification checkpoint (``yolo.classify.YOLOv1Classifier``, pretrain.py): every
        ``features.N.weight`` / ``features.N.bias`` of ``state_dict`` is copied into layer N of this backbone; its other entries (the classifier's
        ``fc.*``) are ignored, and the layers the checkpoint does not hold -- the four convolutions detection adds -- stay as initialised.
        A tensor of another shape, or a layer this backbone does not have, raises naming the key.  Returns the number of tensors loaded
        (40 for the paper's 20 convolutions; 120 with batch_norm=True: 20 conv weights + 20 x (weight, bias, running_mean, running_var,
        num_batches_tracked)).  A plain checkpoint into a BatchNorm backbone, or the reverse, raises naming the first key that does not fit.
        Extension of the reference surface, which pretrains nothing."""
        return _load_features(self, state_dict, f"YOLOv1Backbone(batch_norm={self.batch_norm})")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            if self.batch_norm and self._bn.wants_train_path(self.training):
                return engine.run_bn_plan(self._bn.train_plan(), x, self.training)
            return engine.run_plan(self.hip_plan(), x, self.training and not self.batch_norm)
        if not isinstance(x, torch.Tensor):
            x = x.to_tensor()
        return self.features(x)


class ResNetBackbone(Backbone):
    """ResNet50 trunk up to layer4 (2048 x 14 x 14 for 448 x 448 inputs), reference src/yolo/models.py:131-176.

    The reference wraps ``torchvision.models.resnet50``; torchvision is an un-vendored dependency, so the
    trunk is restated in ``yolo.resnet`` with torchvision's module names (``extractor.N...`` state_dict keys
    are the reference's).  ``pretrained=True`` needs the ImageNet weights, i.e. torchvision + a download.
    Device tensors run on the HIP engine: eval mode with BatchNorm folded and the residual add fused, training mode
    (frozen backbone) with batch-statistics BatchNorm; a trainable trunk keeps every unit's conv output and runs the backward pass
    on the device in both modes (batch statistics in train(), running statistics in eval())."""

    def __init__(self, pretrained: bool = True, freeze: bool = True):
        super().__init__()
        from .resnet import resnet50_trunk
        trunk = resnet50_trunk()
        if pretrained:
            try:
                from torchvision.models import ResNet50_Weights, resnet50
            except ImportError as e:
                raise ImportError("ResNetBackbone(pretrained=True) needs torchvision's ImageNet weights; "
                                  "use pretrained=False or load a checkpoint") from e
            tv = nn.Sequential(*list(resnet50(weights=ResNet50_Weights.DEFAULT).children())[:-2])
            trunk.load_state_dict(tv.state_dict())
        if freeze:
            for p in trunk.parameters():
                p.requires_grad = False
        self.extractor = trunk
        self._plan = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            if self.training and CONFIG.DETERMINISTIC:
                raise NotImplementedError(BN_STATS_NOT_DETERMINISTIC)
            if self._plan is None:
                self._plan = engine.ResNetPlan(self.extractor)
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                # trainable trunk: in training mode -- the reference's default run (src/train.py:144) -- BatchNorm normalises with batch
                # statistics; in eval() mode with the running statistics as they are (stock autograd through batch_norm(training=False))
                return engine.ResNetTrainFunction.apply(self._plan, not self.training, x, *self.extractor.parameters())
            if self.training:
                # frozen but in training mode: BatchNorm uses batch statistics and updates its running statistics, exactly what
                # the reference does (freeze does not put BN in eval; trainer.py:49 calls model.train() on everything)
                return self._plan.forward_batch_stats(x)
            return self._plan.forward(x)
        return self.extractor(x)


class DetectionHead(_PlanOwner, nn.Module):
    """Conv + FC head used on top of ResNet50 features (src/yolo/models.py:279-348):
    4 x (3x3 conv + LeakyReLU), the second with stride 2 (14x14 -> 7x7), then
    Flatten -> Linear(1024*S*S, 4096) -> LeakyReLU -> Dropout(0.5) -> Linear(4096, S*S*(5B+C))."""

    def __init__(self, in_channels: int, num_classes: int = 20, S: int = 7, B: int = 2) -> None:
        super().__init__()
        self.num_classes, self.S, self.B = num_classes, S, B
        self.conv_layers = nn.Sequential(
            *_conv_act(in_channels, 1024, 3, 1, 1), *_conv_act(1024, 1024, 3, 2, 1),
            *_conv_act(1024, 1024, 3, 1, 1), *_conv_act(1024, 1024, 3, 1, 1))
        self.fc_layers = nn.Sequential(
            nn.Flatten(), nn.Linear(1024 * S * S, 4096), nn.LeakyReLU(0.1), nn.Dropout(0.5),
            nn.Linear(4096, S * S * (B * 5 + num_classes)))
        self._plan: engine.Plan | None = None
        self._in_channels = in_channels

    def hip_plan(self) -> engine.Plan:
        if self._plan is None:
            self._plan = engine.Plan.from_modules(list(self.conv_layers) + list(self.fc_layers), self._in_channels, False)
        return self._own(self._plan)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            y = engine.run_plan(self.hip_plan(), x, self.training)
        else:
            y = self.fc_layers(self.conv_layers(x))
        return y.view(-1, self.S, self.S, self.B * 5 + self.num_classes)


class YOLOv1(_PlanOwner, nn.Module):
    """Backbone + detection head -> (N, S, S, 5B + C) raw predictions (no output activation).

    ``YOLOv1()`` = YOLOv1Backbone + Flatten/Linear/LeakyReLU/Dropout/Linear head, exactly the
    reference's default (src/yolo/models.py:198-276).  For that configuration a device forward
    runs backbone and head as a single HIP plan (no NCHW fp32 round trip between them)."""

    def __init__(self, backbone: Backbone | None = None, detection_head: nn.Module | None = None,
                 num_classes: int = 20, S: int = 7, B: int = 2):
        super().__init__()
        self.num_classes, self.S, self.B = num_classes, S, B
        if backbone is None:
            backbone = YOLOv1Backbone()
        self.backbone = backbone
        if detection_head is None:
            if isinstance(backbone, YOLOv1Backbone):
                detection_head = nn.Sequential(
                    nn.Flatten(), nn.Linear(1024 * S * S, 4096), nn.LeakyReLU(0.1), nn.Dropout(0.5),
                    nn.Linear(4096, S * S * (B * 5 + num_classes)))
            elif isinstance(backbone, ResNetBackbone):
                detection_head = DetectionHead(2048, num_classes, S, B)
            else:
                raise ValueError("Must provide detection_head for custom backbone types")
        self.head = detection_head
        self._plan: engine.Plan | None = None
        self._head_plan: engine.Plan | None = None

    def _default_pair(self) -> bool:
        h = self.head
        return (type(self.backbone) is YOLOv1Backbone and type(h) is nn.Sequential and len(h) == 5
                and isinstance(h[0], nn.Flatten) and isinstance(h[1], nn.Linear) and isinstance(h[2], nn.LeakyReLU)
                and isinstance(h[3], nn.Dropout) and isinstance(h[4], nn.Linear))

    def _bn_backbone(self) -> bool:
        return type(self.backbone) is YOLOv1Backbone and self.backbone.batch_norm

    def _fusable(self) -> bool:
        """backbone and head as ONE plan: the default pair -- with a BatchNorm backbone only where its BatchNorm layers fold (no training path)"""
        return self._default_pair() and not (self.backbone.batch_norm and self.backbone._bn.wants_train_path(self.backbone.training))

    def hip_plan(self) -> engine.Plan:
        if self._bn_backbone():
            mods, fresh = self.backbone._bn.folded()
            if self._plan is None or fresh:
                self._plan = engine.Plan.from_modules(list(mods) + list(self.head), 3, True)
            return self._own(self._plan)
        if self._plan is None:
            self._plan = engine.Plan.from_modules(list(self.backbone.features) + list(self.head), 3, True)
        return self._own(self._plan)

    def head_plan(self) -> engine.Plan:
        """BatchNorm backbone with gradients: the default head as a plan of its own behind the BatchNorm chain (never stock device ops)"""
        if self._head_plan is None:
            self._head_plan = engine.Plan.from_modules(list(self.head), 1024, False)
        return self._own(self._head_plan)

    def hip_plans(self) -> list:
        """the plans whose parameters a training step of this model updates, in forward order (``yolo.optim.GradAccumulator``,
        ``parallel.make_grad_reducer``): the fused plan, or -- BatchNorm backbone -- the head's; the backbone's parameters then travel through
        autograd like the ResNet trunk's"""
        if self._bn_backbone() and self._default_pair():
            return [self.head_plan()]
        return [self.hip_plan()] if self._default_pair() else []

    @torch.no_grad()
    def forward_uint8(self, images: torch.Tensor, size: tuple[int, int] = (448, 448)) -> torch.Tensor:
        """Inference from decoded uint8 RGB images [N][H][W][3] on the device: Resize(size) + ToTensor + Normalize
        (the reference's transform, inference.py:58-66, bit-exact) are done by yolo_preprocess_u8 straight into the stem's
        input buffer -- extension of the reference surface for serving; equals ``self(transform(images))``."""
        if not (images.is_cuda and self._fusable()):
            raise RuntimeError("forward_uint8 needs device images and the default YOLOv1 backbone + head")
        y, _ = self.hip_plan().forward(images, False, False, u8_size=size)
        return y.view(-1, self.S, self.S, self.B * 5 + self.num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (N, 3, H, W) fp32 images, or a ``yolo.augment.U8Batch`` (decoded uint8 images + crop / colour parameters): the default
        YOLOv1 augments it straight into the stem's input buffer, every other model takes its fp32 tensor (``U8Batch.to_tensor``)."""
        if x.is_cuda and self._fusable():
            y = engine.run_plan(self.hip_plan(), x, self.training)
        elif x.is_cuda and self._bn_backbone() and self._default_pair():
            y = engine.run_plan(self.head_plan(), self.backbone(x), self.training)
        else:
            if not isinstance(x, torch.Tensor):
                x = x.to_tensor()
            y = self.head(self.backbone(x))
        if y.dim() == 2:
            y = y.view(-1, self.S, self.S, self.B * 5 + self.num_classes)
        return y
