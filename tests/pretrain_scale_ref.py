"""Shared set-ups of tests/test_pretrain_scale_cpu.py, tests/test_gpu_pretrain_scale.py and tests/pretrain_child.py (not a test module).

* the signal-propagation measurement: YOLOv1Classifier(10) from torch.manual_seed(0), two different random batches of four 64 x 64 images, the
  standard deviation of the DIFFERENCE of the two batches' activations behind every LeakyReLU -- the part of the activation that depends on the
  input (what both batches share -- the bias floor -- cancels);
* the learning run: the 8 images of SyntheticClassificationDataset(8, 4, 64, seed=0, train=False) as one batch, plain SGD (no momentum, no weight
  decay) at lr 1e-3, clip 10, 30 steps -- torch.optim.SGD + clip_grad_norm_ on the CPU (the stock modules), yolo.optim.SGD(max_grad_norm=10) on a
  device (the HIP path);
* mixed-size uint8 images and hand-made AugParams for the input path.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

LEARN_STEPS, LEARN_LR, CLIP = 30, 1e-3, 10.0


def classifier(num_classes: int, init: str, seed: int = 0):
    """YOLOv1Classifier from torch.manual_seed(seed); init = "kaiming": yolo.models.init_kaiming_ behind the constructor"""
    from yolo import YOLOv1Classifier
    from yolo.models import init_kaiming_
    torch.manual_seed(seed)
    m = YOLOv1Classifier(num_classes=num_classes)
    if init == "kaiming":
        init_kaiming_(m)
    return m


def signal_propagation(init: str) -> list[float]:
    """std of the difference between two batches' activations behind each of the 20 LeakyReLU layers (stock fp32 modules on the CPU)"""
    m = classifier(10, init).eval()
    acts: list[list] = [[], []]
    which = [0]
    hooks = [mod.register_forward_hook(lambda _m, _i, out: acts[which[0]].append(out.detach())) for mod in m.features if isinstance(mod, nn.LeakyReLU)]
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for which[0] in (0, 1):
            m(torch.randn(4, 3, 64, 64, generator=gen))
    for h in hooks:
        h.remove()
    assert len(acts[0]) == len(acts[1]) == 20
    return [float((a - b).std()) for a, b in zip(*acts)]


def learn_set(device="cpu"):
    from yolo.dataset import SyntheticClassificationDataset
    ds = SyntheticClassificationDataset(8, 4, 64, seed=0, train=False)
    x = torch.stack([ds[i][0] for i in range(8)]).to(device)
    y = torch.tensor([ds[i][1] for i in range(8)]).to(device)
    return x, y


def learning_loop(device, init: str, steps: int = LEARN_STEPS, lr: float = LEARN_LR) -> list[float]:
    """the loss of every step of the learning run"""
    from yolo import SoftmaxCrossEntropy
    x, y = learn_set(device)
    m = classifier(4, init).to(device).train()
    on_dev = torch.device(device).type == "cuda"
    if on_dev:
        from yolo.optim import SGD
        opt = SGD(m.parameters(), lr=lr, max_grad_norm=CLIP)
    else:
        opt = torch.optim.SGD(m.parameters(), lr=lr)
    crit = SoftmaxCrossEntropy()
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss, parts = crit(m(x), y)
        loss.backward()
        if not on_dev:
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=CLIP)
        opt.step()
        losses.append(parts)
    return [p["total"] for p in losses]


def image(h: int, w: int, seed: int) -> torch.Tensor:
    """a smooth-plus-noise uint8 (h, w, 3) image: gradients for the resize to interpolate, noise for the colour operations to clip"""
    rng = np.random.Generator(np.random.PCG64([77, seed]))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([xx * (255.0 / w), yy * (255.0 / h), (xx + yy) * (255.0 / (h + w))], -1)
    return torch.from_numpy(np.clip(base + rng.normal(0.0, 40.0, (h, w, 3)), 0, 255).astype(np.uint8))


def input_cases(S: int):
    """[(uint8 image, AugParams)] for output size S: mixed sizes, 0..3 colour operations in several orders, with and without the flip, a crop
    that already has the output's width (no horizontal pass), one that has its height, one that is the output, and the whole image"""
    from yolo.dataset import OP_BRIGHTNESS as B, OP_HUE as H, OP_SATURATION as Sa, AugParams as P
    big = 2 * S + 37
    return [
        (image(S + 31, S + 50, 0), P(3, 5, S + 20, S + 33, (), 1.0, 1.0, 0.0, False)),
        (image(S + 31, S + 50, 1), P(3, 5, S + 20, S + 33, (), 1.0, 1.0, 0.0, True)),
        (image(big, big - 20, 2), P(10, 7, big - 21, big - 40, (B,), 1.37, 1.0, 0.0, True)),
        (image(big, big - 20, 3), P(0, 0, big, big - 20, (Sa, H), 1.0, 0.55, -0.08, False)),
        (image(S - 9, S + 3, 4), P(1, 2, S - 11, S - 7, (H, B, Sa), 0.62, 1.45, 0.09, True)),          # upscaling
        (image(S + 12, S + 40, 5), P(2, 17, S + 5, S, (Sa, B, H), 1.5, 0.5, 0.1, True)),                # width = output: the vertical pass reads the source
        (image(S + 12, S + 40, 6), P(2, 17, S + 5, S, (B, Sa), 0.5, 1.5, 0.0, False)),
        (image(S + 40, S + 12, 7), P(17, 2, S, S + 5, (H,), 1.0, 1.0, -0.1, True)),                     # height = output
        (image(S + 8, S + 8, 8), P(4, 4, S, S, (B, H, Sa), 1.21, 0.9, 0.04, True)),                     # the crop is the output: no resize at all
        (image(S + 8, S + 8, 9), P(0, 0, S + 8, S + 8)),                                                # validation: the whole image, nothing else
    ]
