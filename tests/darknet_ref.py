"""Shared by tests/test_darknet_augment_cpu.py and tests/test_gpu_darknet_augment.py: the window cases of the Darknet recipe (a window past
each single border of the image, past all four, strictly inside, equal to the image, of exactly the output's width or height while it
leaves the image) and the host path they are compared with."""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))

from yolo.dataset import JitterParams, _DarknetAugment  # noqa: E402

OUT = (48, 64)          # (Ho, Wo) of the small cases
SIZES = [(37, 53), (90, 120)]


def windows(h, w, Ho=OUT[0], Wo=OUT[1]):
    """(name, (top, left, ch, cw)) for an h x w image"""
    return [("past the left border", (2, -5, h - 6, w - 3)),
            ("past the right border", (2, 6, h - 6, w + 1)),
            ("past the top border", (-4, 3, h - 2, w - 7)),
            ("past the bottom border", (5, 3, h + 2, w - 7)),
            ("past all four borders", (-3, -6, h + 9, w + 11)),
            ("strictly inside", (3, 4, h - 8, w - 9)),
            ("equal to the image", (0, 0, h, w)),
            ("cw == Wo, past the left and top border", (-2, -7, h + 1, Wo)),
            ("ch == Ho, past the top border", (-3, 2, Ho, w - 5)),
            ("ch == Ho and cw == Wo, past the top and left border", (-3, -7, Ho, Wo))]


# (hue, saturation, exposure): the range ends of the recipe and values between them
COLOURS = [(0.1, 1.5, 1 / 1.5), (-0.1, 1 / 1.5, 1.5), (0.0, 1.0, 1.0), (0.0371, 1.2345, 0.8123), (-0.004, 0.8123, 1.2345)]


def jitter_cases(h, w, Ho=OUT[0], Wo=OUT[1]):
    """every window of ``windows`` with the flip off and on; the colour parameters rotate through COLOURS"""
    out = []
    for i, (name, win) in enumerate(windows(h, w, Ho, Wo)):
        for flip in (False, True):
            out.append((f"{h}x{w} {name}, flip {flip}", JitterParams(*win, flip, *COLOURS[(2 * i + flip) % len(COLOURS)])))
    return out


def img(h, w, seed):
    """random pixels with rows of exact greys, black, white, single-channel-saturated and bright pixels (tests/test_gpu_augment.py::_img),
    and distinct border rows and columns, so that a replicated border that came from the wrong row or column shows"""
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    k = max(h // 8, 1)
    a[:k] = a[:k, :, :1]
    a[k:2 * k, : w // 2] = 0
    a[k:2 * k, w // 2:] = 255
    a[2 * k:3 * k, :, 0] = 255
    a[3 * k:4 * k, :, 1] = 0
    a[4 * k:5 * k] = np.minimum(a[4 * k:5 * k].astype(int) + 130, 255).astype(np.uint8)
    return a


def host_u8(image, p, size=OUT):
    return np.asarray(_DarknetAugment(size).apply(Image.fromarray(image), [], p)[0])
