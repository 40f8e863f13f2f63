"""Device-augmentation input path without a GPU: the sample / apply split of ``_Augment`` keeps the host path's random stream and
results, the dataset's device mode hands out the same parameters and targets, ``collate_u8`` / ``U8Batch`` pack a ragged batch,
the colour arithmetic of csrc/augment_math.h (compiled for the host) reproduces Pillow's bytes, and yolo_augment_u8's descriptor
and argument checks agree with the header."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))

from yolo.augment import U8Batch, collate_u8  # noqa: E402
from yolo.dataset import OP_BRIGHTNESS, OP_HUE, OP_SATURATION, AugParams, VOCDetectionYOLO, _Augment, _uniform, create_voc_datasets  # noqa: E402
from test_dataset_cpu import _make_voc  # noqa: E402

LIB = os.path.join(ROOT, "yolo-v1_amd", "yolo", "libyolo_hip.so")


def _old_call(aug, image, boxes):
    """``_Augment.__call__`` as it was before the split (crop draws, brightness, saturation, hue, randperm; operations as closures)"""
    w, h = image.size
    top, left, ch, cw = aug._crop_params(w, h)
    image = image.crop((left, top, left + cw, top + ch)).resize((aug.size[1], aug.size[0]), Image.BILINEAR)
    sx, sy = aug.size[1] / cw, aug.size[0] / ch
    out = []
    for x0, y0, x1, y1 in boxes:
        x0, x1 = min(max(x0 - left, 0.0), cw) * sx, min(max(x1 - left, 0.0), cw) * sx
        y0, y1 = min(max(y0 - top, 0.0), ch) * sy, min(max(y1 - top, 0.0), ch) * sy
        out.append([x0, y0, x1, y1])
    ops = []
    if aug.brightness:
        f = _uniform(max(0.0, 1 - aug.brightness), 1 + aug.brightness)
        ops.append(lambda im, f=f: ImageEnhance.Brightness(im).enhance(f))
    if aug.saturation:
        f = _uniform(max(0.0, 1 - aug.saturation), 1 + aug.saturation)
        ops.append(lambda im, f=f: ImageEnhance.Color(im).enhance(f))
    if aug.hue:
        f = _uniform(-aug.hue, aug.hue)
        ops.append(lambda im, f=f: aug._hue(im, f))
    for k in torch.randperm(len(ops)).tolist():
        image = ops[k](image)
    return image, out


@pytest.mark.parametrize("seed", [0, 1, 7, 123])
@pytest.mark.parametrize("hw", [(375, 500), (500, 333), (200, 200), (90, 120), (300, 900)])
def test_split_keeps_the_host_path(seed, hw):
    img = Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=hw + (3,), dtype=np.uint8))
    boxes = [[10.0, 20.0, hw[1] - 5.0, hw[0] - 8.0], [0.0, 0.0, 30.5, 40.25]]
    aug = _Augment((448, 448))
    torch.manual_seed(seed)
    ref_img, ref_boxes = _old_call(aug, img, boxes)
    after_ref = torch.rand(1)
    torch.manual_seed(seed)
    got_img, got_boxes = aug(img, boxes)
    assert torch.equal(torch.rand(1), after_ref)                       # the same number of draws, in the same order
    assert np.array_equal(np.asarray(got_img), np.asarray(ref_img)) and got_boxes == ref_boxes
    torch.manual_seed(seed)
    p = aug.sample(hw[1], hw[0])
    assert sorted(p.ops) == [OP_BRIGHTNESS, OP_SATURATION, OP_HUE] and 0.5 <= p.brightness <= 1.5 and abs(p.hue) <= 0.1
    again, _ = aug.apply(img, boxes, p)
    assert np.array_equal(np.asarray(again), np.asarray(ref_img))


@pytest.fixture()
def voc(tmp_path):
    samples = {"000001": (500, 375, [("dog", 48, 240, 195, 371), ("person", 8, 12, 352, 498)]),
               "000002": (320, 480, [("car", 100, 100, 200, 300)]),
               "000003": (200, 200, []),
               "000004": (400, 300, [("cat", 0, 0, 400, 300)])}
    _make_voc(tmp_path, "2007", samples, {"train": ["000001", "000002", "000003"], "val": ["000003", "000004"]})
    return tmp_path


def test_device_mode_hands_out_the_host_path_parameters(voc):
    host = VOCDetectionYOLO(root=voc, year="2007", image_set="train", augment=True)
    dev = create_voc_datasets([("2007", "train")], augment=True, root=voc, device_transform=True)
    assert dev.device_transform and not host.device_transform
    torch.manual_seed(3)
    h_samples = [host[i] for i in range(3)]
    torch.manual_seed(3)
    d_samples = [dev[i] for i in range(3)]
    for (hx, ht), (u8, p, dt) in zip(h_samples, d_samples):
        assert u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3 and isinstance(p, AugParams)
        assert torch.equal(ht, dt)
    batch, targets = collate_u8(d_samples)
    assert isinstance(batch, U8Batch) and batch.shape == (3, 3, 448, 448) and not batch.is_cuda and len(batch) == 3
    assert torch.equal(targets, torch.stack([t for _, t in h_samples]))
    assert torch.equal(batch.to_tensor(), torch.stack([x for x, _ in h_samples]))       # CPU: the PIL host path, same bits
    assert batch.to("cpu") is batch
    # validation: identity crop, no colour operations, the evaluation transform's bits
    hv = VOCDetectionYOLO(root=voc, year="2007", image_set="val", augment=True)
    dv = VOCDetectionYOLO(root=voc, year="2007", image_set="val", augment=True, device_transform=True)
    vb, vt = collate_u8([dv[0], dv[1]])
    assert [tuple(p) for p in vb.params] == [(0, 0, 200, 200, (), 1.0, 1.0, 0.0), (0, 0, 300, 400, (), 1.0, 1.0, 0.0)]
    assert torch.equal(vb.to_tensor(), torch.stack([hv[0][0], hv[1][0]])) and torch.equal(vt, torch.stack([hv[0][1], hv[1][1]]))
    with pytest.raises(ValueError, match="custom"):
        VOCDetectionYOLO(root=voc, year="2007", image_set="val", transform=lambda im: im, device_transform=True)


def test_collate_layout_and_descriptor_checks():
    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, size=s + (3,), dtype=np.uint8)) for s in [(30, 50), (448, 448), (17, 9)]]
    ps = [AugParams(2, 3, 20, 40, (OP_HUE, OP_BRIGHTNESS), 1.2, 1.0, -0.05), AugParams(0, 0, 448, 448), AugParams(0, 0, 17, 9, (OP_SATURATION,), 1.0, 0.7, 0.0)]
    t = torch.zeros(7, 7, 30)
    batch, targets = collate_u8([(im, p, t) for im, p in zip(imgs, ps)])
    assert batch.offsets == [0, 30 * 50 * 3, 30 * 50 * 3 + 448 * 448 * 3] and batch.data.numel() == batch.offsets[2] + 17 * 9 * 3
    assert batch.sizes == [(30, 50), (448, 448), (17, 9)] and targets.shape == (3, 7, 7, 30)
    for i, im in enumerate(imgs):
        assert torch.equal(batch.image(i), im)
    one, t1 = collate_u8([(imgs[2], ps[2], t)])
    assert one.shape == (1, 3, 448, 448) and t1.shape == (1, 7, 7, 30) and torch.equal(one.image(0), imgs[2])
    assert one.to_uint8().shape == (1, 448, 448, 3)
    with pytest.raises(ValueError, match="outside"):
        U8Batch(imgs[0].reshape(-1), [(30, 50)], [AugParams(0, 11, 30, 40)])
    with pytest.raises(ValueError, match="bytes"):
        U8Batch(imgs[0].reshape(-1)[:-1], [(30, 50)], [AugParams(0, 0, 30, 50)])
    with pytest.raises(RuntimeError, match="no input gradient"):
        batch.requires_grad_()
    assert batch.requires_grad is False


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_descriptor_layout_and_argument_errors(built, tmp_path):
    from yolo import _hip
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(yolo_augment_desc), ' \
            'offsetof(yolo_augment_desc, htab), offsetof(yolo_augment_desc, n_ops), offsetof(yolo_augment_desc, hue_shift));return 0;}\n'
    src = tmp_path / "p.c"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "p")]).split()]
    D = _hip.AugmentDesc
    assert sizes == [ctypes.sizeof(D), D.htab.offset, D.n_ops.offset, D.hue_shift.offset]
    assert (_hip.AUG_BRIGHTNESS, _hip.AUG_SATURATION, _hip.AUG_HUE) == (OP_BRIGHTNESS, OP_SATURATION, OP_HUE)

    fn = built.yolo_augment_u8
    fn.argtypes, fn.restype = _hip._SIGS["yolo_augment_u8"], ctypes.c_int
    built.yolo_hip_last_error.restype = ctypes.c_char_p
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before any HIP call

    def call(d, src=fake, descs_dev=fake, out=fake, tmp=fake, tmp_bytes=1 << 20, std3=std, n=1):
        arr = (D * 1)(d)
        return fn(src, 100 * 100 * 3, arr, descs_dev, n, 448, 448, tmp, tmp_bytes, mean, std3, None, 0, out, None, None)

    def desc(**kw):
        d = D(src_off=0, tmp_off=0, Hs=100, Ws=100, top=0, left=0, ch=100, cw=100, htab=4096, vtab=4096, hk=3, vk=3, n_ops=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for bad in (dict(src=None), dict(descs_dev=None), dict(out=None), dict(n=0), dict(std3=(ctypes.c_float * 3)(0.2, 0.0, 0.2)), dict(tmp=None),
                dict(tmp_bytes=100)):
        assert call(desc(), **bad) == -1, bad
        assert b"yolo_augment_u8" in built.yolo_hip_last_error()
    for bad in (dict(left=1), dict(top=-1), dict(ch=101), dict(cw=0), dict(Hs=101), dict(src_off=1), dict(n_ops=4), dict(n_ops=-1), dict(htab=None),
                dict(vk=0), dict(tmp_off=-1)):
        assert call(desc(**bad)) == -1, bad
    d = desc(n_ops=1)
    d.ops[0] = 3
    assert call(d) == -1 and b"unknown colour operation" in built.yolo_hip_last_error()


def test_colour_arithmetic_equals_pillow(tmp_path):
    """csrc/augment_math.h compiled for the host (plain IEEE arithmetic, no contraction) against Pillow on random pixels, exact greys,
    black, white and single-channel-saturated pixels, at both ends of every factor's range"""
    src = tmp_path / "p.cpp"
    src.write_text('#include "augment_math.h"\nextern "C" void apply(unsigned char *px, long n, int op, float b, float s, int shift) {\n'
                   '  for (long i = 0; i < n; ++i) { int r = px[3*i], g = px[3*i+1], bl = px[3*i+2];\n'
                   '    yolo_aug::color_op(op, r, g, bl, b, s, shift); px[3*i] = r; px[3*i+1] = g; px[3*i+2] = bl; } }\n')
    so = tmp_path / "p.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "yolo-v1_amd", "csrc"), str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    L.apply.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int]
    a = np.random.default_rng(0).integers(0, 256, (400, 600, 3), dtype=np.uint8)
    a[:40] = a[:40, :, :1]
    a[40:60] = 0
    a[60:80] = 255
    a[80:100, :, 0], a[100:120, :, 1], a[120:140, :, 2] = 255, 255, 255
    a[140:160, :, 0], a[160:180, :, 1] = 0, 0
    a[180:200] = np.minimum(a[180:200].astype(int) + 120, 255).astype(np.uint8)      # bright pixels: the clipping branch of brightness > 1
    im = Image.fromarray(a)

    def run(op, b=1.0, s=1.0, shift=0):
        out = a.copy()
        L.apply(out.ctypes.data, out.size // 3, op, b, s, shift)
        return out

    for f in (0.5, 0.7311, 1.0, 1.2345, 1.5):
        assert np.array_equal(run(OP_BRIGHTNESS, b=f), np.asarray(ImageEnhance.Brightness(im).enhance(f))), f
        assert np.array_equal(run(OP_SATURATION, s=f), np.asarray(ImageEnhance.Color(im).enhance(f))), f
    for delta in (-0.1, -0.0371, 0.0, 0.003, 0.1):
        assert np.array_equal(run(OP_HUE, shift=int(delta * 255)), np.asarray(_Augment._hue(im, delta))), delta
