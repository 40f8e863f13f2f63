"""The Darknet training recipe (``_DarknetAugment`` / ``JitterParams``: a window past the image border with edge replication, flip, one
HSV round trip) without a GPU: csrc/augment_math.h compiled for the host reproduces the host path's bytes -- the HSV operation alone and
the whole per-pixel pipeline (window and column addresses, both resize passes, flip, colour) --, the sampler's stream, the boxes, the
dataset's two modes and yolo_augment_u8's refusals.  Every image comparison is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))

from yolo.augment import U8Batch, collate_u8  # noqa: E402
from yolo.dataset import (OP_HSV, AugParams, JitterParams, VOCDetectionYOLO, _Augment, _DarknetAugment, create_voc_datasets,  # noqa: E402
                          jitter_boxes)
from yolo.preprocess import bilinear_tables  # noqa: E402
from darknet_ref import OUT, SIZES, host_u8, img, jitter_cases  # noqa: E402
from test_dataset_cpu import _make_voc  # noqa: E402

LIB = os.path.join(ROOT, "yolo-v1_amd", "yolo", "libyolo_hip.so")
F_FLIP, F_EDGE = 1, 2

# The loops of csrc/augment.hip on the host, over the helpers and the colour operation of the header the kernels use
PROBE = r"""
#include "augment_math.h"
using namespace yolo_aug;
static int clip8(int acc) { const int v = acc >> 22; return v < 0 ? 0 : (v > 255 ? 255 : v); }
extern "C" void colour(unsigned char *px, long n, int op, float b, float s, int shift) {
  for (long i = 0; i < n; ++i) { int r = px[3*i], g = px[3*i+1], bl = px[3*i+2];
    color_op(op, r, g, bl, b, s, shift); px[3*i] = r; px[3*i+1] = g; px[3*i+2] = bl; } }
extern "C" void pipeline(const unsigned char *src, int Hs, int Ws, int top, int left, int ch, int cw, int flags, const int *htab, int hk,
                         const int *vtab, int vk, int Ho, int Wo, int op, float vfac, float sfac, int shift, unsigned char *tmp, unsigned char *out) {
  if (hk > 0)
    for (int y = 0; y < ch; ++y) for (int xx = 0; xx < Wo; ++xx) {
      const int *row = htab + (long)xx * (2 + hk);
      int a[3] = {1 << 21, 1 << 21, 1 << 21};
      for (int x = 0; x < row[1]; ++x) for (int c = 0; c < 3; ++c)
        a[c] += (int)src[((long)src_row(top, y, Hs, flags) * Ws + src_col(left, row[0] + x, Ws, flags)) * 3 + c] * row[2 + x];
      for (int c = 0; c < 3; ++c) tmp[((long)y * Wo + xx) * 3 + c] = (unsigned char)clip8(a[c]);
    }
  for (int yy = 0; yy < Ho; ++yy) for (int xx = 0; xx < Wo; ++xx) {
    const int sx = stage1_col(xx, Wo, flags);
    int px[3];
    for (int c = 0; c < 3; ++c) {
      auto at = [&](int y) { return hk > 0 ? (int)tmp[((long)y * Wo + sx) * 3 + c]
                                           : (int)src[((long)src_row(top, y, Hs, flags) * Ws + src_col(left, sx, Ws, flags)) * 3 + c]; };
      if (vk > 0) {
        const int *row = vtab + (long)yy * (2 + vk);
        int a = 1 << 21;
        for (int y = 0; y < row[1]; ++y) a += at(row[0] + y) * row[2 + y];
        px[c] = clip8(a);
      } else px[c] = at(yy);
    }
    if (op >= 0) color_op(op, px[0], px[1], px[2], vfac, sfac, shift);
    for (int c = 0; c < 3; ++c) out[((long)yy * Wo + xx) * 3 + c] = (unsigned char)px[c];
  } }
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe")
    (d / "p.cpp").write_text(PROBE)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "yolo-v1_amd", "csrc"), str(d / "p.cpp"), "-o",
                           str(d / "p.so")])
    L = ctypes.CDLL(str(d / "p.so"))
    L.colour.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int]
    L.pipeline.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                                   ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_hsv_operation_equals_pillow(probe):
    """the pixel set of test_augment_cpu.py::test_colour_arithmetic_equals_pillow, factors {1/1.5, 0.8123, 1, 1.2345, 1.5}^2 x its five hue shifts"""
    a = np.random.default_rng(0).integers(0, 256, (400, 600, 3), dtype=np.uint8)
    a[:40] = a[:40, :, :1]
    a[40:60] = 0
    a[60:80] = 255
    a[80:100, :, 0], a[100:120, :, 1], a[120:140, :, 2] = 255, 255, 255
    a[140:160, :, 0], a[160:180, :, 1] = 0, 0
    a[180:200] = np.minimum(a[180:200].astype(int) + 120, 255).astype(np.uint8)
    im = Image.fromarray(a)
    factors = (1 / 1.5, 0.8123, 1.0, 1.2345, 1.5)
    for delta in (-0.1, -0.0371, 0.0, 0.003, 0.1):
        for s in factors:
            for v in factors:
                out = a.copy()
                probe.colour(out.ctypes.data, out.size // 3, OP_HSV, v, s, int(delta * 255))
                ref = np.asarray(_DarknetAugment._hsv(im, delta, s, v))
                assert np.array_equal(out, ref), f"hue {delta} S x{s} V x{v}: {(out != ref).sum()} bytes differ"
        # the hue operation of the reference recipe is what it was: the round trip without the two products
        out = a.copy()
        probe.colour(out.ctypes.data, out.size // 3, 2, 1.0, 1.0, int(delta * 255))
        assert np.array_equal(out, np.asarray(_Augment._hue(im, delta)))


def _pipeline(probe, image, p, flags, size=OUT):
    Ho, Wo = size
    h, w = image.shape[:2]
    tabs = []
    for n_in, n_out in ((p.cw, Wo), (p.ch, Ho)):
        if n_in != n_out:
            b, c, k = bilinear_tables(n_in, n_out)
            tabs.append((np.ascontiguousarray(np.concatenate([b, c], axis=1)), k))
        else:
            tabs.append((None, 0))
    (ht, hk), (vt, vk) = tabs
    src = np.ascontiguousarray(image)
    tmp, out = np.zeros((max(p.ch, 1), Wo, 3), np.uint8), np.zeros((Ho, Wo, 3), np.uint8)
    probe.pipeline(src.ctypes.data, h, w, p.top, p.left, p.ch, p.cw, flags, ht.ctypes.data if hk else None, hk, vt.ctypes.data if vk else None, vk, Ho, Wo,
                   OP_HSV, p.exposure, p.saturation, int(p.hue * 255), tmp.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("hw", SIZES)
def test_whole_pipeline_on_the_host(probe, hw):
    """the header's address helpers and HSV operation, looped as the two kernels loop them with Pillow's tables, against _DarknetAugment.apply"""
    image = img(*hw, seed=hw[0])
    for name, p in jitter_cases(*hw):
        ref = host_u8(image, p)
        inside = 0 <= p.top and 0 <= p.left and p.top + p.ch <= hw[0] and p.left + p.cw <= hw[1]
        assert inside == ("inside" in name or "equal" in name), name
        for flags in ([0, F_EDGE] if inside else [F_EDGE]):          # a window inside the image: the clamp changes nothing
            got = _pipeline(probe, image, p, flags | (F_FLIP if p.flip else 0))
            assert np.array_equal(got, ref), f"{name}, flags {flags}: {(got != ref).sum()} bytes differ"


# ---------------------------------------------------------------------------------------------------------------- sampler
def test_sampler_stream_and_ranges():
    aug = _DarknetAugment((448, 448))
    for seed, (w, h) in enumerate([(500, 375), (333, 500), (53, 37), (200, 200)]):
        torch.manual_seed(seed)
        a = aug.sample(w, h)
        after = torch.rand(1)
        torch.manual_seed(seed)
        b = aug.sample(w, h)
        assert a == b and isinstance(a, JitterParams) and torch.equal(torch.rand(1), after)      # same parameters, same number of draws
    torch.manual_seed(5)
    w, h = 500, 375
    flips, inv_s, inv_e = set(), set(), set()
    for _ in range(200):
        p = aug.sample(w, h)
        pright, pbot = w - p.left - p.cw, h - p.top - p.ch
        assert all(isinstance(v, int) for v in p[:4]) and isinstance(p.flip, bool)
        assert abs(p.left) <= int(0.2 * w) and abs(pright) <= int(0.2 * w) and abs(p.top) <= int(0.2 * h) and abs(pbot) <= int(0.2 * h)
        assert p.cw == w - p.left - pright and p.ch == h - p.top - pbot and p.cw > 0 and p.ch > 0
        assert abs(p.hue) <= 0.1 and 1 / 1.5 <= p.saturation <= 1.5 and 1 / 1.5 <= p.exposure <= 1.5
        flips.add(p.flip)
        inv_s.add(p.saturation < 1)
        inv_e.add(p.exposure < 1)
    assert flips == {False, True} and inv_s == {False, True} and inv_e == {False, True}


def test_sampler_draws_in_the_documented_order():
    """pleft, pright / ptop, pbot / flip / hue / saturation (+ its inversion) / exposure (+ its inversion), from torch's global generator"""
    from yolo.dataset import _uniform
    w, h = 500, 375
    torch.manual_seed(9)
    p = _DarknetAugment((448, 448)).sample(w, h)
    torch.manual_seed(9)
    pleft, pright = torch.randint(-100, 101, (2,)).tolist()
    ptop, pbot = torch.randint(-75, 76, (2,)).tolist()
    flip = float(torch.rand(1)) < 0.5
    hue = _uniform(-0.1, 0.1)
    fac = []
    for _ in range(2):
        s = _uniform(1.0, 1.5)
        fac.append(1 / s if float(torch.rand(1)) < 0.5 else s)
    assert p == JitterParams(ptop, pleft, h - ptop - pbot, w - pleft - pright, flip, hue, fac[0], fac[1])


# ---------------------------------------------------------------------------------------------------------------- boxes
def test_boxes_follow_the_pixels():
    """a white rectangle on black, at least one pixel inside every border (edge replication would smear one that touches it), through the
    geometry alone: the bounding box of the output pixels >= 128 agrees with jitter_boxes within 1 output pixel per edge (1/2 px for the
    threshold at half intensity + 1/2 px for integer pixel edges)"""
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    n, worst = 0, 0.0
    for h, w in [(375, 500), (500, 333), (200, 200), (90, 120), (37, 53)]:
        for size in [(448, 448), (48, 64), (128, 96)]:
            aug = _DarknetAugment(size)
            for _ in range(14):
                p = aug.sample(w, h)
                # at least a quarter of each side: the window cuts at most a fifth, so part of the rectangle always shows
                bw, bh = int(rng.integers(w // 4 + 1, w - 2)), int(rng.integers(h // 4 + 1, h - 2))
                x0, y0 = int(rng.integers(1, w - bw)), int(rng.integers(1, h - bh))
                a = np.zeros((h, w, 3), np.uint8)
                a[y0:y0 + bh, x0:x0 + bw] = 255
                out = np.asarray(aug.geometry(Image.fromarray(a), p))[..., 0] >= 128
                boxes, kept = jitter_boxes([[x0, y0, x0 + bw, y0 + bh]], p, size)
                assert kept == [0] and out.any(), (h, w, size, p)
                ys, xs = np.flatnonzero(out.any(axis=1)), np.flatnonzero(out.any(axis=0))
                seen = [xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]
                err = max(abs(s - b) for s, b in zip(seen, boxes[0]))
                worst = max(worst, err)
                assert err <= 1.0, (h, w, size, p, seen, boxes[0])
                n += 1
    assert n >= 200
    print(f"{n} windows, worst edge error {worst:.3f} px")


def test_jitter_boxes_rules():
    p = JitterParams(-10, -20, 120, 140)                     # 100 x 100 image, window past every border; output 60 x 70: scale 0.5
    boxes, kept = jitter_boxes([[0, 0, 100, 100], [30, 40, 50, 80]], p, (60, 70))
    assert kept == [0, 1] and boxes == [[10.0, 5.0, 60.0, 55.0], [25.0, 25.0, 35.0, 45.0]]
    boxes, kept = jitter_boxes([[0, 0, 100, 100], [30, 40, 50, 80]], p._replace(flip=True), (60, 70))
    assert boxes == [[10.0, 5.0, 60.0, 55.0], [35.0, 25.0, 45.0, 45.0]]
    q = JitterParams(50, 60, 40, 30)                         # a window inside the image
    boxes, kept = jitter_boxes([[0, 0, 20, 20], [55, 45, 70, 60], [100, 0, 120, 200], [61, 0, 80, 50.01]], q, (80, 60))
    assert kept == [1]                                       # outside; inside; beside it; 0.02 of a pixel high (< 1e-3 H = 0.08) after the clamp
    assert boxes == [[0.0, 0.0, 20.0, 20.0]]


@pytest.fixture()
def voc(tmp_path):
    samples = {"000001": (500, 375, [("dog", 2, 3, 40, 30), ("person", 150, 100, 260, 300)]),
               "000002": (320, 480, [("car", 100, 100, 200, 300)]),
               "000003": (200, 200, [("cat", 20, 30, 150, 190)]),
               "000004": (400, 300, [("cat", 0, 0, 400, 300)])}
    _make_voc(tmp_path, "2007", samples, {"train": ["000001", "000002", "000003"], "val": ["000003", "000004"]})
    return tmp_path


def test_dropped_box_takes_its_class_and_flip_mirrors_the_cell(voc):
    ds = VOCDetectionYOLO(root=voc, year="2007", image_set="train", augment=True, recipe="darknet")
    _, ann = ds._load(0)
    whole = ds._augmented_target(ann, 500, 375, JitterParams(0, 0, 375, 500))
    assert whole[..., 4].sum() == 2 and whole[0, 0, 4] == 1 and whole[0, 0, 10 + 11] == 1            # the dog, top-left cell
    cut = ds._augmented_target(ann, 500, 375, JitterParams(50, 60, 300, 400))                        # the dog lies wholly outside
    assert cut[..., 4].sum() == 1 and cut[..., 10 + 11].sum() == 0 and cut[..., 10 + 14].sum() == 1  # gone with its class id; the person stays
    # the person: centre x = 205 / 500 -> column 2; mirrored: 295 / 500 -> column 4; same row, same size, mirrored cell offset
    i, j = 3, 2
    assert whole[i, j, 4] == 1 and whole[i, j, 10 + 14] == 1
    flipped = ds._augmented_target(ann, 500, 375, JitterParams(0, 0, 375, 500, True))
    assert flipped[i, 6 - j, 4] == 1 and flipped[i, 6 - j, 10 + 14] == 1 and flipped[i, j, 4] == 0 and flipped[0, 6, 10 + 11] == 1
    assert torch.allclose(flipped[i, 6 - j, 2:4], whole[i, j, 2:4]) and torch.allclose(flipped[i, 6 - j, 0], 1 - whole[i, j, 0], atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- dataset
def test_dataset_modes_agree_and_the_reference_recipe_is_unchanged(voc):
    host = VOCDetectionYOLO(root=voc, year="2007", image_set="train", augment=True, recipe="darknet")
    dev = create_voc_datasets([("2007", "train")], augment=True, root=voc, device_transform=True, recipe="darknet")
    assert isinstance(host.transform, _DarknetAugment) and isinstance(dev.transform, _DarknetAugment) and dev.recipe == "darknet"
    torch.manual_seed(3)
    h_samples = [host[i] for i in range(3)]
    torch.manual_seed(3)
    d_samples = [dev[i] for i in range(3)]
    for (hx, ht), (u8, p, dt) in zip(h_samples, d_samples):
        assert u8.dtype == torch.uint8 and isinstance(p, JitterParams) and torch.equal(ht, dt)
    batch, targets = collate_u8(d_samples)
    assert torch.equal(targets, torch.stack([t for _, t in h_samples]))
    assert torch.equal(batch.to_tensor(), torch.stack([x for x, _ in h_samples]))                   # CPU: the PIL host path, same bits
    # a mixed batch packs, and each entry goes through its own host path
    ref_ds = VOCDetectionYOLO(root=voc, year="2007", image_set="train", augment=True, device_transform=True)
    torch.manual_seed(4)
    mixed = [ref_ds[0], dev[1], ref_ds[2], dev[0]]
    mb, _ = collate_u8(mixed)
    assert [type(p) for p in mb.params] == [AugParams, JitterParams, AugParams, JitterParams] and mb.shape == (4, 3, 448, 448)
    u8 = mb.to_uint8()
    for k, (im, p, _) in enumerate(mixed):
        aug = _DarknetAugment((448, 448)) if isinstance(p, JitterParams) else _Augment((448, 448))
        assert np.array_equal(u8[k].numpy(), np.asarray(aug.apply(Image.fromarray(im.numpy()), [], p)[0]))
    # only a JitterParams window may leave the image, and it has to meet it
    flat = mixed[1][0].reshape(-1)
    hw = mixed[1][0].shape[:2]
    U8Batch(flat, [hw], [JitterParams(-5, -5, hw[0] + 10, hw[1] + 10)])
    with pytest.raises(ValueError, match="outside"):
        U8Batch(flat, [hw], [AugParams(-5, -5, hw[0] + 10, hw[1] + 10)])
    with pytest.raises(ValueError, match="misses"):
        U8Batch(flat, [hw], [JitterParams(hw[0], 0, 10, 10)])
    # recipe="reference" (and no recipe at all): today's samples for a seed -- _Augment's draws, apply and the finishing transform
    from yolo.inference import _Preprocess
    for kw in ({}, {"recipe": "reference"}):
        ds = VOCDetectionYOLO(root=voc, year="2007", image_set="train", augment=True, **kw)
        assert type(ds.transform) is _Augment
        torch.manual_seed(6)
        got = [ds[i] for i in range(3)]
        torch.manual_seed(6)
        for i, (x, t) in enumerate(got):
            image, ann = ds._load(i)
            p = _Augment((448, 448)).sample(*image.size)
            assert torch.equal(x, _Preprocess(size=(448, 448))(_Augment((448, 448)).apply(image, [], p)[0]))
            assert torch.equal(t, ds._augmented_target(ann, *image.size, p))
    # validation splits ignore the recipe
    for dt in (False, True):
        va = VOCDetectionYOLO(root=voc, year="2007", image_set="val", augment=True, device_transform=dt)
        vb = VOCDetectionYOLO(root=voc, year="2007", image_set="val", augment=True, device_transform=dt, recipe="darknet")
        assert not vb.augment and type(vb.transform) is type(va.transform)
        for i in range(2):
            assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(va[i], vb[i]))
    with pytest.raises(ValueError, match="recipe"):
        VOCDetectionYOLO(root=voc, year="2007", image_set="train", recipe="mosaic")


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(LIB)


def test_descriptor_layout_and_refusals(built, tmp_path):
    from yolo import _hip
    D = _hip.AugmentDesc
    fields = [n for n, _ in D._fields_]
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu", sizeof(yolo_augment_desc));\n' + \
            "".join(f'printf(" %zu", offsetof(yolo_augment_desc, {n}));\n' for n in fields) + \
            'printf(" %d %d %d\\n", YOLO_AUG_HSV, YOLO_AUG_F_FLIP, YOLO_AUG_F_EDGE);return 0;}\n'
    (tmp_path / "p.c").write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "p")]).split()]
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in fields] + [_hip.AUG_HSV, _hip.AUG_F_FLIP, _hip.AUG_F_EDGE]
    assert ctypes.sizeof(D) == 96 and D.flags.offset == 92 and fields[-1] == "flags"       # where `reserved` was: the layout of ABI version 2
    assert (_hip.AUG_HSV, _hip.AUG_F_FLIP, _hip.AUG_F_EDGE) == (OP_HSV, F_FLIP, F_EDGE) == (4, 1, 2)

    fn = built.yolo_augment_u8
    fn.argtypes, fn.restype = _hip._SIGS["yolo_augment_u8"], ctypes.c_int
    built.yolo_hip_last_error.restype = ctypes.c_char_p
    mean, std = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.2, 0.2, 0.2)
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before any HIP call

    def refused(ops=(), **kw):
        d = D(src_off=0, tmp_off=0, Hs=100, Ws=100, top=0, left=0, ch=100, cw=100, htab=4096, vtab=4096, hk=3, vk=3, n_ops=len(ops), brightness=1.0,
              saturation=1.0)
        for i, op in enumerate(ops):
            d.ops[i] = op
        for k, v in kw.items():
            setattr(d, k, v)
        rc = fn(fake, 100 * 100 * 3, (D * 1)(d), fake, 1, 448, 448, fake, 1 << 24, mean, std, None, 0, fake, None, None)
        return rc == -1 and built.yolo_hip_last_error()

    assert b"unknown flag" in refused(flags=4) and b"unknown flag" in refused(flags=3 | 8) and b"unknown flag" in refused(flags=-1)
    for ops in ((4, 0), (2, 4), (4, 4), (0, 1, 4)):
        assert b"only operation" in refused(ops=ops), ops
    assert b"unknown colour operation" in refused(ops=(3,))                                   # code 3 stays unassigned
    for bad in (dict(saturation=float("nan")), dict(brightness=float("nan")), dict(saturation=float("inf")), dict(brightness=float("inf")),
                dict(saturation=-0.5), dict(brightness=-1e-9)):
        assert b"finite" in refused(ops=(4,), **bad), bad
    for miss in (dict(top=100), dict(top=-100), dict(left=100), dict(left=-100), dict(top=200, left=-300)):
        assert b"misses" in refused(flags=F_EDGE, **miss), miss
    for bad in (dict(ch=0), dict(cw=-1), dict(cw=40000), dict(top=-40000, ch=32768)):
        assert b"out of range" in refused(flags=F_EDGE, **bad), bad
    for out in (dict(top=-1), dict(left=1), dict(ch=101), dict(top=-5, ch=110)):             # out of the image without F_EDGE: today's refusal
        assert b"outside its" in refused(**out), out
        assert b"outside its" in refused(flags=F_FLIP, **out), out
