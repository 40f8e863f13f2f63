"""yolo_augment_u8 (ragged uint8 batch -> crop -> Pillow-exact resize -> colour jitter -> ToTensor -> Normalize on the device) against the
host path (``_Augment.apply`` on Pillow + ``_Preprocess``): every comparison is exact."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v1_amd"))

pytestmark = pytest.mark.gpu

B, S, H = 0, 1, 2      # OP_BRIGHTNESS, OP_SATURATION, OP_HUE


def _img(h, w, seed, special=True):
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if special:          # exact greys, black, white, single-channel-saturated and bright pixels
        k = max(h // 8, 1)
        a[:k] = a[:k, :, :1]
        a[k:2 * k, : w // 2] = 0
        a[k:2 * k, w // 2:] = 255
        a[2 * k:3 * k, :, 0] = 255
        a[3 * k:4 * k, :, 1] = 0
        a[4 * k:5 * k] = np.minimum(a[4 * k:5 * k].astype(int) + 130, 255).astype(np.uint8)
    return a


def _batch(images, params, size=(448, 448)):
    from yolo.augment import collate_u8
    t = torch.zeros(7, 7, 30)
    return collate_u8([(torch.from_numpy(im), p, t) for im, p in zip(images, params)], size=size)[0]


def _host_u8(images, params, size=(448, 448)):
    from yolo.dataset import _Augment
    aug = _Augment(size)
    return np.stack([np.asarray(aug.apply(Image.fromarray(im), [], p)[0]) for im, p in zip(images, params)])


def _check(images, params, size=(448, 448)):
    got = _batch(images, params, size).cuda().to_uint8().cpu().numpy()
    ref = _host_u8(images, params, size)
    for i in range(len(images)):
        assert np.array_equal(got[i], ref[i]), f"image {i} {images[i].shape} {params[i]}: {(got[i] != ref[i]).sum()} bytes differ"


def test_geometry_in_one_ragged_batch():
    """landscape, portrait, square, an upscaled small image, a crop of exactly the target size, crops touching each border -- one batch of
    different sizes, so a descriptor mix-up cannot hide"""
    from yolo.dataset import AugParams as P
    full = (B, S, H)
    cases = [((375, 500), P(20, 31, 300, 410, full, 1.1, 0.8, 0.03)),
             ((500, 333), P(5, 7, 480, 300, full, 0.9, 1.3, -0.07)),
             ((448, 448), P(0, 0, 448, 448, (), 1.0, 1.0, 0.0)),
             ((90, 120), P(3, 4, 80, 100, (S,), 1.0, 0.6, 0.0)),
             ((600, 700), P(100, 200, 448, 448, (H,), 1.0, 1.0, 0.1)),            # crop == target: no resize pass at all
             ((600, 700), P(10, 20, 448, 300, (B,), 1.4, 1.0, 0.0)),              # vertical size unchanged only
             ((600, 700), P(10, 20, 300, 448, (B,), 0.6, 1.0, 0.0)),              # horizontal size unchanged only
             ((375, 500), P(0, 0, 300, 400, full, 1.0, 1.0, 0.0)),                # top-left corner
             ((375, 500), P(75, 100, 300, 400, full, 1.5, 1.5, -0.1)),            # bottom-right corner
             ((375, 500), P(0, 100, 375, 400, (), 1.0, 1.0, 0.0)),                # full height, right border
             ((1000, 1500), P(0, 0, 1000, 1500, (H, S), 1.0, 0.5, 0.05)),         # strong down-scaling
             ((37, 53), P(0, 0, 37, 53, (B, H), 1.25, 1.0, -0.02))]               # the smallest image last
    images = [_img(h, w, i) for i, ((h, w), _) in enumerate(cases)]
    _check(images, [p for _, p in cases])
    _check(images[-1:], [cases[-1][1]])                                            # a batch of one


def test_colour_operations_orders_and_range_ends():
    from yolo.dataset import AugParams as P
    im = _img(300, 400, 11)
    crop = (10, 20, 250, 330)
    params = [P(*crop, order, 1.3, 0.7, 0.06) for order in itertools.permutations((B, S, H))]
    params += [P(*crop, (B,), f, 1.0, 0.0) for f in (0.5, 1.0, 1.5)]
    params += [P(*crop, (S,), 1.0, f, 0.0) for f in (0.5, 1.0, 1.5)]
    params += [P(*crop, (H,), 1.0, 1.0, d) for d in (-0.1, 0.0, 0.1, 0.0999, -0.004)]
    params += [P(*crop, (), 1.0, 1.0, 0.0), P(*crop, (S, B), 1.5, 1.5, 0.0), P(*crop, (H, B), 1.5, 1.0, 0.1)]
    _check([im] * len(params), params)


def test_random_parameters_from_the_sampler():
    from yolo.dataset import _Augment
    torch.manual_seed(4)
    aug = _Augment((448, 448))
    sizes = [(375, 500), (500, 375), (333, 500), (281, 500), (500, 400), (120, 160), (448, 448), (442, 500)]
    images = [_img(h, w, 50 + i, special=i % 2 == 0) for i, (h, w) in enumerate(sizes)]
    _check(images, [aug.sample(w, h) for h, w in sizes])


def test_fp32_and_stem_buffer_outputs():
    """NCHW fp32 == the host path's tensor; the NHWC4 buffer == its bf16 rounding with channel 3 and the halo zero"""
    from yolo.dataset import AugParams as P, _Augment
    from yolo.engine import Act
    from yolo.inference import _Preprocess
    images = [_img(375, 500, 1), _img(500, 333, 2), _img(448, 448, 3)]
    params = [P(20, 31, 300, 410, (H, B, S), 1.2, 0.8, 0.03), P(0, 0, 500, 333, (S,), 1.0, 1.4, 0.0), P(0, 0, 448, 448)]
    batch = _batch(images, params).cuda()
    aug, fin = _Augment((448, 448)), _Preprocess()
    ref = torch.stack([fin(aug.apply(Image.fromarray(im), [], p)[0]) for im, p in zip(images, params)])
    out = batch.to_tensor()
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), ref)
    assert torch.equal(batch.cpu().to_tensor(), ref)
    act = Act(3, 448, 448, 4, 3, batch.device)
    batch.into_act(act)
    v = act.view().float().cpu()
    inner = v[:, 3:-3, 3:-3, :]
    assert torch.equal(inner[..., :3].permute(0, 3, 1, 2), ref.to(torch.bfloat16).float())
    assert inner[..., 3].abs().sum() == 0 and v[:, :3].abs().sum() == 0 and v[:, -3:].abs().sum() == 0
    assert v[:, :, :3].abs().sum() == 0 and v[:, :, -3:].abs().sum() == 0


def test_identity_parameters_equal_preprocess_u8():
    from yolo.dataset import AugParams as P
    from yolo.preprocess import preprocess_u8
    rng = np.random.default_rng(8)
    for hw in [(375, 500), (448, 448), (448, 300)]:
        imgs = rng.integers(0, 256, size=(3,) + hw + (3,), dtype=np.uint8)
        ref, ract = preprocess_u8(torch.from_numpy(imgs).cuda(), (448, 448), nhwc4_halo=3)
        batch = _batch(list(imgs), [P(0, 0, hw[0], hw[1])] * 3).cuda()
        assert torch.equal(batch.to_tensor(), ref)
        from yolo.engine import Act
        act = Act(3, 448, 448, 4, 3, batch.device)
        batch.into_act(act)
        assert torch.equal(act.t, ract.t)


def test_nothing_is_written_past_the_outputs():
    """guard regions behind every output (and the scratch of the horizontal pass is the library's own allocation: checked through the
    outputs being exact); the last image of the batch is the smallest"""
    from yolo import _hip
    from yolo.dataset import AugParams as P
    import ctypes
    images = [_img(375, 500, 1), _img(200, 300, 2), _img(37, 53, 3)]
    params = [P(5, 5, 300, 400, (B, S, H), 1.2, 0.8, 0.05), P(0, 0, 200, 300, (H,), 1.0, 1.0, -0.05), P(1, 1, 30, 50, (S,), 1.0, 1.2, 0.0)]
    batch = _batch(images, params).cuda()
    N, G = 3, 4096
    n_f32, n_u8 = N * 3 * 448 * 448, N * 448 * 448 * 3
    f32 = torch.full((n_f32 + G,), 7.0, device="cuda")
    u8 = torch.full((n_u8 + G,), 0xA5, dtype=torch.uint8, device="cuda")
    tmp = torch.full((batch._tmp_bytes + G,), 0x5A, dtype=torch.uint8, device="cuda")
    m3, s3 = (ctypes.c_float * 3)(*batch.mean), (ctypes.c_float * 3)(*batch.std)
    _hip.check(_hip.lib().yolo_augment_u8(_hip.ptr(batch.data), batch.data.numel(), batch._descs, _hip.ptr(batch._descs_dev), N, 448, 448, _hip.ptr(tmp),
                                          batch._tmp_bytes, m3, s3, None, 0, _hip.ptr(f32), _hip.ptr(u8), _hip.stream()), "yolo_augment_u8")
    torch.cuda.synchronize()
    assert (f32[n_f32:] == 7.0).all() and (u8[n_u8:] == 0xA5).all() and (tmp[batch._tmp_bytes:] == 0x5A).all()
    assert np.array_equal(u8[:n_u8].view(N, 448, 448, 3).cpu().numpy(), _host_u8(images, params))
    assert torch.equal(f32[:n_f32].view(N, 3, 448, 448), batch.to_tensor())


def _voc(tmp_path):
    from test_dataset_cpu import _make_voc
    samples = {"000001": (500, 375, [("dog", 48, 240, 195, 371), ("person", 8, 12, 352, 498)]),
               "000002": (320, 480, [("car", 100, 100, 200, 300)]),
               "000003": (200, 200, [("cat", 20, 30, 150, 190)]),
               "000004": (400, 300, [("cat", 0, 0, 400, 300)])}
    for year, sets in (("2007", {"trainval": list(samples)}), ("2012", {"train": list(samples), "val": ["000003", "000004"]})):
        _make_voc(tmp_path, year, samples, sets)
    return tmp_path


def test_yolov1_trains_from_a_u8_batch(tmp_path):
    """train() mode, same seed: the stem input buffer filled from the U8Batch is bit-identical to the one filled from the host-augmented fp32
    batch; predictions agree within the project's bound for two forwards of one input (test_gpu_preprocess.py: the split-K Linear's fp32
    atomics); an optimizer step runs and every parameter gradient is finite and non-zero"""
    from yolo import YOLOLoss, YOLOv1
    from yolo.augment import collate_u8
    from yolo.dataset import VOCDetectionYOLO
    from yolo.optim import Adam
    root = _voc(tmp_path)
    host = VOCDetectionYOLO(root=root, year="2012", image_set="train", augment=True)
    dev = VOCDetectionYOLO(root=root, year="2012", image_set="train", augment=True, device_transform=True)
    torch.manual_seed(21)
    hs = [host[i] for i in range(4)]
    torch.manual_seed(21)
    batch, targets = collate_u8([dev[i] for i in range(4)])
    x = torch.stack([s[0] for s in hs]).cuda()
    assert torch.equal(targets, torch.stack([s[1] for s in hs]))
    torch.manual_seed(0)
    m = YOLOv1().cuda().train()
    m.head[3].p = 0.0                      # dropout off (the plan reads p at every forward): two forwards of one input are compared
    # the stem's input buffer, filled by the two routes Plan.forward uses
    from yolo._hip import check, lib, ptr, stream
    from yolo.engine import Act
    a, b = Act(4, 448, 448, 4, 3, x.device), Act(4, 448, 448, 4, 3, x.device)
    check(lib().yolo_nchw_f32_to_nhwc_bf16(ptr(x), 4, 3, 448, 448, a.p, 4, 3, 3, stream()), "nchw->nhwc4")
    batch.cuda().into_act(b)
    assert torch.equal(a.store, b.store)
    ref = m(x).detach()
    got = m(batch.cuda())
    torch.testing.assert_close(got.detach(), ref, rtol=0, atol=1e-3 * ref.abs().mean().item())
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.zero_grad()
    loss, _ = YOLOLoss()(got, targets.cuda())
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
    before = m.head[4].bias.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, m.head[4].bias.detach())
    with pytest.raises(RuntimeError, match="no input gradient"):
        batch.requires_grad_(True)
    m.cpu()


def test_resnet_model_takes_a_u8_batch():
    from yolo import ResNetBackbone, YOLOv1
    from yolo.dataset import AugParams as P
    images = [_img(375, 500, 1), _img(300, 333, 2)]
    batch = _batch(images, [P(20, 31, 300, 410, (H, B, S), 1.2, 0.8, 0.03), P(0, 0, 300, 333)]).cuda()
    torch.manual_seed(1)
    m = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=True)).cuda().eval()
    with torch.no_grad():
        ref = m(batch.cpu().to_tensor().cuda())
        got = m(batch)
    assert got.shape == (2, 7, 7, 30)
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-3 * ref.abs().mean().item())
    m.cpu()


def test_train_cli_with_device_augment(tmp_path):
    root = _voc(tmp_path / "data")
    ck = tmp_path / "ck"
    common = [sys.executable, os.path.join(ROOT, "yolo-v1_amd", "train.py"), "--backbone", "yolov1", "--batch-size", "2", "--num-workers", "0", "--device-augment",
              "--voc-root", str(root), "--checkpoint-dir", str(ck), "--save-frequency", "1"]
    for extra, epoch in ((["--epochs", "1"], 1), (["--epochs", "2", "--resume", str(ck / "yolo_latest.pth")], 2)):
        r = subprocess.run(common + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "done:" in r.stdout, f"--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
        st = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
        assert st["epoch"] == epoch and all(torch.isfinite(v).all() for v in st["model_state_dict"].values())
