"""GPU: batched detection -- yolo_detect_finish through the C ABI against tests/detect_ref.py (every output word, bit for bit),
U8Batch.from_images against the host transform, YOLOInference.predict_batch / predict_batch_arrays and predict.py --batch-size
against the per-batch composition they replace (model -> ops.postprocess_host -> _records_to_detections), exactly."""

import ctypes
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import detect_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
NMS_THR = 0.4
FILL, IFILL = -7.25, -77          # no output word ever holds them
BAND = 64                         # guard rows / ints in front of and behind each output
SIZES = [(500, 375), (375, 500), (480, 360), (333, 500), (448, 448), (97, 61), (640, 427), (500, 333)]      # (W, H)


# ------------------------------------------------------------------------------------------------ yolo_detect_finish
def _groups(pred_np, conf, S, B, C, scoring):
    """decode + NMS (inference variant) on the device, both checked bit for bit elsewhere (test_gpu_postprocess / test_gpu_scoring)"""
    from yolo import ops
    pred = torch.from_numpy(np.array(pred_np, np.float32)).cuda()
    if scoring == "all":
        rec, cnt = ops.decode_classes(pred, conf, S, B, C)
        rec, cnt, gpi = rec.view(-1, S * S * B, 6), cnt.view(-1), C
    else:
        (rec, cnt), gpi = ops.decode(pred, conf, S, B, C), 1
    keep, kc = ops.nms(rec, cnt, NMS_THR, ops._hip.NMS_INFERENCE)
    return rec, keep, kc, gpi


def _finish(rec, keep, kc, gpi, wh):
    """one yolo_detect_finish launch on pre-filled, guarded outputs -> (det rows, image, off) as lists; everything the entry must not
    write -- the guard bands and every row from ``total`` on -- is checked here to still hold the fill pattern"""
    from yolo import _hip
    n_groups, M = keep.shape
    rows, n_img = n_groups * M, n_groups // gpi
    det = torch.full(((BAND + rows + BAND) * 6,), FILL, dtype=torch.float64, device="cuda")
    image = torch.full((BAND + rows + BAND,), IFILL, dtype=torch.int32, device="cuda")
    off = torch.full((BAND + n_img + 1 + BAND,), IFILL, dtype=torch.int32, device="cuda")
    wh_d = None if wh is None else torch.tensor(wh, dtype=torch.float64, device="cuda").reshape(n_img, 2)
    vp = ctypes.c_void_p
    rc = _hip.lib().yolo_detect_finish(_hip.ptr(rec), _hip.ptr(keep), _hip.ptr(kc), n_groups, M, gpi, _hip.ptr(wh_d), vp(det.data_ptr() + BAND * 48),
                                       vp(image.data_ptr() + BAND * 4), vp(off.data_ptr() + BAND * 4), _hip.stream())
    assert rc == 0, _hip.lib().yolo_hip_last_error()
    torch.cuda.synchronize()
    det_h, image_h, off_h = det.cpu().numpy().reshape(-1, 6), image.cpu().numpy(), off.cpu().numpy()
    assert np.all(off_h[:BAND] == IFILL) and np.all(off_h[BAND + n_img + 1:] == IFILL), "guard band of out_off"
    off_l = off_h[BAND: BAND + n_img + 1].tolist()
    total = off_l[-1]
    assert 0 <= total <= rows
    assert np.all(det_h[:BAND] == FILL) and np.all(det_h[BAND + total:] == FILL), "rows behind total / guard band of out_det"
    assert np.all(image_h[:BAND] == IFILL) and np.all(image_h[BAND + total:] == IFILL), "rows behind total / guard band of out_image"
    return det_h[BAND: BAND + total].tolist(), image_h[BAND: BAND + total].tolist(), off_l


def _check_case(pred_np, conf, S, B, C, sizes=SIZES):
    """both scoring modes, with and without img_wh, two launches each; returns the per-image row counts of (argmax, all)"""
    counts = []
    for scoring in ("argmax", "all"):
        rec, keep, kc, gpi = _groups(pred_np, conf, S, B, C, scoring)
        rec_h, keep_h, kc_h = rec.cpu().numpy(), keep.cpu().numpy(), kc.cpu().numpy()
        for wh in (None, [sizes[n % len(sizes)] for n in range(len(pred_np))]):
            want = D.detect_finish(rec_h, keep_h, kc_h, gpi, wh)
            got = _finish(rec, keep, kc, gpi, wh)
            assert got[2] == want[2] and got[1] == want[1], (scoring, wh is not None)
            assert D.bits(got[0]) == D.bits(want[0]), (scoring, wh is not None)
            again = _finish(rec, keep, kc, gpi, wh)
            assert D.bits(again[0]) == D.bits(got[0]) and again[1:] == got[1:], "two launches on the same input"
        counts.append(np.diff(want[2]).tolist())
    return counts


@functools.lru_cache(maxsize=None)
def _random_pred(N, S, B, C, seed=0):
    p = np.random.RandomState(seed).rand(N, S, S, 5 * B + C).astype(np.float32)
    p.setflags(write=False)
    return p


def test_finish_on_the_golden_predictions(golden):
    g = golden("post_cases.npz")
    rows = 0
    for name in g["names"]:
        pred, (conf, _) = g[f"{name}__pred"], g[f"{name}__thr"]
        rows += sum(map(sum, _check_case(pred, float(conf), 7, 2, 20)))
    assert rows > 5000


def test_finish_many_rows():
    """conf 0.01 on uniform random predictions: nearly every (box, class) pair is a candidate"""
    argmax, every = _check_case(_random_pred(3, 7, 2, 20), 0.01, 7, 2, 20)
    assert max(every) > 200 and min(argmax) > 0


@pytest.mark.parametrize("N,empty", [(3, (0, 1, 2)), (5, (0, 2, 4)), (6, (0, 2, 3, 5))])
def test_finish_offsets_around_images_without_detections(N, empty):
    """conf 0.5 with the first, middle and the last image left without a detection: their offsets repeat"""
    pred = _random_pred(N, 7, 2, 20, seed=1).copy()
    pred[list(empty), :, :, 4] = 0.0
    pred[list(empty), :, :, 9] = 0.0
    for counts in _check_case(pred, 0.5, 7, 2, 20):
        assert [n for n in range(N) if counts[n] == 0] == list(empty)


def test_finish_keeps_the_list_order_of_equal_scores():
    """conf_b * prob_c equal across classes and across boxes (0.75 * 0.75 and 0.5 * 0.5, exact): the order is that of the list alone"""
    pred = np.zeros((2, 7, 7, 30), np.float32)
    pred[..., 0:2] = pred[..., 5:7] = 0.5
    pred[..., 2:4] = 0.125            # boxes of neighbouring cells do not meet
    pred[..., 7:9] = 0.0625           # box 1 inside box 0: IoU 0.25 < 0.4, both stay
    pred[..., 4], pred[..., 9] = 0.75, 0.75
    pred[0, ::2, :, 4] = 0.5
    pred[..., 10 + 3] = pred[..., 10 + 4] = pred[..., 10 + 17] = 0.75
    pred[1, :, 1::3, 10 + 9] = 0.5
    argmax, every = _check_case(pred, 0.2, 7, 2, 20)
    assert every[0] == 3 * 98 and every[1] > 3 * 98 and argmax == [98, 98]


def test_finish_small_grid():
    _check_case(_random_pred(4, 3, 1, 2), 0.1, 3, 1, 2)


def test_finish_beyond_the_staged_scores():
    """20 groups of 588 = 11760 > 4096: the header promises the same ranking out of global memory, no shape refused"""
    argmax, every = _check_case(_random_pred(1, 14, 3, 20), 0.01, 14, 3, 20)
    assert every[0] > 4096


def test_finish_without_groups():
    from yolo import _hip
    off = torch.full((3,), IFILL, dtype=torch.int32, device="cuda")
    one = torch.full((6,), FILL, dtype=torch.float64, device="cuda")
    kc = torch.zeros(1, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    for gpi in (1, 20):
        rc = _hip.lib().yolo_detect_finish(_hip.ptr(one), _hip.ptr(kc), _hip.ptr(kc), 0, 98, gpi, None, _hip.ptr(one), _hip.ptr(kc), vp(off.data_ptr() + 4), _hip.stream())
        assert rc == 0, _hip.lib().yolo_hip_last_error()
    torch.cuda.synchronize()
    assert off.tolist() == [IFILL, 0, IFILL] and one.tolist() == [FILL] * 6 and kc.tolist() == [0]


def test_ops_detect_and_detect_host():
    """the wrappers: three launches, worst-case sized device outputs; detect_host copies ``off`` and exactly ``total`` rows"""
    from yolo import ops
    pred = torch.from_numpy(_random_pred(3, 7, 2, 20)).cuda()
    wh = np.array(SIZES[:3], np.float64)
    for scoring in ("argmax", "all"):
        rec, keep, kc, gpi = _groups(_random_pred(3, 7, 2, 20), 0.3, 7, 2, 20, scoring)
        for size in (None, wh, torch.from_numpy(wh).cuda()):
            want = D.detect_finish(rec.cpu().numpy(), keep.cpu().numpy(), kc.cpu().numpy(), gpi, None if size is None else wh)
            det, image, off = ops.detect(pred, 0.3, NMS_THR, 7, 2, 20, scoring, size)
            assert det.is_cuda and det.shape == (rec.shape[0] * 98, 6) and image.shape == (rec.shape[0] * 98,) and off.shape == (4,)
            total = want[2][-1]
            assert off.tolist() == want[2] and image[:total].tolist() == want[1] and D.bits(det[:total].tolist()) == D.bits(want[0])
            det_h, image_h, off_h = ops.detect_host(pred, 0.3, NMS_THR, 7, 2, 20, scoring, size)
            assert det_h.shape == (total, 6) and image_h.dtype == np.int32 and off_h.dtype == np.int32
            assert off_h.tolist() == want[2] and image_h.tolist() == want[1] and D.bits(det_h.tolist()) == D.bits(want[0])
    with pytest.raises(ValueError):
        ops.detect(pred, 0.3, NMS_THR, 7, 2, 20, "x")
    with pytest.raises(RuntimeError):
        ops.detect(pred, 0.3, NMS_THR, 7, 2, 20, "all", wh[:2])


# ------------------------------------------------------------------------------------------------ U8Batch.from_images
def _noise_images(sizes, seed=2):
    rng = np.random.RandomState(seed)
    return [np.asarray(Image.fromarray(rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8)).resize((w, h), Image.BILINEAR)) for w, h in sizes]


def test_from_images_equals_the_host_transform():
    """448 x 448 (no resize table), a smaller and a larger non-square image: .to_tensor() == the stacked transform results, bit for bit"""
    from yolo.augment import U8Batch
    from yolo.inference import _Preprocess
    arrays = _noise_images([(448, 448), (97, 61), (640, 427)])
    want = torch.stack([_Preprocess()(Image.fromarray(a)) for a in arrays])
    batch = U8Batch.from_images([arrays[0], torch.from_numpy(arrays[1].copy()), arrays[2]]).to("cuda")
    assert batch._descs[0].hk == 0 and batch._descs[0].vk == 0 and batch._descs[1].hk > 0 and batch._descs[2].vk > 0
    assert torch.equal(batch.to_tensor().cpu(), want)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def detector():
    """the default YOLOv1, random weights; the last bias puts the scores of all but the first cells above 0.5 (margins between -0.02 and 0.26), gives every cell a second box inside the first (suppressed under one class, IoU 0.64) and two likely classes"""
    from yolo import YOLOv1
    from yolo.inference import YOLOInference
    torch.manual_seed(0)
    model = YOLOv1()
    bias = np.zeros((7, 7, 30), np.float32)
    cell = np.arange(49).reshape(7, 7)
    bias[..., 0:2] = bias[..., 5:7] = 0.5
    bias[..., 2:4], bias[..., 7:9] = 0.25, 0.2
    bias[..., 4] = 0.6 + 0.35 * cell / 48
    bias[..., 9] = bias[..., 4] - 0.05
    np.put_along_axis(bias[..., 10:], (cell % 20)[..., None], 0.8, -1)
    np.put_along_axis(bias[..., 10:], ((cell + 7) % 20)[..., None], 0.7, -1)
    with torch.no_grad():
        model.head[4].bias.copy_(torch.from_numpy(bias.reshape(-1)))
    return YOLOInference(model.cuda().eval(), device="cuda")


def _reference(engine, arrays, batch_size, conf, scoring, names=None):
    """model(U8Batch) -> ops.postprocess_host -> _records_to_detections, batch by batch: per image (detections, kept records, (W, H))"""
    from yolo import ops
    from yolo.augment import U8Batch
    out = []
    for i in range(0, len(arrays), batch_size):
        chunk = arrays[i: i + batch_size]
        with torch.no_grad():
            pred = engine.model(U8Batch.from_images(chunk).to("cuda"))
        for a, (rec, keep) in zip(chunk, ops.postprocess_host(pred, conf, NMS_THR, ops._hip.NMS_INFERENCE, 7, 2, 20, scoring)):
            dets = engine._records_to_detections(rec, names)
            out.append(([dets[k] for k in keep], rec[keep], (a.shape[1], a.shape[0])))
    return out


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    """five mixed-size images, as arrays and as PNG files"""
    folder = tmp_path_factory.mktemp("five")
    arrays = _noise_images(SIZES[:5])
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(folder / f"im{i}.png"))
        Image.fromarray(a).save(paths[-1])
    return arrays, paths


@pytest.mark.parametrize("scoring", ["argmax", "all"])
def test_predict_batch_equals_the_composition_it_replaces(detector, five, scoring):
    from yolo._post_cpu import voc_pixel_boxes
    arrays, paths = five
    ref = _reference(detector, arrays, 2, 0.5, scoring)
    counts = [len(r[0]) for r in ref]
    print("detections per image:", counts)
    assert min(counts) >= 1 and max(counts) > 20
    mixed = [paths[0], arrays[1], Image.open(paths[2]), torch.from_numpy(arrays[3].copy()), paths[4]]
    got = detector.predict_batch(mixed, conf_threshold=0.5, nms_threshold=NMS_THR, scoring=scoring, batch_size=2, workers=3)
    assert got == [r[0] for r in ref]
    idx, cls, score, box, sizes = detector.predict_batch_arrays(paths, conf_threshold=0.5, nms_threshold=NMS_THR, scoring=scoring, batch_size=2)
    kept = np.concatenate([r[1] for r in ref])
    assert sizes.tolist() == [list(r[2]) for r in ref] and idx.tolist() == [n for n, c in enumerate(counts) for _ in range(c)]
    assert cls.tolist() == kept[:, 0].astype(int).tolist() and D.bits([score.tolist()]) == D.bits([kept[:, 1].tolist()])
    want_box = np.concatenate([voc_pixel_boxes(r[1][:, 2:6], *r[2]) for r in ref])
    assert D.bits(box.tolist()) == D.bits(want_box.tolist())
    *same, xywh = detector.predict_batch_arrays(paths, conf_threshold=0.5, nms_threshold=NMS_THR, scoring=scoring, batch_size=2, normalized=True)
    assert D.bits(xywh.tolist()) == D.bits(kept[:, 2:6].tolist()) and all(np.array_equal(a, b) for a, b in zip(same, (idx, cls, score, box, sizes)))


def test_a_model_that_is_no_engine_plan_takes_the_fp32_batch(five):
    """any other device model: U8Batch.to_tensor() -- a last batch of one included"""
    from yolo import ops
    from yolo.augment import U8Batch
    from yolo.inference import YOLOInference

    class Tiny(torch.nn.Module):
        S, B = 7, 2

        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.conv = torch.nn.Conv2d(3, 30, 64, stride=64)

        def forward(self, x):
            assert isinstance(x, torch.Tensor) and x.dtype == torch.float32
            return torch.sigmoid(4 * self.conv(x)).permute(0, 2, 3, 1).contiguous()

    arrays, _ = five
    engine = YOLOInference(Tiny(), device="cuda")
    want = []
    for i in (0, 2, 4):
        with torch.no_grad():
            pred = engine.model(U8Batch.from_images(arrays[i: i + 2]).to("cuda").to_tensor())
        for rec, keep in ops.postprocess_host(pred, 0.3, NMS_THR, ops._hip.NMS_INFERENCE, 7, 2, 20, "all"):
            dets = engine._records_to_detections(rec, None)
            want.append([dets[k] for k in keep])
    assert sum(map(len, want)) > 20
    assert engine.predict_batch(arrays, conf_threshold=0.3, nms_threshold=NMS_THR, scoring="all", batch_size=2) == want


def test_broken_file_on_the_device_path(detector, five, tmp_path):
    import threading
    arrays, paths = five
    bad = str(tmp_path / "broken.png")
    open(bad, "wb").write(b"no image")
    before = set(threading.enumerate())
    with pytest.raises(RuntimeError) as e:
        detector.predict_batch(paths[:3] + [bad] + paths[3:], batch_size=2, workers=2)
    assert bad in str(e.value) and set(threading.enumerate()) <= before


def test_predict_cli_json_equals_predict_batch_arrays(detector, tmp_path, monkeypatch, capsys):
    """predict.py --batch-size 4 --json on a folder of six PNGs (batches of 4 and 2), in this process on the shared model"""
    folder = tmp_path / "six"
    folder.mkdir()
    for i, a in enumerate(_noise_images(SIZES[2:8], seed=4)):
        Image.fromarray(a).save(str(folder / f"p{i}.png"))
    spec = importlib.util.spec_from_file_location("predict_cli_gpu", os.path.join(PKG, "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "load_model", lambda *a, **k: detector.model)
    out = str(tmp_path / "det.json")
    monkeypatch.setattr(sys, "argv", ["predict.py", str(folder), "--device", "cuda", "--backbone", "yolov1", "--batch-size", "4", "--json", out, "--scoring", "all"])
    mod.main()
    text = capsys.readouterr().out
    paths = [str(folder / f"p{i}.png") for i in range(6)]
    idx, cls, score, box, sizes = detector.predict_batch_arrays(paths, scoring="all", batch_size=4)
    doc = json.load(open(out))
    assert [e["image"] for e in doc] == paths and [[e["width"], e["height"]] for e in doc] == sizes.tolist() == [list(s) for s in SIZES[2:8]]
    flat = [d for e in doc for d in e["detections"]]
    assert [len(e["detections"]) for e in doc] == np.bincount(idx, minlength=6).tolist() and len(flat) > 20
    assert [d["class_id"] for d in flat] == cls.tolist() and [d["class_name"] for d in flat] == [mod.VOC_CLASSES[c] for c in cls]
    assert D.bits([[d["confidence"]] + d["bbox"] for d in flat]) == D.bits(np.concatenate([score[:, None], box], 1).tolist())
    assert [line for line in text.splitlines() if not line.startswith(" ")] == [f"{p}: {n} detections" for p, n in zip(paths, np.bincount(idx, minlength=6))]
