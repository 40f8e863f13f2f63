"""GPU: class-specific scoring (scoring="all") -- yolo_decode_classes through the C ABI, the grouped yolo_nms / yolo_map_match
path, mAPMetric, YOLOInference and evaluate.py -- against tests/scoring_ref.py.  Bar: records, counts, kept indices and
orders bit for bit; metric keys to 1e-12."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scoring_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NMS_THR = 0.4
FILL = -7.25            # no record field and no count ever holds it
BAND = 96               # guard elements in front of and behind each output
KINDS = {"random": R.random_pred, "tied": R.tied_pred, "overlap": R.overlap_pred}


@functools.lru_cache(maxsize=None)
def _pred(shape, kind):
    p = KINDS[kind](*shape)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _ref_groups(shape, kind, thr):
    """per image the C lists of scoring_ref, computed once per (case, threshold) and shared"""
    N, S, B, C = shape
    return tuple(R.decode_classes(_pred(shape, kind)[n], thr, S, B, C) for n in range(N))


@functools.lru_cache(maxsize=None)
def _thresholds(shape, kind):
    N, S, B, C = shape
    return tuple(R.thresholds(_pred(shape, kind), S, B, C))


def _ids(shape, kind):
    return f"{'x'.join(map(str, shape))}-{kind}"


def _abi_decode_classes(pred_np, shape, thr):
    """yolo_decode_classes on guarded buffers -> rec (N,C,M,6), counts (N,C) host arrays; the guard bands are checked here"""
    from yolo import _hip
    N, S, B, C = shape
    M = S * S * B
    pred = torch.zeros(max(1, pred_np.size), dtype=torch.float32, device="cuda")
    pred[: pred_np.size] = torch.from_numpy(np.array(pred_np, np.float32)).reshape(-1).cuda()
    rec = torch.full((BAND + N * C * M * 6 + BAND,), FILL, dtype=torch.float64, device="cuda")
    cnt = torch.full((BAND + N * C + BAND,), -77, dtype=torch.int32, device="cuda")
    rc = _hip.lib().yolo_decode_classes(ctypes.c_void_p(pred.data_ptr()), N, S, B, C, float(thr), ctypes.c_void_p(rec.data_ptr() + BAND * 8),
                                        ctypes.c_void_p(cnt.data_ptr() + BAND * 4), _hip.stream())
    assert rc == 0, _hip.lib().yolo_hip_last_error()
    torch.cuda.synchronize()
    rec_h, cnt_h = rec.cpu().numpy(), cnt.cpu().numpy()
    assert np.all(rec_h[:BAND] == FILL) and np.all(rec_h[BAND + N * C * M * 6:] == FILL), "guard band of rec"
    assert np.all(cnt_h[:BAND] == -77) and np.all(cnt_h[BAND + N * C:] == -77), "guard band of counts"
    return rec_h[BAND: BAND + N * C * M * 6].reshape(N, C, M, 6), cnt_h[BAND: BAND + N * C].reshape(N, C)


@pytest.mark.parametrize("shape,kind", [pytest.param(s, k, id=_ids(s, k)) for s in R.SHAPES for k in ("random", "tied")])
def test_decode_classes_abi_bit_exact(shape, kind):
    N, S, B, C = shape
    M = S * S * B
    pred = _pred(shape, kind)
    names = [n for n, _ in _thresholds(shape, kind)]
    assert names == (["below", "above", "equal"] if N else ["below", "above"])
    for name, thr in _thresholds(shape, kind):
        rec, cnt = _abi_decode_classes(pred, shape, thr)
        ref = _ref_groups(shape, kind, thr)
        for n in range(N):
            for c in range(C):
                want = R.as_array(ref[n][c])
                assert cnt[n, c] == len(want), (name, n, c)
                assert np.array_equal(rec[n, c, : cnt[n, c]], want), (name, n, c)
                assert np.all(rec[n, c, cnt[n, c]:] == FILL), "rows behind counts are not written"
        if name == "below":
            assert np.all(cnt == M)
        elif name == "above":
            assert np.all(cnt == 0)
        else:
            valid = np.arange(M)[None, None, :] < cnt[..., None]
            assert not np.any(rec[..., 1][valid] == thr), "a score equal to the threshold is dropped"
            assert any(r[1] == thr for g in _ref_groups(shape, kind, -1.0) for rows in g for r in rows), "the threshold is a score that occurs"
    if kind == "tied" and N:
        scores = [r[1] for g in _ref_groups(shape, kind, -1.0) for rows in g for r in rows]
        assert len(set(scores)) <= 10 < len(scores) or len(scores) <= 10, "quarters times quarters: at most ten distinct scores"


def test_decode_classes_error_returns():
    from yolo import _hip
    L = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    null = ctypes.c_void_p(None)
    call = lambda pred, N, S, B, C, rec, cnt: L.yolo_decode_classes(pred, N, S, B, C, 0.5, rec, cnt, _hip.stream())
    assert call(null, 1, 1, 1, 1, p, p) == _hip.E_ARG
    assert call(p, 1, 1, 1, 1, null, p) == _hip.E_ARG
    assert call(p, 1, 1, 1, 1, p, null) == _hip.E_ARG
    assert call(p, -1, 1, 1, 1, p, p) == _hip.E_ARG
    assert call(p, 1, 1, 1, 0, p, p) == _hip.E_ARG
    assert b"yolo_decode_classes" in L.yolo_hip_last_error()
    assert call(p, 1, 33, 1, 1, p, p) == _hip.E_UNSUPPORTED          # S*S*B = 1089 > 1024
    assert call(p, 1, 1, 9, 1, p, p) == _hip.E_UNSUPPORTED           # B > 8
    assert call(p, 0, 7, 2, 20, p, p) == 0                           # an empty batch succeeds and writes nothing
    torch.cuda.synchronize()
    assert not buf.any()


def _path_cases():
    for shape in R.SHAPES:
        if shape[0] == 0:
            continue
        for kind in KINDS:
            yield pytest.param(shape, kind, id=_ids(shape, kind))


@pytest.mark.parametrize("shape,kind", list(_path_cases()))
def test_whole_device_path_bit_exact(shape, kind):
    """decode_classes + yolo_nms on the N*C groups (S*S*B > 128: nms_big_kernel), both variants: the records and kept indices of
    every group, and the per-image list and order of postprocess_host"""
    from yolo import ops
    N, S, B, C = shape
    M = S * S * B
    pred = torch.from_numpy(_pred(shape, kind).copy()).cuda()
    thr = dict(_thresholds(shape, kind))["equal"]
    ref = _ref_groups(shape, kind, thr)
    rec, cnt = ops.decode_classes(pred, thr, S, B, C)
    assert rec.shape == (N, C, M, 6) and cnt.shape == (N, C)
    rec_h, cnt_h = rec.cpu().numpy(), cnt.cpu().numpy()
    for variant in (R.INFERENCE, R.METRICS):
        keep, kc = ops.nms(rec.view(N * C, M, 6), cnt.view(N * C), NMS_THR, variant)
        keep_h, kc_h = keep.view(N, C, M).cpu().numpy(), kc.view(N, C).cpu().numpy()
        res = ops.postprocess_host(pred, thr, NMS_THR, variant, S, B, C, scoring="all")
        assert len(res) == N
        for n in range(N):
            rrec, rkeep, per_class = R.image_result(ref[n], NMS_THR, variant)
            for c in range(C):
                assert np.array_equal(rec_h[n, c, : cnt_h[n, c]], R.as_array(ref[n][c])), (variant, n, c)
                assert keep_h[n, c, : kc_h[n, c]].tolist() == per_class[c], (variant, n, c)
            got_rec, got_keep = res[n]
            assert np.array_equal(got_rec, R.as_array(rrec)), (variant, n)
            assert got_keep.tolist() == rkeep, (variant, n)
    if kind == "overlap" and M >= 72:
        assert kc_h.sum() < cnt_h.sum(), "NMS suppressed something"


@pytest.mark.parametrize("kind", ["random", "tied"])
def test_every_argmax_record_is_in_the_group_of_its_class(kind):
    from yolo import ops
    shape = (3, 7, 2, 20)
    pred = torch.from_numpy(_pred(shape, kind).copy()).cuda()
    for thr in (-1.0, 0.0, 0.2):
        arec, acnt = (t.cpu().numpy() for t in ops.decode(pred, thr, 7, 2, 20))
        rec, cnt = (t.cpu().numpy() for t in ops.decode_classes(pred, thr, 7, 2, 20))
        for n in range(3):
            assert acnt[n] > 0
            for row in arec[n, : acnt[n]]:
                c = int(row[0])
                assert np.any(np.all(rec[n, c, : cnt[n, c]] == row, axis=1)), (thr, n, row)


@pytest.mark.parametrize("conf_thr", [0.0, 0.2])
def test_one_hot_class_vectors_give_the_argmax_detections(conf_thr):
    """exactly one positive class per cell: "all" returns the detections of ops.decode + ops.nms, in the same per-image order
    (inference variant); in the metrics variant the default lists the classes in first-appearance order and "all" ascending, so
    the lists are compared class by class"""
    from yolo import ops
    S, B, C = 7, 2, 20
    pred = torch.from_numpy(R.one_hot_pred(3, S, B, C)).cuda()
    for variant in (R.INFERENCE, R.METRICS):
        arg = ops.postprocess_host(pred, conf_thr, NMS_THR, variant, S, B, C)
        every = ops.postprocess_host(pred, conf_thr, NMS_THR, variant, S, B, C, scoring="all")
        for (arec, akeep), (rec, keep) in zip(arg, every):
            assert len(akeep) > 3
            if variant == R.INFERENCE:
                assert np.array_equal(rec[keep], arec[akeep])
            else:
                assert len(keep) == len(akeep)
                for c in range(C):
                    assert np.array_equal(rec[keep][rec[keep, 0] == c], arec[akeep][arec[akeep, 0] == c])


def test_metric_on_device_tensors_equals_the_cpu_result():
    """map_case inputs through mAPMetric(scoring="all").update on device tensors (yolo_decode_classes, grouped yolo_nms, grouped
    yolo_map_match) == the same metric on CPU tensors; then the host matching on the very same device-built lists"""
    from yolo import mAPMetric
    d = np.load(os.path.join(GOLDEN, "map_case.npz"))
    pred, tgt = torch.from_numpy(d["pred"]), torch.from_numpy(d["tgt"])
    cpu = mAPMetric(20, conf_threshold=0.05, nms_threshold=0.4, scoring="all")
    cpu.update(pred, tgt)
    want = cpu.compute()
    m = mAPMetric(20, conf_threshold=0.05, nms_threshold=0.4, scoring="all")
    half = pred.shape[0] // 2
    m.update(pred[:half].cuda(), tgt[:half].cuda())
    m.update(pred[half:].cuda(), tgt[half:].cuda())
    assert m._dev_images == pred.shape[0] == len(m.all_predictions) and len(m._dev) == 2, "the device matching path must have been taken"
    assert m.all_predictions == cpu.all_predictions
    fast = m.compute()
    m._dev_images = -1             # the host protocol on the same lists
    slow = m.compute()
    assert set(fast) == set(slow) == set(want) and len(want) > 70
    for k, v in want.items():
        assert float(fast[k]) == pytest.approx(float(v), abs=1e-12), k
        assert float(slow[k]) == pytest.approx(float(v), abs=1e-12), k
    assert want["mAP50"] > 0.3


class _Tiny(torch.nn.Module):
    """(1,3,448,448) -> (1,7,7,30) in (0,1): a 7x7 average pool and one fixed 3 -> 30 map -- synthetic weights, no training"""
    S, B = 7, 2

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(3, 30, generator=g) * 4.0)
        self.b = torch.nn.Parameter(torch.randn(30, generator=g) * 0.5)
        self.last = None

    def forward(self, x):
        y = torch.sigmoid(torch.nn.functional.adaptive_avg_pool2d(x, 7).permute(0, 2, 3, 1) @ self.w + self.b)
        self.last = y.detach()
        return y


class _Fixed(torch.nn.Module):
    S, B = 7, 2

    def __init__(self, pred):
        super().__init__()
        self.pred = pred

    def forward(self, x):
        return self.pred


def test_predict_on_a_gpu_model_equals_the_cpu_engine(tmp_path, monkeypatch):
    from PIL import Image
    from yolo import _post_cpu
    from yolo.inference import YOLOInference
    img = tmp_path / "img.png"
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (120, 160, 3), dtype=np.uint8)).resize((500, 375), Image.BILINEAR).save(img)
    model = _Tiny().cuda()
    gpu = YOLOInference(model, device="cuda")
    host_nms = []
    orig = _post_cpu.nms
    monkeypatch.setattr(_post_cpu, "nms", lambda *a, **k: host_nms.append(1) or orig(*a, **k))
    got = gpu.predict(str(img), conf_threshold=0.2, nms_threshold=NMS_THR, scoring="all")
    assert not host_nms, "a GPU model must not take the host NMS loop"
    pred = model.last.cpu()
    assert pred.shape == (1, 7, 7, 30)
    cpu = YOLOInference(_Fixed(pred), device="cpu")
    want = cpu.predict(str(img), conf_threshold=0.2, nms_threshold=NMS_THR, scoring="all")
    assert len(want) > 5 and got == want                               # class ids, confidences and boxes exact, same order
    assert [d.confidence for d in got] == sorted((d.confidence for d in got), reverse=True)
    boxes = {(d.bbox.x, d.bbox.y, d.bbox.width, d.bbox.height) for d in got}
    assert len(boxes) < len(got), "a box comes out under several classes"
    assert gpu.parse_predictions(model.last[0], 0.2, scoring="all") == cpu.parse_predictions(pred[0], 0.2, scoring="all")
    assert gpu.predict(str(img), conf_threshold=0.2, nms_threshold=NMS_THR) == cpu.predict(str(img), conf_threshold=0.2, nms_threshold=NMS_THR)


def _evaluate(args, cwd):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--synthetic", "8", "--backbone", "yolov1", "--batch-size", "8"] + args,
                       cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"


def test_evaluate_command_line(tmp_path):
    """evaluate.py --scoring all and the default, on the device.  A seeded checkpoint makes the runs comparable: a constant last
    bias lifts every confidence and class score to about 0.3, so both modes have candidates above evaluate.py's 0.01."""
    from yolo import YOLOv1, YOLOv1Backbone
    torch.manual_seed(0)
    sd = YOLOv1(backbone=YOLOv1Backbone(), num_classes=20).state_dict()
    sd["head.4.bias"].fill_(0.3)
    ck = tmp_path / "seeded.pth"
    torch.save({"model_state_dict": sd}, ck)
    del sd
    common = ["--checkpoint", str(ck)]
    _evaluate(common + ["--scoring", "all", "--output", str(tmp_path / "all.txt")], str(tmp_path))
    _evaluate(common + ["--scoring", "argmax", "--output", str(tmp_path / "argmax.txt")], str(tmp_path))
    _evaluate(common + ["--output", str(tmp_path / "plain.txt")], str(tmp_path))
    plain = (tmp_path / "plain.txt").read_bytes()
    assert (tmp_path / "argmax.txt").read_bytes() == plain and b"scoring" not in plain
    lines = (tmp_path / "all.txt").read_text().strip().splitlines()
    assert lines[-1] == "scoring: all"
    keys = dict(line.split(": ") for line in lines)
    assert set(keys) - {"scoring"} == set(dict(line.split(": ") for line in plain.decode().strip().splitlines()))
    assert 0.0 <= float(keys["mAP50"]) <= 1.0
