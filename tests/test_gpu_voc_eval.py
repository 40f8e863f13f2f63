"""GPU: yolo_voc_match through the C ABI, VOCMetric on device tensors and evaluate.py --protocol voc against tests/voc_ref.py.
Bar: status words, classes, image indices, scores, boxes and the total bit for bit; metric keys to 1e-12."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import voc_cases as K
import voc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
BAND = 64                       # guard rows in front of and behind each output
FILL_F, FILL_I = -7.25, -77     # no output ever holds them
S, B, C, N = 3, 2, 3, 3
M = S * S * B


def _norm(box, W, H):
    """pixel corners -> the normalised centre box a record holds"""
    x1, y1, x2, y2 = box
    return ((x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H)


@functools.lru_cache(maxsize=None)
def crafted():
    """-> (wh, gts per image [(cls, difficult, box)], dets per (image, class) [(score, x, y, w, h)] in descending score)"""
    wh = [(200, 100), (100, 200), (200, 100)]
    A, D, E, F = (20, 20, 60, 60), (100, 20, 140, 60), (104, 20, 144, 60), (150, 50, 180, 90)
    tiles = [((k % 10) * 20, (k // 10) * 14, (k % 10) * 20 + 15, (k // 10) * 14 + 10) for k in range(70)]
    tiles[67] = tiles[3]                    # equal overlap inside one lane (slots 0 and 1): the first wins
    tiles[6] = tiles[5]                     # equal overlap in two lanes: the lower index wins
    gts = [
        [(1, False, A), (1, True, D), (1, False, E), (2, False, F), (2, False, F)],
        [],                                 # an image without ground truth
        [(0, False, (0, 0, 25, 12))] + [(1, k == 69, t) for k, t in enumerate(tiles)],
    ]
    n = lambda box, i: _norm(box, *wh[i])   # noqa: E731
    dets = {
        # image 0, class 0: no kept detection -- the first group is empty
        (0, 1): [(0.9, *n(A, 0)),                        # TP
                 (0.8, *n((22, 21, 62, 61), 0)),         # the second detection on A: FP
                 (0.7, *n(D, 0)),                        # best match D is difficult, the non-difficult E passes 0.5 too: ignored
                 (0.6, *n((101, 20, 141, 60), 0)),       # D again: ignored again
                 (0.5, *n(E, 0)),                        # E was not consumed: TP
                 (0.4, *n((150, 5, 190, 15), 0))],       # touches nothing: FP
        (0, 2): [(0.9, *n(F, 0)), (0.9, *n(F, 0))],      # two equal ground truths: both detections pick the first, the second is FP; tied scores
        (1, 0): [(0.8, 0.5, 0.5, 0.2, 0.2), (0.3, 0.2, 0.7, 0.1, 0.1)],
        # image 1, class 1: a group with no kept detection
        (1, 2): [(0.6, 0.05, 0.95, 0.3, 0.4)],           # clamped at the left and the bottom border
        (2, 0): [(0.7, 0.0625, 0.125, 0.125, 0.25),      # pixels (0, 0, 25, 25) exactly; ground truth (0, 0, 25, 12): overlap 338 / 676 = 0.5 exactly
                 (0.2, 1.0, 0.06, 0.26, 0.5)],           # clamped at the right and the top border, overlaps nothing
        (2, 1): [(0.95, *n(tiles[3], 2)), (0.9, *n(tiles[3], 2)), (0.85, *n(tiles[5], 2)), (0.8, *n(tiles[5], 2)), (0.75, *n(tiles[64], 2)),
                 (0.7, *n(tiles[69], 2)), (0.65, *n(tiles[0], 2)), (0.6, *n(tiles[63], 2)), (0.55, *n(tiles[65], 2)), (0.5, *n(tiles[64], 2))],
        # image 2, class 2: the last group is empty
    }
    return wh, gts, dets


THRESHOLD_SETS = {"T1": (0.5,), "T16": (0.5, 0.5000000001, 0.05, 0.1, 0.2, 0.3, 0.4, 0.45, 0.55, 0.6, 0.7, 0.8, 0.9, 0.95, 0.999, 1.0)}


def _layout(per_image):
    """crafted() as the arrays of the C ABI: rec / keep / counts for groups_per_image = C or 1 (records stored in reverse, ``keep`` puts
    them in order), the ground-truth table, and the lists of voc_ref in output order"""
    wh, gts, dets = crafted()
    groups = [[(c, d) for c in range(C) if per_image == 1 or c == g % C for d in dets.get((g // per_image, c), ())] for g in range(N * per_image)]
    rec = np.full((len(groups), M, 6), FILL_F, np.float64)
    keep = np.full((len(groups), M), FILL_I, np.int32)
    kc = np.array([len(g) for g in groups], np.int32)
    ref_dets = []
    for g, rows in enumerate(groups):
        assert len(rows) <= M
        for k, (c, d) in enumerate(rows):
            rec[g, M - 1 - k] = (c, *d)
            keep[g, k] = M - 1 - k
            ref_dets.append((g // per_image, c, *d))
    gt_off = np.concatenate(([0], np.cumsum([len(g) for g in gts]))).astype(np.int32)
    flat = [g for img in gts for g in img]
    gt = dict(box=np.array([g[2] for g in flat], np.float64), cls=np.array([g[0] for g in flat], np.int32),
              dif=np.array([g[1] for g in flat], np.uint8), off=gt_off, wh=np.array(wh, np.float64))
    ref_gts = [(i, g[0], g[1], *map(float, g[2])) for i, img in enumerate(gts) for g in img]
    return rec, keep, kc, gt, ref_dets, ref_gts, wh


def _abi(rec, keep, kc, per_image, gt, image_base, thresholds, max_gt=None):
    """yolo_voc_match on guarded outputs -> (score, cls_img, status, box, total); guard bands and the rows behind the total are checked here"""
    from yolo import _hip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    pad = lambda a, tail: np.concatenate([a.reshape((-1,) + tail), np.zeros((1,) + tail, a.dtype)])   # noqa: E731  (no empty allocations)
    d_rec, d_keep, d_kc = dev(rec), dev(keep), dev(pad(kc, ()))
    d_box, d_cls, d_dif, d_off, d_wh = dev(pad(gt["box"], (4,))), dev(pad(gt["cls"], ())), dev(pad(gt["dif"], ())), dev(gt["off"]), dev(pad(gt["wh"], (2,)))
    rows = rec.shape[0] * rec.shape[1]
    full = BAND + rows + BAND
    score = torch.full((full,), FILL_F, dtype=torch.float64, device="cuda")
    cls_img = torch.full((full, 2), FILL_I, dtype=torch.int32, device="cuda")
    status = torch.full((full,), FILL_I, dtype=torch.int32, device="cuda")
    box = torch.full((full, 4), FILL_F, dtype=torch.float64, device="cuda")
    total = torch.full((2 * BAND + 1,), FILL_I, dtype=torch.int32, device="cuda")
    thr = (ctypes.c_double * len(thresholds))(*thresholds)
    p = lambda t, skip=0: ctypes.c_void_p(t.data_ptr() + skip)   # noqa: E731
    if max_gt is None:
        max_gt = int(np.diff(gt["off"]).max())
    rc = _hip.lib().yolo_voc_match(p(d_rec), p(d_keep), p(d_kc), rec.shape[0], rec.shape[1], per_image, p(d_box), p(d_cls), p(d_dif), p(d_off), p(d_wh),
                                   max_gt, image_base, thr, len(thresholds), p(score, BAND * 8), p(cls_img, BAND * 8), p(status, BAND * 4),
                                   p(box, BAND * 32), p(total, BAND * 4), _hip.stream())
    assert rc == 0, _hip.lib().yolo_hip_last_error()
    torch.cuda.synchronize()
    score, cls_img, status, box, total = (t.cpu().numpy() for t in (score, cls_img, status, box, total))
    n = int(total[BAND])
    assert 0 <= n <= rows
    assert np.all(total[:BAND] == FILL_I) and np.all(total[BAND + 1:] == FILL_I), "guard band of the total"
    for name, a, fill in (("score", score, FILL_F), ("cls_img", cls_img, FILL_I), ("status", status, FILL_I), ("box", box, FILL_F)):
        assert np.all(a[:BAND] == fill) and np.all(a[BAND + rows:] == fill), f"guard band of {name}"
        assert np.all(a[BAND + n: BAND + rows] == fill), f"{name}: rows behind the total are not written"
    sl = slice(BAND, BAND + n)
    return score[sl], cls_img[sl], status[sl].view(np.uint32), box[sl], n


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(got, ref_dets, ref_gts, wh, thresholds, image_base):
    score, cls_img, status, box, n = got
    want_status, want_box = R.match(ref_dets, ref_gts, wh, thresholds)
    assert n == len(ref_dets)
    assert np.array_equal(_bits(score), _bits([d[2] for d in ref_dets]))
    assert cls_img[:, 0].tolist() == [d[1] for d in ref_dets] and cls_img[:, 1].tolist() == [image_base + d[0] for d in ref_dets]
    assert np.array_equal(_bits(box), _bits(want_box).reshape(-1, 4))
    assert status.tolist() == want_status
    return want_status, want_box


@pytest.mark.parametrize("image_base", [0, 7])
@pytest.mark.parametrize("tset", ["T1", "T16"])
@pytest.mark.parametrize("per_image", [C, 1], ids=["per_class", "per_image"])
def test_voc_match_abi_bit_exact(per_image, tset, image_base):
    rec, keep, kc, gt, ref_dets, ref_gts, wh = _layout(per_image)
    thresholds = THRESHOLD_SETS[tset]
    got = _abi(rec, keep, kc, per_image, gt, image_base, thresholds)
    status, box = _check(got, ref_dets, ref_gts, wh, thresholds, image_base)
    # the crafted cases do what they were crafted for (at threshold 0.5, the first of both sets)
    by_group = {}
    for d, s, b in zip(ref_dets, status, box):
        by_group.setdefault((d[0], d[1]), []).append((s & 3, b))
    st = lambda key: [s for s, _ in by_group[key]]   # noqa: E731
    assert st((0, 1)) == [R.TP, R.FP, R.IGNORED, R.IGNORED, R.TP, R.FP]
    assert st((0, 2)) == [R.TP, R.FP]
    assert st((1, 0)) == [R.FP, R.FP] and st((1, 2)) == [R.FP]
    assert by_group[(1, 2)][0][1] == (0.0, 150.0, 20.0, 200.0) and by_group[(2, 0)][1][1][2] == 200.0 and by_group[(2, 0)][1][1][1] == 0.0
    assert by_group[(2, 0)][0][1] == (0.0, 0.0, 25.0, 25.0) and st((2, 0)) == [R.TP, R.FP]
    assert st((2, 1)) == [R.TP, R.FP, R.TP, R.FP, R.TP, R.IGNORED, R.TP, R.TP, R.TP, R.FP]
    if per_image == C:
        assert kc[0] == 0 and kc[-1] == 0 and kc[4] == 0, "first, last and one inner group are empty"
    if tset == "T16":
        exact = status[[k for k, d in enumerate(ref_dets) if (d[0], d[1]) == (2, 0)][0]]
        assert (exact >> 0) & 3 == R.TP and (exact >> 2) & 3 == R.FP, "an overlap equal to the threshold passes, one above it does not"
        assert len(set(status)) > 3, "the thresholds tell the detections apart"


def test_voc_match_group_of_588_records():
    """S = 14, B = 3: one image is one group of 588 records, ordered by nms_big_kernel; ten chunks of 64 in the walk"""
    from yolo import ops
    rng = np.random.Generator(np.random.PCG64(9))
    S2, B2, C2 = 14, 3, 3
    pred = rng.uniform(0.05, 0.95, size=(1, S2, S2, 5 * B2 + C2)).astype(np.float32)
    pred[..., [2, 3, 7, 8, 12, 13]] *= 0.25                                           # small boxes: most survive the NMS
    rec, cnt = ops.decode(torch.from_numpy(pred).cuda(), -1.0, S2, B2, C2)
    keep, kc = ops.nms(rec, cnt, 0.6, 1)
    rec_h, keep_h, kc_h = rec.cpu().numpy(), keep.cpu().numpy(), kc.cpu().numpy()
    assert cnt.item() == 588 and 128 < kc_h[0] <= 588
    W, H = 320, 240
    boxes = np.array([[x, y, x + 50, y + 40] for x in (10, 90, 170, 250) for y in (10, 80, 150)], np.float64)
    gt = dict(box=boxes, cls=np.arange(12, dtype=np.int32) % C2, dif=(np.arange(12) % 4 == 1).astype(np.uint8), off=np.array([0, 12], np.int32),
              wh=np.array([[W, H]], np.float64))
    thresholds = (0.5, 0.1, 0.3)
    got = _abi(rec_h, keep_h, kc_h, 1, gt, 3, thresholds)
    ref_dets = [(0, int(r[0]), *map(float, r[1:])) for r in rec_h[0][keep_h[0, : kc_h[0]]]]
    ref_gts = [(0, int(c), bool(d), *map(float, b)) for b, c, d in zip(gt["box"], gt["cls"], gt["dif"])]
    status, _ = _check(got, ref_dets, ref_gts, [(W, H)], thresholds, 3)
    assert {(s >> 2) & 3 for s in status} == {R.FP, R.TP, R.IGNORED}


def test_voc_match_empty_batch_and_error_returns():
    """argument checks return before any launch; nothing here reaches a kernel with a bad argument"""
    from yolo import _hip
    L = _hip.lib()
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    tot = torch.full((1,), FILL_I, dtype=torch.int32, device="cuda")
    p, null = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(None)
    thr = (ctypes.c_double * 17)(*[0.5] * 17)

    def call(n_groups=3, M=18, per_image=1, T=1, max_gt=4, image_base=0, **ptrs):
        a = {k: ptrs.get(k, p) for k in ("rec", "keep", "kc", "box", "cls", "dif", "off", "wh", "score", "cls_img", "status", "obox")}
        return L.yolo_voc_match(a["rec"], a["keep"], a["kc"], n_groups, M, per_image, a["box"], a["cls"], a["dif"], a["off"], a["wh"], max_gt, image_base,
                                ptrs.get("thr", thr), T, a["score"], a["cls_img"], a["status"], a["obox"], ptrs.get("total", ctypes.c_void_p(tot.data_ptr())),
                                _hip.stream())

    assert call(T=17) == _hip.E_ARG and b"yolo_voc_match" in L.yolo_hip_last_error()
    assert call(T=0) == _hip.E_ARG
    assert call(max_gt=257) == _hip.E_ARG
    for name in ("rec", "keep", "kc", "box", "cls", "dif", "off", "wh", "score", "cls_img", "status", "obox", "total"):
        assert call(**{name: null}) == _hip.E_ARG, name
    assert call(thr=None) == _hip.E_ARG
    assert call(n_groups=-1) == _hip.E_ARG and call(M=0) == _hip.E_ARG and call(M=1025) == _hip.E_ARG and call(per_image=0) == _hip.E_ARG
    assert call(n_groups=4, per_image=3) == _hip.E_ARG and call(max_gt=-1) == _hip.E_ARG and call(image_base=-1) == _hip.E_ARG
    torch.cuda.synchronize()
    assert tot.item() == FILL_I and not buf.any(), "a refused call writes nothing"
    assert call(n_groups=0) == 0                                      # an empty batch succeeds: total 0, nothing else written
    torch.cuda.synchronize()
    assert tot.item() == 0 and not buf.any()


def _metric(scoring, ap_mode, thresholds=K.THRESHOLDS):
    from yolo.voc_eval import VOCGroundTruth, VOCMetric
    images, _ = K.split()
    return VOCMetric(K.C, VOCGroundTruth.from_images(images), iou_thresholds=thresholds, ap_mode=ap_mode, scoring=scoring, conf_threshold=K.CONF_THR,
                     nms_threshold=K.NMS_THR, S=K.S, B=K.B)


@functools.lru_cache(maxsize=None)
def _reference(scoring):
    images, pred = K.split()
    return K.ref_lists(images, [K.kept_records(pred[n], scoring) for n in range(K.N)])


@pytest.mark.parametrize("scoring", ["all", "argmax"])
@pytest.mark.parametrize("ap_mode", ["voc07", "area"])
def test_metric_on_device_tensors(scoring, ap_mode, monkeypatch):
    from yolo import _post_cpu
    images, pred = K.split()
    cpu = _metric(scoring, ap_mode)
    cpu.update(torch.from_numpy(pred.copy()), 0)
    host = []
    orig = _post_cpu.voc_match
    monkeypatch.setattr(_post_cpu, "voc_match", lambda *a, **k: host.append(1) or orig(*a, **k))
    m = _metric(scoring, ap_mode)
    m.update(torch.from_numpy(pred[:3].copy()).cuda(), 0)
    first = m._staging
    m.update(torch.from_numpy(pred[3:].copy()).cuda(), 3)
    assert not host and first is not None and m._staging is first, "device tensors take yolo_voc_match, into the same staging buffers"
    for a, b in zip(m._arrays(), cpu._arrays()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    dets, gts, wh = _reference(scoring)
    status, _ = R.match(dets, gts, wh, K.THRESHOLDS)
    assert m._arrays()[3].tolist() == status and len(status) > 40
    want = R.evaluate(dets, gts, wh, K.C, K.THRESHOLDS, ap_mode)
    K.close(m.compute(), want)
    K.close(cpu.compute(), want)
    assert 0.0 < want["mAP"] < 1.0 and want["num_ignored"] > 0


def test_metric_beyond_the_kernel_limits_takes_the_host_matching():
    """17 thresholds: decode and NMS on the device, matching on the host -- the same result as on CPU tensors"""
    _, pred = K.split()
    thresholds = tuple(0.1 + 0.05 * k for k in range(17))
    cpu, m = _metric("all", "area", thresholds), _metric("all", "area", thresholds)
    cpu.update(torch.from_numpy(pred.copy()), 0)
    m.update(torch.from_numpy(pred.copy()).cuda(), 0)
    assert m._staging is None
    for a, b in zip(m._arrays(), cpu._arrays()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    K.close(m.compute(), cpu.compute(), tol=0.0)


def _evaluate(args, cwd):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(PKG, "evaluate.py"), "--synthetic", "8", "--batch-size", "4", "--backbone", "yolov1"] + args,
                       cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r.stdout


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """seeded weights whose constant last bias lifts every confidence and class score to about 0.3: candidates above evaluate.py's 0.01"""
    from yolo import YOLOv1, YOLOv1Backbone
    torch.manual_seed(0)
    sd = YOLOv1(backbone=YOLOv1Backbone(), num_classes=20).state_dict()
    sd["head.4.bias"].fill_(0.3)
    path = tmp_path_factory.mktemp("voc_cli") / "seeded.pth"
    torch.save({"model_state_dict": sd}, path)
    return str(path)


def test_evaluate_command_line_voc_protocol(tmp_path, checkpoint):
    from yolo.dataset import VOC_CLASSES
    out = _evaluate(["--checkpoint", checkpoint, "--protocol", "voc", "--scoring", "all", "--write-detections", str(tmp_path / "det"),
                     "--output", str(tmp_path / "voc.txt")], str(tmp_path))
    lines = (tmp_path / "voc.txt").read_text().strip().splitlines()
    assert lines[-3:] == ["scoring: all", "protocol: voc", "ap_mode: voc07"]
    keys = dict(line.split(": ") for line in lines)
    assert "mAP" in keys and "mAP: " in out and int(float(keys["num_detections"])) > 0
    assert float(keys["mAP"]) != float(keys["mAP"]) or 0.0 <= float(keys["mAP"]) <= 1.0
    files = sorted(os.listdir(tmp_path / "det"))
    assert files == sorted(f"comp4_det_test_{n}.txt" for n in VOC_CLASSES) and len(files) == 20
    n_lines = sum(len(open(tmp_path / "det" / f).read().splitlines()) for f in files)
    assert n_lines == int(float(keys["num_detections"]))


def test_evaluate_command_line_grid_protocol_is_the_default(tmp_path, checkpoint):
    _evaluate(["--checkpoint", checkpoint, "--scoring", "all", "--protocol", "grid", "--output", str(tmp_path / "grid.txt")], str(tmp_path))
    _evaluate(["--checkpoint", checkpoint, "--scoring", "all", "--output", str(tmp_path / "plain.txt")], str(tmp_path))
    assert (tmp_path / "grid.txt").read_bytes() == (tmp_path / "plain.txt").read_bytes()
    assert b"protocol" not in (tmp_path / "plain.txt").read_bytes()
