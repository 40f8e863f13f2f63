"""CPU: the PASCAL VOC devkit evaluation (yolo/voc_eval.py, yolo/_post_cpu.py voc_match, the datasets' ground_truth) against the plain
restatement in tests/voc_ref.py.  Bar: status words and pixel boxes equal, every result key to 1e-12."""

import math
import os

import numpy as np
import pytest
import torch

import voc_cases as K
import voc_ref as R


def _metric(scoring, ap_mode, thresholds=K.THRESHOLDS):
    from yolo.voc_eval import VOCGroundTruth, VOCMetric
    images, _ = K.split()
    return VOCMetric(K.C, VOCGroundTruth.from_images(images), iou_thresholds=thresholds, ap_mode=ap_mode, scoring=scoring, conf_threshold=K.CONF_THR,
                     nms_threshold=K.NMS_THR, S=K.S, B=K.B)


def test_the_split_has_what_the_protocol_is_about():
    images, pred = K.split()
    n_gt = sum(len(g["class_ids"]) for g in images)
    cells = sum(len({(min(int(K.S * (b[1] + b[3]) / 2 / g["height"]), K.S - 1), min(int(K.S * (b[0] + b[2]) / 2 / g["width"]), K.S - 1))
                     for b in g["boxes"]}) for g in images)
    assert n_gt > cells, "objects that share a cell"
    assert 0 < sum(int(g["difficult"].sum()) for g in images) < n_gt
    assert all(g["width"] != g["height"] for g in images)


@pytest.mark.parametrize("scoring", ["all", "argmax"])
@pytest.mark.parametrize("ap_mode", ["voc07", "area"])
def test_host_path_equals_the_reference(scoring, ap_mode):
    images, pred = K.split()
    m = _metric(scoring, ap_mode)
    m.update(torch.from_numpy(pred[:3].copy()), 0)
    m.update(torch.from_numpy(pred[3:].copy()), 3)
    dets, gts, wh = K.ref_lists(images, [K.kept_records(pred[n], scoring) for n in range(K.N)])
    status, boxes = R.match(dets, gts, wh, K.THRESHOLDS)
    score, cls, img, got_status, got_box = m._arrays()
    assert len(dets) > 40 and len(score) == len(dets)
    assert score.tolist() == [d[2] for d in dets] and cls.tolist() == [d[1] for d in dets] and img.tolist() == [d[0] for d in dets]
    assert got_status.tolist() == status
    assert got_box.tolist() == [list(b) for b in boxes]
    kinds = {(s >> (2 * t)) & 3 for s in status for t in range(len(K.THRESHOLDS))}
    assert kinds == {R.FP, R.TP, R.IGNORED}
    want = R.evaluate(dets, gts, wh, K.C, K.THRESHOLDS, ap_mode)
    got = m.compute()
    K.close(got, want)
    assert 0.0 < got["mAP"] < 1.0 and got["num_ignored"] > 0 and "mAP@0.75" in got
    assert any(math.isnan(got[f"AP_class_{c}"]) for c in range(K.C)) or all(got[f"npos_class_{c}"] > 0 for c in range(K.C))
    m.reset()
    assert m.compute()["num_detections"] == 0


def test_one_threshold_has_no_per_threshold_keys():
    images, pred = K.split()
    m = _metric("all", "voc07", thresholds=(0.5,))
    m.update(torch.from_numpy(pred.copy()), 0)
    dets, gts, wh = K.ref_lists(images, [K.kept_records(pred[n], "all") for n in range(K.N)])
    got = m.compute()
    K.close(got, R.evaluate(dets, gts, wh, K.C, (0.5,), "voc07"))
    assert not any(k.startswith("mAP@") for k in got)


def test_the_entry_refuses_bad_arguments_without_a_device():
    """yolo_voc_match validates before any HIP call, like the other entries (tests/test_abi.py): safe without a GPU"""
    import ctypes
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    buf = (ctypes.c_double * 64)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(None)
    thr = (ctypes.c_double * 17)(*[0.5] * 17)
    call = lambda first, T, max_gt: L.yolo_voc_match(first, p, p, 3, 18, 1, p, p, p, p, p, max_gt, 0, thr, T, p, p, p, p, p, null)   # noqa: E731
    assert call(null, 1, 4) == _hip.E_ARG and b"yolo_voc_match" in L.yolo_hip_last_error()
    assert call(p, 17, 4) == _hip.E_ARG and call(p, 1, 257) == _hip.E_ARG
    assert not any(buf)


# ---------------------------------------------------------------------------------------------- a hand-built VOC tree
_OBJ = "<object><name>{name}</name>{dif}<bndbox><xmin>{b[0]}</xmin><ymin>{b[1]}</ymin><xmax>{b[2]}</xmax><ymax>{b[3]}</ymax></bndbox></object>"


def _voc_tree(root):
    from PIL import Image
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(root / d)
    objects = {
        "000001": ((140, 70), [("dog", 0, (10, 10, 50, 40)), ("dog", 0, (14, 12, 54, 44)),      # two dogs whose centres share a grid cell
                               ("cat", 1, (80, 5, 130, 60)), ("unicorn", 0, (1, 1, 20, 20)), ("person", None, (60, 30, 75, 65))]),
        "000002": ((90, 120), [("dog", 0, (5, 6, 70, 100))]),
    }
    for name, ((w, h), objs) in objects.items():
        Image.fromarray(np.full((h, w, 3), 90, np.uint8)).save(root / "JPEGImages" / f"{name}.jpg")
        body = "".join(_OBJ.format(name=n, dif="" if d is None else f"<difficult>{d}</difficult>", b=b) for n, d, b in objs)
        (root / "Annotations" / f"{name}.xml").write_text(
            f"<annotation><filename>{name}.jpg</filename><size><width>{w}</width><height>{h}</height><depth>3</depth></size>{body}</annotation>")
    (root / "ImageSets" / "Main" / "test.txt").write_text("000001\n000002\n")
    return objects


def test_ground_truth_from_the_annotations(tmp_path):
    from yolo.dataset import CombinedVOCDataset, VOCDetectionYOLO
    from yolo.voc_eval import VOCGroundTruth, VOCMetric
    _voc_tree(tmp_path)
    ds = VOCDetectionYOLO(root=tmp_path, year="2007", image_set="test", augment=False)
    g = ds.ground_truth(0)
    assert g["image_id"] == "000001" and (g["width"], g["height"]) == (140, 70)
    assert g["boxes"].dtype == np.float64 and g["class_ids"].dtype == np.int64 and g["difficult"].dtype == bool
    assert g["boxes"].tolist() == [[10, 10, 50, 40], [14, 12, 54, 44], [80, 5, 130, 60], [60, 30, 75, 65]]       # the unicorn is no VOC class
    idx = ds.class_to_idx
    assert g["class_ids"].tolist() == [idx["dog"], idx["dog"], idx["cat"], idx["person"]]
    assert g["difficult"].tolist() == [False, False, True, False]                                             # no tag: not difficult
    both = CombinedVOCDataset([ds, ds])
    assert both.ground_truth(3)["image_id"] == "000002" and both.ground_truth(3)["boxes"].tolist() == [[5, 6, 70, 100]]
    with pytest.raises(IndexError):
        both.ground_truth(4)
    # the grid target holds one dog of image 0, the annotation two
    _, target = ds[0]
    assert int((target[..., 4] > 0).sum()) == 3 and int(target[..., 10 + idx["dog"]].sum()) == 1
    gt = VOCGroundTruth.from_dataset(ds)
    assert gt.offsets.tolist() == [0, 4, 5] and gt.wh.tolist() == [[140, 70], [90, 120]] and gt.image_ids == ["000001", "000002"]
    m = VOCMetric(20, gt)
    m.update(torch.zeros(2, 7, 7, 30), 0)
    res = m.compute()
    assert res[f"npos_class_{idx['dog']}"] == 3 and res[f"npos_class_{idx['cat']}"] == 0 and res[f"npos_class_{idx['person']}"] == 1
    assert res[f"AP_class_{idx['dog']}"] == 0.0 and math.isnan(res[f"AP_class_{idx['cat']}"]) and res["mAP"] == 0.0
    # only the images that were seen count
    m.reset()
    m.update(torch.zeros(1, 7, 7, 30), 1)
    assert m.compute()[f"npos_class_{idx['dog']}"] == 1


# ---------------------------------------------------------------------------------------------- AP by hand
def _hand_case():
    """one 100 x 100 image, class 0: ground truths A, B and a difficult D; detections on A (0.9), on nothing (0.8), on D (0.7), on B (0.6)"""
    from yolo.voc_eval import VOCGroundTruth, VOCMetric
    gt = VOCGroundTruth([[10, 10, 40, 40], [60, 60, 90, 90], [10, 60, 40, 90]], [0, 0, 0], [False, False, True], [0, 3], [[100, 100]], ["img"])
    pred = np.zeros((1, 7, 7, 30), np.float32)
    for (xc, yc), conf in (((0.25, 0.25), 0.9), ((0.75, 0.25), 0.8), ((0.25, 0.75), 0.7), ((0.75, 0.75), 0.6)):
        i, j = int(7 * yc), int(7 * xc)
        pred[0, i, j, :5] = [7 * xc - j, 7 * yc - i, 0.3, 0.3, conf]
        pred[0, i, j, 10] = 1.0
    return gt, torch.from_numpy(pred), VOCMetric


@pytest.mark.parametrize("scoring", ["all", "argmax"])
def test_ap_written_out_by_hand(scoring):
    gt, pred, VOCMetric = _hand_case()
    want = {}
    # sorted: TP, FP, ignored, TP -> ctp 1 1 1 2, cfp 0 1 1 1, npos 2 -> rec .5 .5 .5 1, prec 1 .5 .5 2/3
    # voc07: t = 0 .. 0.5 see precision 1 (six points), t = 0.6 .. 1 see 2/3 (five points)
    want["voc07"] = (6 * 1.0 + 5 * (2.0 / 3.0)) / 11
    # area: the envelope is 1 up to recall 0.5 and 2/3 up to recall 1
    want["area"] = 0.5 * 1.0 + 0.5 * (2.0 / 3.0)
    for mode in ("voc07", "area"):
        m = VOCMetric(20, gt, ap_mode=mode, scoring=scoring, conf_threshold=0.1)
        m.update(pred, 0)
        res = m.compute()
        assert m._arrays()[3].tolist() == [1, 0, 2, 1]
        assert res["AP_class_0"] == pytest.approx(want[mode], abs=1e-12) and res["mAP"] == res["AP_class_0"]
        assert res["npos_class_0"] == 2 and res["num_detections"] == 4 and res["num_ignored"] == 1
        assert all(math.isnan(res[f"AP_class_{c}"]) for c in range(1, 20))


def test_write_detections_round_trip(tmp_path):
    images, pred = K.split()
    m = _metric("all", "voc07")
    m.update(torch.from_numpy(pred.copy()), 0)
    paths = m.write_detections(str(tmp_path / "det"))
    from yolo.dataset import VOC_CLASSES
    assert [os.path.basename(p) for p in paths] == [f"comp4_det_test_{n}.txt" for n in VOC_CLASSES]
    score, cls, img, _, box = m._arrays()
    total = 0
    for c, path in enumerate(paths):
        rows = [line.split(" ") for line in open(path).read().splitlines()]
        assert all(len(r) == 6 for r in rows)
        sel = np.nonzero(cls == c)[0]
        assert [r[0] for r in rows] == [m.gt.image_ids[i] for i in img[sel]]
        assert all(len(v.split(".")[1]) == 6 for r in rows for v in r[1:]), "the devkit's %f"
        got = np.array([[float(v) for v in r[1:]] for r in rows], np.float64).reshape(-1, 5)
        assert np.all(np.abs(got[:, 0] - score[sel]) <= 5.1e-7)
        assert np.all(np.abs(got[:, 1:] - (box[sel] + 1)) <= 5.1e-7), "1-based corners"
        total += len(rows)
    assert total == len(score) > 40


def test_synthetic_ground_truth_agrees_with_the_target():
    from yolo.dataset import SyntheticYOLODataset
    ds = SyntheticYOLODataset(12, S=3, B=2, C=5, max_obj=6, seed=4, size=32)
    dropped = 0
    for n in range(len(ds)):
        g = ds.ground_truth(n)
        _, target = ds[n]
        assert (g["width"], g["height"]) == (32, 32) and not g["difficult"].any() and g["boxes"].shape == (len(g["class_ids"]), 4)
        first = {}
        for b, cid in zip(g["boxes"] / 32.0, g["class_ids"]):
            xc, yc = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
            first.setdefault((min(int(3 * yc), 2), min(int(3 * xc), 2)), (xc, yc, b[2] - b[0], b[3] - b[1], int(cid)))
        filled = {(int(i), int(j)) for i, j in zip(*np.nonzero(target[..., 4].numpy() > 0))}
        assert filled == set(first)
        for (i, j), (xc, yc, w, h, cid) in first.items():
            cell = target[i, j].numpy()
            assert np.allclose(cell[:4], [3 * xc - j, 3 * yc - i, w, h], atol=1e-5) and cell[10 + cid] == 1.0 and cell[10:].sum() == 1.0
        dropped += len(g["class_ids"]) - len(first)
    assert dropped > 0, "some object shares its cell: the ground truth keeps it, the target does not"
