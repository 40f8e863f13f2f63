"""Inputs shared by tests/test_voc_eval_cpu.py and tests/test_gpu_voc_eval.py: a small synthetic split with cell collisions and
hand-set difficult flags, network-like predictions for it, and the conversion of kept records into the lists tests/voc_ref.py takes."""

import functools

import numpy as np

S, B, C, N = 7, 2, 20, 5
CONF_THR, NMS_THR = 0.05, 0.4
THRESHOLDS = (0.5, 0.3, 0.75)


@functools.lru_cache(maxsize=None)
def split():
    """(ground_truth dicts of N images, predictions (N,S,S,5B+C) float32, read-only).  Image sizes differ and W != H; every third object
    is difficult; the predictions put one box on every object -- slot 0 for the first object of a cell, slot 1 for the second -- over noise."""
    from yolo.dataset import SyntheticYOLODataset
    ds = SyntheticYOLODataset(N, S=S, B=B, C=C, max_obj=7, seed=11, size=64)
    rng = np.random.Generator(np.random.PCG64(3))
    images, n_obj = [], 0
    pred = rng.uniform(0.0, 0.3, size=(N, S, S, 5 * B + C)).astype(np.float32)
    for n in range(N):
        g = ds.ground_truth(n)
        W, H = 500 - 40 * n, 333 + 25 * n
        g["boxes"] = g["boxes"] / 64.0 * np.array([W, H, W, H], np.float64)          # the same normalised boxes on a W x H image
        g["width"], g["height"] = W, H
        g["difficult"] = np.array([(n_obj + k) % 3 == 2 for k in range(len(g["class_ids"]))], bool)
        n_obj += len(g["class_ids"])
        filled = {}
        for (x1, y1, x2, y2), cid in zip(g["boxes"], g["class_ids"]):
            xc, yc, w, h = (x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H
            i, j = min(int(S * yc), S - 1), min(int(S * xc), S - 1)
            b = filled.get((i, j), 0)
            filled[(i, j)] = b + 1
            if b >= B:
                continue
            noise = rng.normal(0, 0.02, 4)
            pred[n, i, j, 5 * b: 5 * b + 5] = [S * xc - j + noise[0], S * yc - i + noise[1], w + noise[2], h + noise[3], 0.6 + 0.3 * rng.uniform()]
            pred[n, i, j, 5 * B + cid] = 0.7 + 0.05 * b
        images.append(g)
    pred.setflags(write=False)
    return tuple(images), pred


def kept_records(pred_img, scoring):
    """the kept records of one image in metrics-NMS order, by the host decode and NMS the project already has"""
    from yolo import _post_cpu
    if scoring == "all":
        rec, keep = _post_cpu.nms_classes(_post_cpu.decode_classes(pred_img, CONF_THR, S, B), NMS_THR, _post_cpu.METRICS)
    else:
        rec = _post_cpu.decode(pred_img, CONF_THR, S, B)
        keep = _post_cpu.nms(rec, NMS_THR, _post_cpu.METRICS)
    return rec[keep]


def ref_lists(images, kept_per_image):
    """-> (dets, gts, wh) as tests/voc_ref.py takes them"""
    dets = [(n, int(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5])) for n, k in enumerate(kept_per_image) for r in k]
    gts = [(n, int(c), bool(d), *map(float, b)) for n, g in enumerate(images) for b, c, d in zip(g["boxes"], g["class_ids"], g["difficult"])]
    wh = [(g["width"], g["height"]) for g in images]
    return dets, gts, wh


def close(got, want, tol=1e-12):
    """metric keys: equal to ``tol``, nan where the reference has nan"""
    assert set(got) == set(want), set(got) ^ set(want)
    for k, v in want.items():
        if isinstance(v, float) and np.isnan(v):
            assert np.isnan(got[k]), k
        else:
            assert abs(float(got[k]) - float(v)) <= tol, (k, got[k], v)
