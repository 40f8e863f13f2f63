"""What yolo_detect_finish computes (include/yolo_hip.h), restated in plain Python floats and lists: no NumPy arithmetic, nothing
shared with yolo/ops.py or yolo/_post_cpu.py.  Python floats are IEEE doubles and every operation below rounds once, so the
expected rows are exact: the tests compare bit patterns."""

import struct


def _lists(a):
    return a.tolist() if hasattr(a, "tolist") else a


def pixel_corners(x, y, w, h, W, H):
    """normalised centre box -> pixel corners of a W x H image, clamped to it"""
    W, H = float(W), float(H)
    out = [(x - w / 2) * W, (y - h / 2) * H, (x + w / 2) * W, (y + h / 2) * H]
    for i, lim in enumerate((W, H, W, H)):
        if out[i] < 0:
            out[i] = 0.0
        if out[i] > lim:
            out[i] = lim
    return out


def detect_finish(rec, keep, kc, groups_per_image, img_wh=None):
    """rec [n_groups][M][6], keep [n_groups][M], kc [n_groups] as yolo_nms (inference variant) takes and leaves them ->
    (det: rows of 6 floats, image: one index per row, off: images + 1 row offsets)"""
    rec, keep, kc = _lists(rec), _lists(keep), _lists(kc)
    img_wh = None if img_wh is None else _lists(img_wh)
    assert len(rec) == len(keep) == len(kc) and len(rec) % groups_per_image == 0
    det, image, off = [], [], [0]
    for n in range(len(rec) // groups_per_image):
        rows = []
        for g in range(n * groups_per_image, (n + 1) * groups_per_image):
            rows += [rec[g][keep[g][k]] for k in range(kc[g])]
        if groups_per_image > 1:
            rows = [rows[i] for i in sorted(range(len(rows)), key=lambda i: -rows[i][1])]      # sorted() is stable
        for c, s, x, y, w, h in rows:
            det.append([c, s] + (pixel_corners(x, y, w, h, *img_wh[n]) if img_wh is not None else [x, y, w, h]))
            image.append(n)
        off.append(len(det))
    return det, image, off


def bits(rows):
    """the bit patterns of a table of doubles: equal floats that differ in a bit (0.0 / -0.0) or NaNs do not pass for equal"""
    return [[struct.unpack("<q", struct.pack("<d", v))[0] for v in row] for row in rows]
