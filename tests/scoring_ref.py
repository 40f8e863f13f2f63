"""Class-specific scoring, the test-time protocol of the YOLOv1 paper (section 2) and of Darknet (get_detection_boxes +
do_nms_sort), restated as plain loops over Python floats.  Nothing of yolo._post_cpu is used: this file is what the CPU path
and the device path (yolo_decode_classes + grouped yolo_nms) are compared with, bit for bit.

Protocol.  For cell (i, j), box b and class c:  score = conf_b * prob_c  (fp32 values widened to double, this operand
order); a candidate is kept iff score > conf_thr; its record is [c, score, (j + x) / S, (i + y) / S, w, h].  The candidates of
a class are in (i, j, b) scan order.  Every class is NMS-filtered on its own: sort by score descending (stable: ties keep
the scan order), walk the list, a later box falls iff not (IoU(kept, later) < thr).  Two IoU variants, the project's:
INFERENCE has +1e-6 in the denominator, METRICS returns 0 for an empty union.  Per image: METRICS lists the classes
ascending, each in its NMS order; INFERENCE sorts all kept detections by score descending, stable over that list.
"""

import numpy as np

INFERENCE, METRICS = 0, 1


def decode_classes(pred, conf_thr, S, B, C):
    """pred (S,S,5B+C) fp32 -> C lists of rows [c, score, x, y, w, h] (Python floats)."""
    pred = np.asarray(pred, np.float32).reshape(S, S, 5 * B + C)
    groups = [[] for _ in range(C)]
    for c in range(C):
        for i in range(S):
            for j in range(S):
                cell = [float(v) for v in pred[i, j]]
                for b in range(B):
                    x, y, w, h, conf = cell[5 * b: 5 * b + 5]
                    score = conf * cell[5 * B + c]
                    if score > conf_thr:
                        groups[c].append([float(c), score, (float(j) + x) / float(S), (float(i) + y) / float(S), w, h])
    return groups


def iou(a, b, variant):
    """a, b = (x, y, w, h).  max / min with Python's rule (the first argument unless the second is strictly beyond it)."""
    ax1, ay1, ax2, ay2 = a[0] - a[2] / 2, a[1] - a[3] / 2, a[0] + a[2] / 2, a[1] + a[3] / 2
    bx1, by1, bx2, by2 = b[0] - b[2] / 2, b[1] - b[3] / 2, b[0] + b[2] / 2, b[1] + b[3] / 2
    ix1 = bx1 if bx1 > ax1 else ax1
    iy1 = by1 if by1 > ay1 else ay1
    ix2 = bx2 if bx2 < ax2 else ax2
    iy2 = by2 if by2 < ay2 else ay2
    dw, dh = ix2 - ix1, iy2 - iy1
    inter = (dw if dw > 0 else 0.0) * (dh if dh > 0 else 0.0)
    a1, a2 = a[2] * a[3], b[2] * b[3]
    if variant == INFERENCE:
        return inter / (a1 + a2 - inter + 1e-6)
    union = a1 + a2 - inter
    return 0.0 if union == 0 else inter / union


def nms_one_class(rows, thr, variant):
    """rows of ONE class -> kept indices into rows, in score order (ties: scan order)."""
    order = sorted(range(len(rows)), key=lambda k: -rows[k][1])          # sorted() is stable
    alive = [True] * len(order)
    kept = []
    for p, k in enumerate(order):
        if not alive[p]:
            continue
        kept.append(k)
        for q in range(p + 1, len(order)):
            if alive[q] and not (iou(rows[k][2:6], rows[order[q]][2:6], variant) < thr):
                alive[q] = False
    return kept


def image_result(groups, thr, variant):
    """-> (rec, keep, per_class_keep): rec = the groups one behind the other, keep = indices into rec in the result order of
    ``variant``, per_class_keep = the kept indices of every class into its own group."""
    rec, keep, per_class, off = [], [], [], 0
    for rows in groups:
        k = nms_one_class(rows, thr, variant)
        per_class.append(k)
        keep += [off + v for v in k]
        rec += rows
        off += len(rows)
    if variant == INFERENCE:
        keep = sorted(keep, key=lambda v: -rec[v][1])
    return rec, keep, per_class


def as_array(rows):
    return np.asarray(rows, np.float64).reshape(-1, 6)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (2, 2, 2, 3), (3, 7, 2, 20), (1, 14, 3, 20), (2, 3, 8, 2), (0, 7, 2, 20)]


def random_pred(N, S, B, C, seed=0):
    """fp32 in [0, 1) everywhere: conf, prob and the box fields"""
    rng = np.random.Generator(np.random.PCG64([seed, N, S, B, C]))
    return rng.uniform(0, 1, size=(N, S, S, 5 * B + C)).astype(np.float32)


def tied_pred(N, S, B, C, seed=1):
    """conf and prob on a grid of quarters, box fields on a grid of eighths: many exactly tied scores (zeros among them), many
    equal and many overlapping boxes, IoUs that hit round values"""
    p = random_pred(N, S, B, C, seed)
    q = np.round(p * 8) / 8
    for b in range(B):
        q[..., 5 * b + 4] = np.round(p[..., 5 * b + 4] * 4) / 4
    q[..., 5 * B:] = np.round(p[..., 5 * B:] * 4) / 4
    return q.astype(np.float32)


def overlap_pred(N, S, B, C, seed=2):
    """every cell predicts a large box around its own centre, from three widths, three heights and three confidences: the
    boxes of neighbouring cells overlap heavily -- suppression chains, score ties and equal IoUs inside a class"""
    rng = np.random.Generator(np.random.PCG64([seed, N, S, B, C]))
    p = random_pred(N, S, B, C, seed)
    for b in range(B):
        p[..., 5 * b + 0] = 0.5
        p[..., 5 * b + 1] = 0.5
        p[..., 5 * b + 2] = (0.6 + 0.1 * rng.integers(0, 3, size=p.shape[:3])).astype(np.float32)
        p[..., 5 * b + 3] = (0.5 + 0.125 * rng.integers(0, 3, size=p.shape[:3])).astype(np.float32)
        p[..., 5 * b + 4] = (0.25 * rng.integers(1, 4, size=p.shape[:3])).astype(np.float32)
    p[..., 5 * B:] = (0.25 * rng.integers(0, 4, size=p.shape[:3] + (C,))).astype(np.float32)
    return p


def one_hot_pred(N, S, B, C, seed=3):
    """class vector with exactly one positive entry per cell and zeros elsewhere"""
    rng = np.random.Generator(np.random.PCG64([seed, N, S, B, C]))
    p = random_pred(N, S, B, C, seed)
    hot = rng.integers(0, C, size=p.shape[:3])
    val = p[..., 5 * B:].max(-1) * 0.9 + 0.05
    p[..., 5 * B:] = 0.0
    np.put_along_axis(p[..., 5 * B:], hot[..., None], val[..., None], -1)
    return p


def thresholds(pred, S, B, C):
    """(name, conf_thr): below every score, above every score, equal to a score that occurs (the median of all of them)"""
    scores = sorted(r[1] for n in range(pred.shape[0]) for g in decode_classes(pred[n], -1.0, S, B, C) for r in g)
    out = [("below", -1.0), ("above", 2.0)]
    if scores:
        out.append(("equal", scores[len(scores) // 2]))
    return out
