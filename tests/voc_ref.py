"""The PASCAL VOC devkit's detection evaluation, restated plainly in Python floats (fp64): detection by detection, ground truth by
ground truth, nothing shared with yolo/voc_eval.py or yolo/_post_cpu.py.  The reference of tests/test_voc_eval_cpu.py and
tests/test_gpu_voc_eval.py.

A detection is (image, class, score, x, y, w, h) with a normalised centre box; a ground truth is (image, class, difficult, xmin, ymin,
xmax, ymax) in pixels; ``wh[image] = (W, H)``.  Detections come in image order, then list order.
"""

import math

FP, TP, IGNORED = 0, 1, 2
EPS = 5e-324          # the smallest positive fp64


def clamp(v, hi):
    if v < 0:
        v = 0.0
    if v > hi:
        v = hi
    return v


def pixel_box(x, y, w, h, W, H):
    W, H = float(W), float(H)
    x1 = (x - w / 2) * W
    y1 = (y - h / 2) * H
    x2 = (x + w / 2) * W
    y2 = (y + h / 2) * H
    return clamp(x1, W), clamp(y1, H), clamp(x2, W), clamp(y2, H)


def lesser(a, b):
    return b if b < a else a


def greater(a, b):
    return b if b > a else a


def overlap(box, g):
    """devkit overlap of a pixel box and a ground-truth box, or None where it does not take part"""
    x1, y1, x2, y2 = box
    gx1, gy1, gx2, gy2 = g
    iw = lesser(x2, gx2) - greater(x1, gx1) + 1
    ih = lesser(y2, gy2) - greater(y1, gy1) + 1
    if iw > 0 and ih > 0:
        ua = (x2 - x1 + 1) * (y2 - y1 + 1) + (gx2 - gx1 + 1) * (gy2 - gy1 + 1) - iw * ih
        return iw * ih / ua
    return None


def match(dets, gts, wh, thresholds):
    """-> (status words, pixel boxes), one per detection in the order of ``dets``; 2 bits per threshold"""
    boxes = [pixel_box(d[3], d[4], d[5], d[6], *wh[d[0]]) for d in dets]
    status = [0] * len(dets)
    classes = sorted({d[1] for d in dets})
    for c in classes:
        idx = [k for k, d in enumerate(dets) if d[1] == c]
        idx.sort(key=lambda k: -dets[k][2])                     # stable: ties keep image order, then list order
        for t, thr in enumerate(thresholds):
            taken = set()
            for k in idx:
                ovmax, jmax = -math.inf, None
                for j, g in enumerate(gts):
                    if g[0] != dets[k][0] or g[1] != c:
                        continue
                    ov = overlap(boxes[k], g[3:7])
                    if ov is not None and ov > ovmax:
                        ovmax, jmax = ov, j
                st = FP
                if jmax is not None and ovmax >= thr:
                    if gts[jmax][2]:
                        st = IGNORED
                    elif jmax not in taken:
                        st = TP
                        taken.add(jmax)
                status[k] |= st << (2 * t)
    return status, boxes


def ap_voc07(rec, prec):
    ap = 0.0
    for k in range(11):
        t = k * 0.1                                             # np.arange(0, 1.1, 0.1) of the devkit
        p = 0.0
        for r, q in zip(rec, prec):
            if r >= t and q > p:
                p = q
        ap = ap + p / 11.0
    return ap


def ap_area(rec, prec):
    mrec = [0.0] + list(rec) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        if mpre[i + 1] > mpre[i]:
            mpre[i] = mpre[i + 1]
    ap = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            ap += (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return ap


def evaluate(dets, gts, wh, num_classes, thresholds, ap_mode):
    """-> the result dictionary of VOCMetric.compute()"""
    status, _ = match(dets, gts, wh, thresholds)
    npos = [sum(1 for g in gts if g[1] == c and not g[2]) for c in range(num_classes)]
    per_thr = []
    for t in range(len(thresholds)):
        aps = []
        for c in range(num_classes):
            if npos[c] == 0:
                aps.append(math.nan)
                continue
            idx = [k for k, d in enumerate(dets) if d[1] == c]
            idx.sort(key=lambda k: -dets[k][2])
            ctp = cfp = 0.0
            rec, prec = [], []
            for k in idx:
                st = (status[k] >> (2 * t)) & 3
                ctp += st == TP
                cfp += st == FP
                rec.append(ctp / npos[c])
                prec.append(ctp / max(ctp + cfp, EPS))
            aps.append(ap_voc07(rec, prec) if ap_mode == "voc07" else ap_area(rec, prec))
        per_thr.append(aps)

    def mean(aps):
        v = [a for a in aps if not math.isnan(a)]
        return sum(v) / len(v) if v else math.nan

    out = {"mAP": mean(per_thr[0])}
    if len(thresholds) > 1:
        for thr, aps in zip(thresholds, per_thr):
            out["mAP@%g" % thr] = mean(aps)
    for c in range(num_classes):
        out["AP_class_%d" % c] = per_thr[0][c]
        out["npos_class_%d" % c] = npos[c]
    out["num_detections"] = len(dets)
    out["num_ignored"] = sum(1 for s in status if (s & 3) == IGNORED)
    return out
