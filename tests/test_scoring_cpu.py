"""CPU: class-specific scoring (scoring="all", the YOLOv1 paper's test-time protocol) on the host path -- yolo._post_cpu,
mAPMetric, YOLOInference and the two command lines -- against tests/scoring_ref.py, bit for bit."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scoring_ref as R
from yolo import _post_cpu as P
from yolo import mAPMetric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NMS_THR = 0.4
KINDS = {"random": R.random_pred, "tied": R.tied_pred, "overlap": R.overlap_pred}


@functools.lru_cache(maxsize=None)
def _pred(shape, kind):
    p = KINDS[kind](*shape)
    p.setflags(write=False)
    return p


def _cases():
    for shape in R.SHAPES:
        for kind in KINDS:
            yield pytest.param(shape, kind, id=f"{'x'.join(map(str, shape))}-{kind}")


@pytest.mark.parametrize("shape,kind", list(_cases()))
def test_decode_and_both_results_equal_the_restated_protocol(shape, kind):
    N, S, B, C = shape
    pred = _pred(shape, kind)
    big = S * S * B > 128
    for name, thr in R.thresholds(pred, S, B, C):
        for n in range(N):
            ref = R.decode_classes(pred[n], thr, S, B, C)
            got = P.decode_classes(pred[n], thr, S, B)
            assert len(got) == C
            for c in range(C):
                assert got[c].dtype == np.float64 and np.array_equal(got[c], R.as_array(ref[c])), (name, n, c)
            if name == "below":
                assert all(len(g) == S * S * B for g in got)
            elif name == "above":
                assert all(len(g) == 0 for g in got)
            else:
                assert not any(thr in g[:, 1] for g in got), "a score equal to the threshold is dropped"
            if big and name == "below":
                continue            # 20 full lists of 588 through the pure-Python NMS: the "equal" threshold keeps half of them
            for variant in (P.INFERENCE, P.METRICS):
                rrec, rkeep, _ = R.image_result(ref, NMS_THR, variant)
                rec, keep = P.nms_classes(got, NMS_THR, variant)
                assert np.array_equal(rec, R.as_array(rrec)), (name, n, variant)
                assert keep.tolist() == rkeep, (name, n, variant)


def test_the_tied_and_overlap_cases_are_what_they_claim():
    shape = (3, 7, 2, 20)
    groups = R.decode_classes(_pred(shape, "tied")[0], -1.0, 7, 2, 20)
    scores = [r[1] for g in groups for r in g]
    assert len(set(scores)) < len(scores) // 20, "many exactly tied scores"
    groups = R.decode_classes(_pred(shape, "overlap")[0], 0.1, 7, 2, 20)
    kept = sum(len(k) for k in R.image_result(groups, NMS_THR, R.METRICS)[2])
    assert 0 < kept < sum(len(g) for g in groups) // 2, "NMS has work to do"


@pytest.mark.parametrize("kind", ["random", "tied"])
def test_every_argmax_record_is_in_the_group_of_its_class(kind):
    shape = (3, 7, 2, 20)
    pred = _pred(shape, kind)
    for thr in (-1.0, 0.0, 0.2):
        for n in range(3):
            groups = P.decode_classes(pred[n], thr, 7, 2)
            for row in P.decode(pred[n], thr, 7, 2):
                g = groups[int(row[0])]
                assert np.any(np.all(g == row, axis=1)), (thr, n, row)


@pytest.mark.parametrize("conf_thr", [0.0, 0.2])
def test_one_hot_class_vectors_give_the_argmax_detections(conf_thr):
    """exactly one positive class per cell: every other class scores conf * 0 = 0, which no threshold >= 0 keeps"""
    S, B, C = 7, 2, 20
    pred = R.one_hot_pred(3, S, B, C)
    for n in range(3):
        arg = P.decode(pred[n], conf_thr, S, B)
        rec, keep = P.nms_classes(P.decode_classes(pred[n], conf_thr, S, B), NMS_THR, P.INFERENCE)
        assert np.array_equal(rec[keep], arg[P.nms(arg, NMS_THR, P.INFERENCE)])
        # metrics variant: argmax groups the classes in first-appearance order, "all" lists them ascending -- same set, and inside
        # every class the same order
        rec, keep = P.nms_classes(P.decode_classes(pred[n], conf_thr, S, B), NMS_THR, P.METRICS)
        want = arg[P.nms(arg, NMS_THR, P.METRICS)]
        assert len(keep) == len(want)
        for c in range(C):
            assert np.array_equal(rec[keep][rec[keep, 0] == c], want[want[:, 0] == c])


def test_one_hot_through_the_inference_engine():
    """YOLOInference on CPU tensors: predict(scoring="all") returns the detections of the default, in the same order"""
    from PIL import Image
    from yolo.inference import YOLOInference

    class Fixed(torch.nn.Module):
        S, B = 7, 2

        def __init__(self, pred):
            super().__init__()
            self.pred = pred

        def forward(self, x):
            return self.pred

    pred = torch.from_numpy(R.one_hot_pred(1, 7, 2, 20))
    eng = YOLOInference(Fixed(pred), device="cpu")
    eng.load_image = lambda path: Image.new("RGB", (32, 32))
    a = eng.predict("x.jpg", conf_threshold=0.1, nms_threshold=NMS_THR)
    b = eng.predict("x.jpg", conf_threshold=0.1, nms_threshold=NMS_THR, scoring="all")
    assert len(a) > 3 and a == b
    assert eng.parse_predictions(pred[0], 0.1, scoring="all") == sorted(eng.parse_predictions(pred[0], 0.1), key=lambda d: d.class_id)
    with pytest.raises(ValueError):
        eng.predict("x.jpg", scoring="x")
    with pytest.raises(ValueError):
        eng.parse_predictions(pred[0], 0.1, scoring="x")


def _map_case():
    d = np.load(os.path.join(GOLDEN, "map_case.npz"))
    return d["pred"], d["tgt"]


def reference_shaped_metric(pred, tgt, conf_thr, nms_thr):
    """the host machinery of mAPMetric (the reference's protocol restated) on lists filled by hand from scoring_ref"""
    m = mAPMetric(20, conf_threshold=conf_thr, nms_threshold=nms_thr)
    for n in range(pred.shape[0]):
        rec, keep, _ = R.image_result(R.decode_classes(pred[n], conf_thr, 7, 2, 20), nms_thr, R.METRICS)
        m.all_predictions.append([(int(rec[k][0]), rec[k][1], tuple(rec[k][2:6])) for k in keep])
        m.all_ground_truths.append(m._parse_ground_truth(torch.from_numpy(tgt[n])))
    return m.compute()


def test_metric_on_cpu_tensors_equals_the_host_machinery_on_the_restated_lists():
    pred, tgt = _map_case()
    m = mAPMetric(20, conf_threshold=0.05, nms_threshold=0.4, scoring="all")
    m.update(torch.from_numpy(pred), torch.from_numpy(tgt))
    res = m.compute()
    want = reference_shaped_metric(pred, tgt, 0.05, 0.4)
    assert set(res) == set(want) and len(res) > 70
    for k, v in want.items():
        assert float(res[k]) == pytest.approx(float(v), abs=1e-12), k
    assert sum(len(p) for p in m.all_predictions) > 2 * 16 * 20, "far more candidates than one class per cell gives"


def test_default_scoring_is_unchanged_against_the_recorded_values():
    pred, tgt = _map_case()
    ref = json.load(open(os.path.join(GOLDEN, "map_case.json")))
    for m in (mAPMetric(20, conf_threshold=0.05, nms_threshold=0.4), mAPMetric(20, None, 0.05, 0.4, 7, 2, "argmax")):
        assert m.scoring == "argmax"
        m.update(torch.from_numpy(pred), torch.from_numpy(tgt))
        res = m.compute()
        assert set(res) == set(ref)
        for k, v in ref.items():
            assert float(res[k]) == pytest.approx(v, abs=1e-12), k


def test_keyword_is_last_and_defaults_to_argmax():
    import inspect
    from yolo import evaluate_model
    from yolo.inference import YOLOInference
    from yolo import ops
    for fn in (mAPMetric.__init__, evaluate_model, YOLOInference.predict, YOLOInference.parse_predictions, ops.postprocess_host):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "scoring" and last.default == "argmax", fn


def test_unknown_scoring_value_raises():
    with pytest.raises(ValueError):
        mAPMetric(20, scoring="x")
    with pytest.raises(ValueError):
        from yolo import evaluate_model
        evaluate_model(torch.nn.Identity(), [], "cpu", scoring="x")


@pytest.mark.parametrize("script", ["evaluate.py", "predict.py"])
def test_command_line_refuses_an_unknown_scoring(script, tmp_path):
    """argparse exits with status 2 while parsing: no checkpoint is read, no model built, no output written"""
    args = [sys.executable, os.path.join(PKG, script), "--scoring", "bogus", "--device", "cpu"]
    args += ["--output", str(tmp_path / "out.txt")] if script == "evaluate.py" else ["nonexistent.jpg"]
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--scoring" in r.stderr and "bogus" in r.stderr
    assert not list(tmp_path.iterdir())
