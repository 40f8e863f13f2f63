"""Classification pretraining, the parts that need no device: tests/classify_ref.py against stock torch in fp64, the top-k hit rule, the surface of
YOLOv1Classifier / YOLOv1Backbone.load_pretrained / SoftmaxCrossEntropy on the CPU, pretrain.py and train.py --backbone-weights as subprocesses,
and the ABI surface of csrc/classify.hip."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import classify_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
E_ARG = -1


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_ref_loss_and_gradient_equal_torch_fp64(eps):
    for N, K, _eps, shift, x, y in cr.xent_cases():
        if _eps != eps:
            continue
        t = torch.from_numpy(x).double().requires_grad_(True)
        loss = F.cross_entropy(t, torch.from_numpy(y), label_smoothing=eps, reduction="mean")
        loss.backward()
        ref_l, rows, ref_d, _, flag = cr.xent(x, y, eps)
        assert flag == 0.0
        assert abs(loss.item() - ref_l) <= 1e-12 * max(1.0, abs(ref_l)), (N, K, shift, loss.item(), ref_l)
        assert np.abs(t.grad.numpy() - ref_d).max() <= 1e-12, (N, K, shift)
        assert abs(rows.sum() / N - ref_l) <= 1e-12 * max(1.0, abs(ref_l))


def test_ref_mean_equals_torch_fp64():
    rng = np.random.Generator(np.random.PCG64(5))
    for HW in (1, 49, 50, 196):
        x = rng.standard_normal((3, 8, HW)).astype(np.float32)
        ref = torch.from_numpy(x).double().view(3, 8, HW, 1).mean((2, 3)).numpy()
        assert np.abs(cr.gap(x) - ref).max() <= 1e-12
        assert (cr.gap_bound(x) > 0).all()
        dy = rng.standard_normal((3, 8)).astype(np.float32)
        dx = cr.gap_bwd(dy, HW)
        assert dx.dtype == np.float32 and dx.shape == (3, 8, HW) and np.array_equal(dx[..., 0], dy * np.float32(1.0 / HW))


def test_hit_rule_equals_topk_membership_without_ties():
    rng = np.random.Generator(np.random.PCG64(6))
    for N, K in ((16, 7), (16, 1000), (4, 5), (4, 3)):
        x = rng.permutation(N * K).reshape(N, K).astype(np.float32)          # all distinct
        y = rng.integers(0, K, N)
        top = torch.topk(torch.from_numpy(x), min(5, K), dim=1).indices.numpy()
        want = np.stack([top[:, 0] == y, (top == y[:, None]).any(1)], 1).astype(np.int32)
        assert np.array_equal(cr.hits(x, y), want), (N, K)


def test_hit_rule_with_ties_pinned_by_hand():
    x = np.array([[1, 1, 1, 1, 1, 1, 1],            # all tied: nothing is strictly greater -> both hit, whichever label
                  [3, 3, 2, 1, 0, 0, 0],            # label 1 ties with the maximum: top-1 hit
                  [9, 8, 7, 6, 6, 5, 5],            # label 5: five logits above -> no top-5; the tie with logit 6 does not matter
                  [9, 8, 7, 6, 5, 5, 5],            # label 4: four above -> top-5, not top-1
                  [2, 2, 2, 2, 2, 1, 1]],           # label 6: five above
                 dtype=np.float32)
    y = np.array([3, 1, 5, 4, 6])
    assert cr.hits(x, y).tolist() == [[1, 1], [1, 1], [0, 0], [0, 1], [0, 0]]
    assert cr.hits(np.array([[0.5, -1.0, 2.0]], dtype=np.float32), np.array([1])).tolist() == [[0, 1]]      # K < 5: top-5 always hits a valid label
    assert cr.hits(np.array([[0.5, -1.0, 2.0]], dtype=np.float32), np.array([3])).tolist() == [[0, 0]]      # a label outside [0, K) never does
    from yolo.classify import topk_hits
    assert topk_hits(torch.from_numpy(x), torch.from_numpy(y)).tolist() == cr.hits(x, y).tolist()


def test_ref_invalid_labels_contribute_nothing():
    x, y = cr.xent_case(5, 7, 0)
    y2 = y.copy()
    y2[1], y2[3] = -1, 7
    mean, rows, d, h, flag = cr.xent(x, y2, 0.1)
    mean0, rows0, d0, h0, _ = cr.xent(x, y, 0.1)
    assert flag == 1.0 and rows[1] == rows[3] == 0.0 and not d[1].any() and not d[3].any() and not h[1].any() and not h[3].any()
    assert np.array_equal(rows[[0, 2, 4]], rows0[[0, 2, 4]]) and np.array_equal(d[[0, 2, 4]], d0[[0, 2, 4]])
    assert abs(mean - rows0[[0, 2, 4]].sum() / 5) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------------------------
# module surface
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def classifier():
    from yolo import YOLOv1Classifier
    torch.manual_seed(0)
    return YOLOv1Classifier(num_classes=6)


def test_classifier_surface(classifier):
    from yolo import YOLOv1Backbone, YOLOv1Classifier, GlobalAvgPool, SoftmaxCrossEntropy  # noqa: F401  (exported)
    m = classifier.eval()
    with torch.no_grad():
        y = m(torch.randn(2, 3, 64, 64))
    assert y.shape == (2, 6)
    convs = [mod for mod in m.features if isinstance(mod, nn.Conv2d)]
    assert len(convs) == 20 and isinstance(m.features[-1], nn.LeakyReLU) and isinstance(m.features[-2], nn.Conv2d)
    assert isinstance(m.pool, GlobalAvgPool) and isinstance(m.fc, nn.Linear) and (m.fc.in_features, m.fc.out_features) == (1024, 6)
    bb = YOLOv1Backbone().state_dict()
    sd = m.state_dict()
    feat = {k: v for k, v in sd.items() if k.startswith("features.")}
    assert len(feat) == 40 and set(sd) == set(feat) | {"fc.weight", "fc.bias"}
    for k, v in feat.items():
        assert k in bb and bb[k].shape == v.shape, k
    assert sum(isinstance(mod, nn.Conv2d) for mod in YOLOv1Backbone().features) == 24
    assert YOLOv1Classifier().fc.out_features == 1000
    p = GlobalAvgPool()(torch.randn(2, 5, 3, 4))
    assert p.shape == (2, 5, 1, 1)


def test_load_pretrained_round_trip(classifier):
    from yolo import YOLOv1Backbone
    torch.manual_seed(1)
    bb = YOLOv1Backbone()
    before = {k: v.clone() for k, v in bb.state_dict().items()}
    sd = classifier.state_dict()
    assert bb.load_pretrained(sd) == 40
    after = bb.state_dict()
    for k, v in after.items():
        if k in sd:
            assert torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr(), k
        else:
            assert torch.equal(v, before[k]), f"{k} is not part of the checkpoint and must stay as initialised"
    assert sum(k not in sd for k in after) == 8          # the four convolutions detection adds
    bad = dict(sd)
    bad["features.3.weight"] = torch.zeros(192, 64, 5, 5)
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        bb.load_pretrained(bad)
    assert torch.equal(bb.state_dict()["features.0.weight"], sd["features.0.weight"])
    with pytest.raises(KeyError, match=r"features\.99\.weight"):
        bb.load_pretrained({"features.99.weight": torch.zeros(1)})


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_softmax_cross_entropy_on_the_cpu(eps):
    from yolo import SoftmaxCrossEntropy
    x, y = cr.xent_case(5, 7, 0)
    crit = SoftmaxCrossEntropy(label_smoothing=eps)
    a = torch.from_numpy(x).clone().requires_grad_(True)
    b = torch.from_numpy(x).clone().requires_grad_(True)
    loss, parts = crit(a, torch.from_numpy(y))
    loss.backward()
    ref = F.cross_entropy(b, torch.from_numpy(y), label_smoothing=eps)
    ref.backward()
    assert torch.equal(loss.detach(), ref.detach()) and torch.equal(a.grad, b.grad)
    h = cr.hits(x, y)
    assert set(parts.keys()) == {"total", "top1", "top5"}
    assert parts["total"] == pytest.approx(ref.item(), rel=1e-6) and parts["top1"] == h[:, 0].mean() and parts["top5"] == h[:, 1].mean()
    assert float(parts.device_flag) == 0.0
    # a label outside [0, K): the flag, no contribution, and the error at the first read
    y2 = y.copy()
    y2[2] = 7
    c = torch.from_numpy(x).clone().requires_grad_(True)
    loss2, parts2 = crit(c, torch.from_numpy(y2))
    loss2.backward()
    mean, _, d, _, flag = cr.xent(x, y2, eps)
    assert flag == 1.0 and float(parts2.device_flag) == 1.0
    assert abs(loss2.item() - mean) <= 1e-5 * max(1.0, abs(mean)) and np.abs(c.grad.numpy() - d).max() <= 1e-6 and not c.grad[2].any()
    with pytest.raises(RuntimeError, match="label out of bounds"):
        parts2["total"]
    with pytest.raises(ValueError):
        SoftmaxCrossEntropy(label_smoothing=1.0)


def test_datasets(tmp_path):
    from PIL import Image
    from yolo.dataset import ImageFolderClassification, SyntheticClassificationDataset
    rng = np.random.Generator(np.random.PCG64(3))
    for split, per in (("train", 3), ("val", 1)):
        for cls in ("zebra", "ant"):
            d = tmp_path / split / cls
            d.mkdir(parents=True)
            for i in range(per):
                Image.fromarray(rng.integers(0, 255, (40 + i, 50, 3), dtype=np.uint8).astype(np.uint8), "RGB").save(d / f"{i}.png")
            (d / "notes.txt").write_text("not an image")
    tr = ImageFolderClassification(tmp_path, "train", 64)
    va = ImageFolderClassification(tmp_path, "val", 64, classes=tr.classes)
    assert tr.classes == ["ant", "zebra"] and len(tr) == 6 and len(va) == 2 and tr.transform.train and not va.transform.train
    x, y = tr[5]
    assert x.shape == (3, 64, 64) and x.dtype == torch.float32 and y == 1
    xa, _ = va[0]
    xb, _ = va[0]
    assert torch.equal(xa, xb), "the validation transform draws nothing"
    with pytest.raises(FileNotFoundError):
        ImageFolderClassification(tmp_path, "test", 64)
    with pytest.raises(ValueError, match="zebra"):
        ImageFolderClassification(tmp_path, "val", 64, classes=["ant"])
    s = SyntheticClassificationDataset(8, 4, 64, seed=0)
    assert len(s) == 8 and [s[i][1] for i in range(8)] == [0, 1, 2, 3, 0, 1, 2, 3] and s[1][0].shape == (3, 64, 64)
    assert torch.equal(s[2][0], s[2][0]) and not torch.equal(s[2][0], s[6][0])


# ---------------------------------------------------------------------------------------------------------------------------------
# the command-line tools
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(args, timeout=600):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def test_pretrain_then_train_from_its_checkpoint(tmp_path):
    ck = tmp_path / "pre"
    _run([os.path.join(PKG, "pretrain.py"), "--device", "cpu", "--synthetic", "8", "--num-classes", "4", "--image-size", "64", "--epochs", "1",
          "--batch-size", "8", "--num-workers", "0", "--checkpoint-dir", str(ck)])
    assert (ck / "yolo_latest.pth").is_file() and (ck / "yolo_best_top1.pth").is_file()
    data = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    for key in ("epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "train_loss", "val_loss"):      # the reference's keys
        assert key in data, key
    assert data["num_classes"] == 4 and data["image_size"] == 64 and data["epoch"] == 1
    assert data["model_state_dict"]["fc.weight"].shape == (4, 1024) and "features.0.weight" in data["model_state_dict"]
    r = _run([os.path.join(PKG, "train.py"), "--backbone", "yolov1", "--backbone-weights", str(ck / "yolo_latest.pth"), "--synthetic", "4", "--epochs", "1",
              "--device", "cpu", "--batch-size", "4", "--num-workers", "0", "--checkpoint-dir", str(tmp_path / "det")])
    assert re.search(r"backbone: loaded 40 tensors", r.stdout), r.stdout[-2000:]
    det = torch.load(tmp_path / "det" / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert "backbone.features.0.weight" in det["model_state_dict"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_classify_entry_is_declared_bound_and_called_by_the_gpu_test():
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "classify.hip")) as f:
        src = f.read()
    entries = set(re.findall(r"YOLO_API int (yolo_\w+)", src))
    assert entries == {"yolo_gap_fwd", "yolo_gap_bwd", "yolo_softmax_xent_fwd_bwd"}
    assert "atomic" not in src.lower().replace("no atomics", ""), "no atomics: two runs are bit-equal"
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_classify.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header) and _hip.ABI_VERSION == 2
    with open(os.path.join(PKG, "csrc", "Makefile")) as f:
        assert "classify.hip" in f.read()


def test_classify_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call, so they can be exercised without a device; the pointers are never dereferenced"""
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    p = 4096          # a non-null address that is never read
    for fn in (L.yolo_gap_fwd, L.yolo_gap_bwd):
        assert fn(None, 1, 8, 49, p, None) == E_ARG and fn(p, 1, 8, 49, None, None) == E_ARG
        assert fn(p, -1, 8, 49, p, None) == E_ARG and fn(p, 1, 0, 49, p, None) == E_ARG and fn(p, 1, 8, 0, p, None) == E_ARG
        assert fn(p, 0, 8, 49, p, None) == 0, "an empty batch launches nothing"
    x = L.yolo_softmax_xent_fwd_bwd
    good = dict(logits=p, labels=p, N=2, K=5, eps=0.1, out=p, dlogits=p, hits=p, work=p)

    def call(**kw):
        a = {**good, **kw}
        return x(a["logits"], a["labels"], a["N"], a["K"], a["eps"], a["out"], a["dlogits"], a["hits"], a["work"], None)
    for name in ("logits", "labels", "out", "hits", "work"):
        assert call(**{name: None}) == E_ARG, name
    assert call(N=-1) == E_ARG and call(K=0) == E_ARG
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        assert call(eps=eps) == E_ARG, eps
    assert b"label_smoothing" in L.yolo_hip_last_error()
