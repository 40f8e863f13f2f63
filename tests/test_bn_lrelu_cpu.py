"""BatchNorm variant of the YOLOv1 network, the parts that need no device: tests/bn_lrelu_ref.py against stock torch in fp64, the surface of
YOLOv1Backbone / YOLOv1Classifier with batch_norm=True, the eval-mode fold, the ABI surface of the two new entries of csrc/bn.hip, and the command lines."""

import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_lrelu_ref as br
import launch_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
E_ARG, E_UNSUPPORTED = -1, -2
ENTRIES = {"yolo_batchnorm_train_fwd_lrelu", "yolo_batchnorm_bwd_lrelu"}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the fp64 reference against stock torch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [False, True])
def test_reference_equals_torch_fp64(pool):
    N, H, W, C = 2, 6, 10, 64
    g = torch.Generator().manual_seed(3)
    z = torch.randn(N, H, W, C, dtype=torch.float64, generator=g) * 1.5 + 0.3
    gamma = torch.rand(C, dtype=torch.float64, generator=g) + 0.5
    beta = torch.randn(C, dtype=torch.float64, generator=g) * 0.5
    zc = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gc, bc = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yc = F.leaky_relu(F.batch_norm(zc, None, None, gc, bc, True, 0.1, 1e-5), 0.1)
    if pool:
        w = br.windows(yc.detach().permute(0, 2, 3, 1))
        top2 = w.topk(2, dim=3).values
        assert bool((top2[:, :, :, 0] > top2[:, :, :, 1]).all()), "the random inputs have no exact tie inside a window"
        yc = F.max_pool2d(yc, 2)
    dy = torch.randn(yc.shape, dtype=torch.float64, generator=g)
    yc.backward(dy)

    zz = z.reshape(-1, C)
    mean, var, dm, dv = lr.bn_stats_ref(zz, 1)
    R = br.fwd_ref(z, mean, var, dm, dv, gamma, beta, 1e-5, 0.1, pool=pool)
    assert _rel(R.y, yc.detach().permute(0, 2, 3, 1)) <= 1e-12
    assert bool((R.bnd > 0).all())
    B = br.bwd_ref(dy.permute(0, 2, 3, 1), z, gamma, R.save, 1, 0.1, R.mask, R.sel)
    assert _rel(B.dz, zc.grad.permute(0, 2, 3, 1)) <= 1e-12
    assert _rel(B.dgamma, gc.grad) <= 1e-12 and _rel(B.dbeta, bc.grad) <= 1e-12
    assert bool((B.bnd > 0).all()) and bool((B.dgamma_bnd > 0).all()) and bool((B.dbeta_bnd > 0).all())
    # frozen: running statistics, no batch terms
    rm, rv = torch.randn(C, dtype=torch.float64, generator=g) * 0.3, torch.rand(C, dtype=torch.float64, generator=g) + 0.5
    zc.grad = None
    gc.grad, bc.grad = None, None
    yf = F.leaky_relu(F.batch_norm(zc, rm, rv, gc, bc, False, 0.1, 1e-5), 0.1)
    yf = F.max_pool2d(yf, 2) if pool else yf
    yf.backward(dy)
    zero = torch.zeros_like(rm)
    Rf = br.fwd_ref(z, rm, rv, zero, zero, gamma, beta, 1e-5, 0.1, pool=pool)
    Bf = br.bwd_ref(dy.permute(0, 2, 3, 1), z, gamma, Rf.save, 1, 0.1, Rf.mask, Rf.sel, frozen=True)
    assert _rel(Rf.y, yf.detach().permute(0, 2, 3, 1)) <= 1e-12 and _rel(Bf.dz, zc.grad.permute(0, 2, 3, 1)) <= 1e-12
    assert _rel(Bf.dgamma, gc.grad) <= 1e-12 and _rel(Bf.dbeta, bc.grad) <= 1e-12


def test_reference_gives_a_tied_window_to_the_first_position_in_scan_order():
    y = torch.tensor([[1.0, 3.0, 0.0, 0.0],
                      [3.0, 3.0, 0.0, 0.0]], dtype=torch.float64).view(1, 2, 4, 1)       # window 0: 3 at (0,1), (1,0), (1,1); window 1: all equal
    sel = br.first_argmax(y)
    assert sel.view(-1).tolist() == [1, 0]
    yc = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(yc, 2).backward(torch.tensor([5.0, 7.0], dtype=torch.float64).view(1, 1, 1, 2))
    got = br.scatter(torch.tensor([5.0, 7.0], dtype=torch.float64).view(1, 1, 2, 1), sel)
    assert torch.equal(got, yc.grad.permute(0, 2, 3, 1))          # aten's rule
    assert torch.equal(br.select(y, sel).view(-1), torch.tensor([3.0, 0.0], dtype=torch.float64))
    assert torch.equal(br.unwindows(br.windows(y)), y)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_construction_is_unchanged():
    from yolo import YOLOv1Backbone, YOLOv1Classifier
    torch.manual_seed(0)
    a = YOLOv1Backbone().state_dict()
    end_a = torch.rand(1)
    torch.manual_seed(0)
    b = YOLOv1Backbone(batch_norm=False).state_dict()
    end_b = torch.rand(1)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and torch.equal(end_a, end_b)
    convs = [m for m in YOLOv1Backbone().features if isinstance(m, nn.Conv2d)]
    assert len(convs) == 24 and all(c.bias is not None for c in convs)
    assert not any(isinstance(m, nn.BatchNorm2d) for m in YOLOv1Backbone().features)
    torch.manual_seed(0)
    c = YOLOv1Classifier(7).state_dict()
    torch.manual_seed(0)
    d = YOLOv1Classifier(7, batch_norm=False).state_dict()
    assert list(c) == list(d) and all(torch.equal(c[k], d[k]) for k in c) and len([k for k in c if k.startswith("features.")]) == 40


def test_batch_norm_surface_and_load_pretrained():
    from yolo import YOLOv1, YOLOv1Backbone, YOLOv1Classifier
    from yolo.models import init_kaiming_
    bb = YOLOv1Backbone(batch_norm=True)
    mods = list(bb.features)
    convs = [m for m in mods if isinstance(m, nn.Conv2d)]
    assert len(convs) == 24 and all(c.bias is None for c in convs) and sum(isinstance(m, nn.BatchNorm2d) for m in mods) == 24
    assert sum(isinstance(m, nn.MaxPool2d) for m in mods) == 4
    for i, m in enumerate(mods):
        if isinstance(m, nn.Conv2d):
            assert isinstance(mods[i + 1], nn.BatchNorm2d) and mods[i + 1].num_features == m.out_channels
            assert isinstance(mods[i + 2], nn.LeakyReLU) and mods[i + 2].negative_slope == 0.1
    torch.manual_seed(1)
    cl = YOLOv1Classifier(4, batch_norm=True)
    assert isinstance(cl.features[-1], nn.LeakyReLU) and isinstance(cl.features[-2], nn.BatchNorm2d) and isinstance(cl.features[-3], nn.Conv2d)
    assert sum(isinstance(m, nn.Conv2d) for m in cl.features) == 20
    sd = cl.state_dict()
    feat = {k: v for k, v in sd.items() if k.startswith("features.")}
    assert len(feat) == 120 and set(sd) == set(feat) | {"fc.weight", "fc.bias"}
    own = bb.state_dict()
    for k, v in feat.items():
        assert k in own and own[k].shape == v.shape, k
    with torch.no_grad():
        for m in cl.features:
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.num_batches_tracked.fill_(3)
    before = {k: v.clone() for k, v in bb.state_dict().items()}
    assert bb.load_pretrained(cl.state_dict()) == 120
    after = bb.state_dict()
    for k, v in after.items():
        assert torch.equal(v, sd[k] if k in sd else before[k]), k
    assert int(after["features.1.num_batches_tracked"]) == 3
    # the other kind of checkpoint: refused, naming the first key that does not fit; nothing copied
    plain = YOLOv1Classifier(4).state_dict()
    with pytest.raises(KeyError, match=r"features\.0\.bias"):
        bb.load_pretrained(plain)
    assert torch.equal(bb.state_dict()["features.0.weight"], sd["features.0.weight"])
    with pytest.raises(KeyError, match=r"features\.1\.weight"):
        YOLOv1Backbone().load_pretrained(sd)
    bad = dict(sd)
    bad["features.1.running_var"] = torch.zeros(65)
    with pytest.raises(ValueError, match=r"features\.1\.running_var"):
        bb.load_pretrained(bad)
    # He initialisation leaves the BatchNorm layers as constructed
    init_kaiming_(cl)
    for m in cl.features:
        if isinstance(m, nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    # YOLOv1 around it: never one fused plan while gradients are wanted; the head is a plan of its own
    model = YOLOv1(backbone=YOLOv1Backbone(batch_norm=True))
    assert not model.train()._fusable() and not model.eval()._fusable()
    with torch.no_grad():
        assert model.eval()._fusable() and not model.train()._fusable()
    assert YOLOv1()._fusable()
    plans = model.hip_plans()
    assert len(plans) == 1 and [p for p in plans[0].params] == [model.head[1].weight, model.head[1].bias, model.head[4].weight, model.head[4].bias]
    assert len(cl.hip_plans()) == 1 and cl.hip_plans()[0].params == [cl.fc.weight, cl.fc.bias]
    assert len(YOLOv1Classifier(4).hip_plans()) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. fold
# ---------------------------------------------------------------------------------------------------------------------------------
def test_folded_modules_equal_the_batch_norm_stack_in_eval_mode():
    from yolo.models import _BNFeatures, _conv_act
    torch.manual_seed(2)
    stack = nn.Sequential(*_conv_act(3, 64, 7, 2, 3, bn=True), nn.MaxPool2d(2, 2), *_conv_act(64, 192, 3, 1, 1, bn=True), nn.MaxPool2d(2, 2),
                          *_conv_act(192, 128, 1, bn=True), *_conv_act(128, 256, 3, 2, 1, bn=True)).eval()
    with torch.no_grad():
        for m in stack:
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)
    f = _BNFeatures(stack)
    mods, fresh = f.folded()
    assert fresh and [type(m) for m in mods] == [nn.Conv2d, nn.LeakyReLU, nn.MaxPool2d, nn.Conv2d, nn.LeakyReLU, nn.MaxPool2d, nn.Conv2d, nn.LeakyReLU,
                                                 nn.Conv2d, nn.LeakyReLU]
    assert all(m.bias is not None for m in mods if isinstance(m, nn.Conv2d))
    assert not any(k.startswith("_") for k in stack.state_dict()) and len(stack.state_dict()) == 4 * 6
    x = torch.randn(2, 3, 64, 96)
    with torch.no_grad():
        want, got = stack(x), nn.Sequential(*mods)(x)
    assert lr.rel_l2(got, want) <= 1e-5
    # refreshed when a parameter or a buffer changes, the module objects stay (a plan built on them keeps its layers)
    with torch.no_grad():
        stack[1].running_mean.add_(0.5)
        stack[0].weight.mul_(1.1)
    mods2, fresh2 = f.folded()
    assert not fresh2 and all(a is b for a, b in zip(mods, mods2))
    with torch.no_grad():
        want2 = stack(x)
        assert lr.rel_l2(nn.Sequential(*mods2)(x), want2) <= 1e-5 and lr.rel_l2(want, want2) > 1e-2


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. entries
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_new_entry_is_declared_bound_and_called_by_the_gpu_test():
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "bn.hip")) as f:
        src = f.read()
    entries = set(re.findall(r"YOLO_API int (yolo_\w+)", src))
    assert entries == ENTRIES | {"yolo_batchnorm_train_fwd", "yolo_batchnorm_bwd"}
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_bn_lrelu.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header) and _hip.ABI_VERSION == 2
    assert "leaky_relu" in header and "max_pool2d" in header          # the comment names the stock-torch operations the entries replace
    from yolo.config import SWITCHES, EngineConfig
    assert EngineConfig().BN_POOL_FUSED is True and "BN_POOL_FUSED" in SWITCHES


def test_new_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call, so they can be exercised without a device; the pointers are never dereferenced"""
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    p = 4096          # a non-null address that is never read
    fgood = dict(z=p, N=2, H=6, W=10, C=64, halo=1, gamma=p, beta=p, rm=p, rv=p, pool2=0, acc=p, ss=p, out=p, out_halo=1, save=p, ready=0)

    def fwd(**kw):
        a = {**fgood, **kw}
        return L.yolo_batchnorm_train_fwd_lrelu(a["z"], a["N"], a["H"], a["W"], a["C"], a["halo"], a["gamma"], a["beta"], 1e-5, 0.1, a["rm"], a["rv"], 0.1,
                                                a["pool2"], a["acc"], a["ss"], a["out"], a["out_halo"], a["save"], a["ready"], None)
    for name in ("z", "gamma", "beta", "acc", "ss", "out"):
        assert fwd(**{name: None}) == E_ARG, name          # out == NULL included: z is always kept
    assert fwd(N=0) == E_ARG and fwd(halo=-1) == E_ARG and fwd(pool2=2) == E_ARG and fwd(ready=3) == E_ARG
    assert fwd(rm=None) == E_ARG and fwd(rm=None, rv=None, ready=2) == E_ARG
    assert fwd(C=60) == E_UNSUPPORTED
    assert fwd(pool2=1, H=7) == E_UNSUPPORTED and fwd(pool2=1, W=9) == E_UNSUPPORTED and fwd(pool2=1, H=7, W=7) == E_UNSUPPORTED
    assert b"yolo_maxpool2_fwd" in L.yolo_hip_last_error()          # the message says what to run instead
    bgood = dict(dy=p, z=p, N=2, H=6, W=10, C=64, gamma=p, save=p, pool2=0, dz=p, s_img=8 * 12 * 64, s_row=12 * 64, s_px=64, off=13 * 64, frozen=0,
                 dg=p, db=p, acc=p, coef=p)

    def bwd(**kw):
        a = {**bgood, **kw}
        return L.yolo_batchnorm_bwd_lrelu(a["dy"], 1, a["z"], 1, a["N"], a["H"], a["W"], a["C"], a["gamma"], a["save"], 0.1, a["pool2"], a["dz"], a["s_img"],
                                          a["s_row"], a["s_px"], a["off"], a["frozen"], a["dg"], a["db"], a["acc"], a["coef"], None)
    for name in ("dy", "z", "gamma", "save", "dz", "dg", "db", "acc", "coef"):
        assert bwd(**{name: None}) == E_ARG, name
    assert bwd(N=-1) == E_ARG and bwd(pool2=3) == E_ARG and bwd(frozen=2) == E_ARG
    assert bwd(C=60) == E_UNSUPPORTED and bwd(s_px=60) == E_UNSUPPORTED and bwd(off=4) == E_UNSUPPORTED
    assert bwd(pool2=1, H=7) == E_UNSUPPORTED and bwd(pool2=1, W=9) == E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. command lines
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(args, ok=True, timeout=600):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def test_command_lines_on_the_cpu(tmp_path):
    pre, det = tmp_path / "pre", tmp_path / "det"
    _run([os.path.join(PKG, "pretrain.py"), "--device", "cpu", "--batch-norm", "--synthetic", "8", "--num-classes", "4", "--image-size", "64", "--epochs", "1",
          "--batch-size", "8", "--num-workers", "0", "--checkpoint-dir", str(pre)])
    data = torch.load(pre / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert data["batch_norm"] is True and "features.1.running_mean" in data["model_state_dict"] and "features.0.bias" not in data["model_state_dict"]
    assert int(data["model_state_dict"]["features.1.num_batches_tracked"]) == 1
    common = ["--device", "cpu", "--backbone", "yolov1", "--synthetic", "2", "--batch-size", "2", "--epochs", "1", "--num-workers", "0"]
    r = _run([os.path.join(PKG, "train.py"), *common, "--batch-norm", "--backbone-weights", str(pre / "yolo_latest.pth"), "--checkpoint-dir", str(det)])
    assert "loaded 120 tensors" in r.stdout, r.stdout[-2000:]
    ck = torch.load(det / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert ck["batch_norm"] is True and "backbone.features.1.running_var" in ck["model_state_dict"]
    # refused combinations: each message names both sides
    r = _run([os.path.join(PKG, "train.py"), *common, "--batch-norm", "--deterministic"], ok=False)
    assert r.returncode == 2 and "--deterministic" in r.stderr and "--batch-norm" in r.stderr
    r = _run([os.path.join(PKG, "pretrain.py"), "--device", "cpu", "--batch-norm", "--deterministic", "--synthetic", "8"], ok=False)
    assert r.returncode == 2 and "--deterministic" in r.stderr and "--batch-norm" in r.stderr
    r = _run([os.path.join(PKG, "train.py"), "--device", "cpu", "--batch-norm", "--synthetic", "2"], ok=False)          # --backbone resnet50
    assert r.returncode == 2 and "--backbone yolov1" in r.stderr
    r = _run([os.path.join(PKG, "train.py"), *common, "--resume", str(det / "yolo_latest.pth")], ok=False)
    assert r.returncode == 2 and "batch_norm" in r.stderr and "--resume" in r.stderr
    r = _run([os.path.join(PKG, "train.py"), *common, "--backbone-weights", str(pre / "yolo_latest.pth")], ok=False)
    assert r.returncode == 2 and "batch_norm" in r.stderr and "--backbone-weights" in r.stderr
    # evaluate.py builds the BatchNorm model from the checkpoint's record
    _run([os.path.join(PKG, "evaluate.py"), "--device", "cpu", "--backbone", "yolov1", "--checkpoint", str(det / "yolo_latest.pth"), "--synthetic", "2",
          "--batch-size", "2", "--output", str(tmp_path / "ev.txt")])
    assert (tmp_path / "ev.txt").is_file()
