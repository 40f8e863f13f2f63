"""Pretraining for a real run, without a GPU: He initialisation (yolo.models.init_kaiming_, --init kaiming), the classifier under several ranks
and gradient accumulation, and the host side of pretrain.py --device-augment.  The set-ups are tests/pretrain_scale_ref.py's; children are
tests/pretrain_child.py, started through torch.distributed.run."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import accum_ref as acr
import launch_ref as lr
import pretrain_scale_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
CHILD = os.path.join(ROOT, "tests", "pretrain_child.py")


def _run(args, timeout=600):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def _two_ranks(args, port_base):
    return _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                 str(port_base + os.getpid() % 300)] + args)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. initialisation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_init_kaiming_rule_order_and_count():
    from yolo import DetectionHead, YOLOv1, YOLOv1Classifier
    from yolo.models import init_kaiming_
    gain = math.sqrt(2.0 / (1.0 + 0.1 ** 2))
    torch.manual_seed(5)
    m = YOLOv1Classifier(num_classes=7)
    fc_before = (m.fc.weight.detach().clone(), m.fc.bias.detach().clone())
    torch.manual_seed(9)
    assert init_kaiming_(m) == 40
    assert torch.equal(m.fc.weight, fc_before[0]) and torch.equal(m.fc.bias, fc_before[1]), "the logits layer keeps its initialisation"
    # the draws: torch's global generator, module order
    torch.manual_seed(9)
    for mod in m.features:
        if isinstance(mod, nn.Conv2d):
            want = nn.init.kaiming_normal_(torch.empty_like(mod.weight), a=0.1, mode="fan_in", nonlinearity="leaky_relu")
            assert torch.equal(mod.weight, want) and not mod.bias.any()
            fan = mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
            if mod.weight.numel() >= 1 << 16:
                assert abs(float(mod.weight.detach().std()) * math.sqrt(fan) / gain - 1.0) < 0.02
    # the detector: every convolution and FC1, not the output layer; a head on its own likewise
    head = DetectionHead(64, num_classes=3, S=2, B=1)
    last = head.fc_layers[4].weight.detach().clone()
    assert init_kaiming_(head) == 10 and torch.equal(head.fc_layers[4].weight, last) and not head.fc_layers[1].bias.any()
    tiny = nn.Sequential(nn.Conv2d(3, 4, 3), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(16, 8), nn.Linear(8, 2))
    kept = tiny[4].weight.detach().clone()
    assert init_kaiming_(tiny) == 4 and torch.equal(tiny[4].weight, kept) and not tiny[3].bias.any() and not tiny[0].bias.any()
    assert init_kaiming_(nn.LeakyReLU(0.1)) == 0
    del m
    assert sum(1 for mod in YOLOv1().modules() if isinstance(mod, (nn.Conv2d, nn.Linear))) == 26      # 24 convolutions + 2 Linear: 50 tensors written


def test_signal_propagation():
    """the input-dependent part of the activations behind the 20th LeakyReLU, relative to the first layer's: at least 1 % after init_kaiming_
    (14 % measured), below 1e-6 with PyTorch's default (1e-8 measured) -- the second line is a condition on stock torch, it documents why the
    flag exists"""
    he, default = ps.signal_propagation("kaiming"), ps.signal_propagation("default")
    print(f"He: first {he[0]:.3g} 20th {he[19]:.3g} ratio {he[19] / he[0]:.3g}; default: first {default[0]:.3g} 8th {default[7]:.3g} "
          f"20th {default[19]:.3g} ratio {default[19] / default[0]:.3g}")
    assert he[19] >= 0.01 * he[0]
    assert default[19] < 1e-6 * default[0]


@pytest.fixture(scope="module")
def he_curve():
    return ps.learning_loop("cpu", "kaiming")


def test_learning_from_he_init(he_curve):
    print(f"He init on the stock CPU path: first loss {he_curve[0]:.4f}, loss of step {len(he_curve)} {he_curve[-1]:.4f}")
    assert len(he_curve) == ps.LEARN_STEPS and np.isfinite(he_curve).all()
    assert he_curve[-1] < 0.75 * he_curve[0]


def test_default_init_learns_nothing():
    losses = ps.learning_loop("cpu", "default")
    print(f"default init on the stock CPU path: first loss {losses[0]:.4f}, loss of step {len(losses)} {losses[-1]:.4f}")
    assert all(abs(v - math.log(4.0)) <= 1e-3 for v in losses)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the command-line tools
# ---------------------------------------------------------------------------------------------------------------------------------
_PRE = ["--device", "cpu", "--synthetic", "8", "--num-classes", "4", "--image-size", "64", "--batch-size", "4", "--num-workers", "0", "--seed", "3"]


def test_pretrain_cli_init_kaiming(tmp_path):
    """--init kaiming is recorded, a seeded run repeats its weights bit for bit, the default records nothing, and --resume wins over the flag"""
    script = os.path.join(PKG, "pretrain.py")
    for d in ("a", "b"):
        _run([script] + _PRE + ["--epochs", "1", "--init", "kaiming", "--checkpoint-dir", str(tmp_path / d)])
    a, b = (torch.load(tmp_path / d / "yolo_latest.pth", map_location="cpu", weights_only=True) for d in ("a", "b"))
    assert a["init"] == "kaiming" and a["seed"] == 3 and "accum_steps" not in a
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), f"{k}: two seeded runs differ"
    # zero biases moved by two small steps only; a default run's are uniform in +-1 / sqrt(fan_in)
    _run([script] + _PRE + ["--epochs", "1", "--checkpoint-dir", str(tmp_path / "c")])
    c = torch.load(tmp_path / "c" / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert "init" not in c
    assert float(a["model_state_dict"]["features.3.bias"].abs().max()) < 0.1 * float(c["model_state_dict"]["features.3.bias"].abs().max())
    assert float(a["model_state_dict"]["features.3.weight"].std()) > 2.0 * float(c["model_state_dict"]["features.3.weight"].std())
    # --resume: the flag is ignored -- the same bits as a resume without it, and the record stays the file's
    for d, extra in (("r1", ["--init", "kaiming"]), ("r2", [])):
        _run([script] + _PRE + ["--epochs", "2", "--resume", str(tmp_path / "c" / "yolo_latest.pth"), "--checkpoint-dir", str(tmp_path / d)] + extra)
    r1, r2 = (torch.load(tmp_path / d / "yolo_latest.pth", map_location="cpu", weights_only=True) for d in ("r1", "r2"))
    assert r1["epoch"] == 2 and "init" not in r1
    for k, v in r1["model_state_dict"].items():
        assert torch.equal(v, r2["model_state_dict"][k]), f"{k}: --init changed a resumed run"
    assert any(not torch.equal(v, c["model_state_dict"][k]) for k, v in r1["model_state_dict"].items())


def test_train_cli_init_kaiming_before_backbone_weights(tmp_path):
    """train.py --init kaiming: applied before --backbone-weights (the 40 trunk tensors are the checkpoint's), the four detection convolutions
    and FC1 keep it, the output layer keeps PyTorch's; the checkpoint records it; --resume ignores it"""
    pre = tmp_path / "pre"
    _run([os.path.join(PKG, "pretrain.py")] + _PRE + ["--epochs", "1", "--checkpoint-dir", str(pre)])
    det = tmp_path / "det"
    common = [os.path.join(PKG, "train.py"), "--backbone", "yolov1", "--synthetic", "2", "--device", "cpu", "--batch-size", "2", "--num-workers", "0",
              "--seed", "1", "--lr", "1e-6", "--checkpoint-dir", str(det)]
    r = _run(common + ["--epochs", "1", "--init", "kaiming", "--backbone-weights", str(pre / "yolo_latest.pth")])
    assert "backbone: loaded 40 tensors" in r.stdout
    ck = torch.load(det / "yolo_latest.pth", map_location="cpu", weights_only=True)
    sd, trunk = ck["model_state_dict"], torch.load(pre / "yolo_latest.pth", map_location="cpu", weights_only=True)["model_state_dict"]
    assert ck["init"] == "kaiming"
    gain = math.sqrt(2.0 / 1.01)
    # one Adam step at lr 1e-6 moves nothing by more than ~1e-6: the initialisation is still readable
    torch.testing.assert_close(sd["backbone.features.0.weight"], trunk["features.0.weight"], rtol=0, atol=1e-5)
    for key, fan in (("backbone.features.50.weight", 1024 * 9), ("head.1.weight", 1024 * 49)):
        assert abs(float(sd[key].std()) * math.sqrt(fan) / gain - 1.0) < 0.02, key
    assert float(sd["backbone.features.50.bias"].abs().max()) < 1e-4 and float(sd["head.1.bias"].abs().max()) < 1e-4
    assert abs(float(sd["head.4.weight"].abs().max()) * math.sqrt(4096) - 1.0) < 0.05, "the output layer keeps uniform(+-1 / sqrt(fan_in))"
    _run(common + ["--epochs", "2", "--init", "default", "--resume", str(det / "yolo_latest.pth")])
    ck2 = torch.load(det / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert ck2["epoch"] == 2 and ck2["init"] == "kaiming"


# ---------------------------------------------------------------------------------------------------------------------------------
# B. ranks and accumulation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_batch():
    """the He-initialised classifier rank 0 starts from, its gradient on the 8 images as one batch, and the parameters after one SGD step"""
    from yolo import SoftmaxCrossEntropy
    m = ps.classifier(4, "kaiming", seed=100).train()
    x, y = ps.learn_set()
    loss, _ = SoftmaxCrossEntropy()(m(x), y)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    torch.optim.SGD(m.parameters(), lr=ps.LEARN_LR).step()
    return grads, {n: p.detach().clone() for n, p in m.named_parameters()}


def test_two_ranks_equal_the_full_batch(tmp_path, full_batch):
    out = tmp_path / "ranks.pt"
    _two_ranks([CHILD, "cpu_ranks", str(out)], 30900)
    r = [torch.load(f"{out}.r{k}", weights_only=True) for k in (0, 1)]
    grads, params = full_batch
    worst = 0.0
    for n, want in grads.items():
        for d in r:
            worst = max(worst, float(((d["grads"][n] - want).abs() / (1e-6 + 1e-5 * want.abs())).max()))
    print(f"two ranks x 4 images against one process x 8: worst |err| / (1e-6 + 1e-5 |ref|) {worst:.3f}")
    for n, want in grads.items():
        for d in r:
            torch.testing.assert_close(d["grads"][n], want, rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")
        assert torch.equal(r[0]["grads"][n], r[1]["grads"][n]), f"{n}: the ranks' gradients differ"
        assert torch.equal(r[0]["params"][n], r[1]["params"][n]), f"{n}: the replicas drifted apart"
        torch.testing.assert_close(r[0]["params"][n], params[n], rtol=1e-5, atol=1e-6)


def test_pretrain_cli_two_ranks_write_each_checkpoint_once(tmp_path):
    ck = tmp_path / "ck"
    r = _two_ranks([os.path.join(PKG, "pretrain.py"), "--device", "cpu", "--synthetic", "16", "--num-classes", "4", "--image-size", "64", "--batch-size", "4",
                    "--num-workers", "0", "--epochs", "1", "--init", "kaiming", "--accum-steps", "2", "--seed", "0", "--save-frequency", "1",
                    "--checkpoint-dir", str(ck)], 31300)
    assert sorted(os.listdir(ck)) == ["yolo_best_top1.pth", "yolo_epoch_1.pth", "yolo_latest.pth"], sorted(os.listdir(ck))
    text = r.stdout + r.stderr
    assert text.count("checkpoint saved") == 2 and text.count("new best model") == 1 and text.count("done:") == 1, text[-3000:]
    d = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert d["accum_steps"] == 2 and d["init"] == "kaiming" and d["epoch"] == 1
    # 16 images over 2 ranks in batches of 4: two batches per rank, one group of K = 2, one optimizer step
    moved = [k for k, s in d["optimizer_state_dict"]["state"].items() if "momentum_buffer" in s]
    assert len(moved) == 42


def test_accumulation_on_the_cpu(full_batch):
    """K = 2 x 4 images through GradAccumulator on the classifier: the folded gradient within accum_chain_ref of the two micro-gradients it was
    given (alpha = 1/2: the stock ops' separate multiplication is exact, so the chain's one rounding per link holds), and the SGD step behind it
    against the step from one batch of 8"""
    from yolo import GradAccumulator, SoftmaxCrossEntropy
    K = 2
    m = ps.classifier(4, "kaiming", seed=100).train()
    x, y = ps.learn_set()
    acc = GradAccumulator(m, K)
    assert not acc._arenas and len(acc._rest) == 42
    opt = torch.optim.SGD(m.parameters(), lr=ps.LEARN_LR)
    crit = SoftmaxCrossEntropy()
    micro = []
    for k in range(K):
        opt.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, parts = crit(m(x[4 * k: 4 * k + 4]), y[4 * k: 4 * k + 4])
        loss.backward()
        micro.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
        assert acc.after_backward(parts.device_flag) is (k == K - 1)
    assert float(acc.skip_if) == 0.0
    fails, worst = [], 0.0
    for n, p in m.named_parameters():
        ref, bnd = acr.accum_chain_ref([mg[n] for mg in micro], K)
        worst = max(worst, lr.check_values(ref, bnd, p.grad, n, fails, "folded"))
    print(f"folded gradients on the CPU: worst |err| / bound {worst:.3f}")
    assert not fails, "\n".join(fails[:12])
    opt.step()
    for n, p in m.named_parameters():
        torch.testing.assert_close(p.detach(), full_batch[1][n], rtol=1e-5, atol=1e-6, msg=lambda s, n=n: f"{n}: {s}")


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the host side of --device-augment
# ---------------------------------------------------------------------------------------------------------------------------------
def _today(image_u8, p, S):
    """the host path as the class ran it before the split, spelt out in Pillow calls: crop, resize, the colour operations in order, the flip,
    Resize (a no-op) + ToTensor + Normalize"""
    from PIL import Image, ImageEnhance
    from yolo.dataset import OP_BRIGHTNESS, OP_SATURATION, _Augment
    from yolo.inference import _Preprocess
    im = Image.fromarray(image_u8.numpy()).crop((p.left, p.top, p.left + p.cw, p.top + p.ch)).resize((S, S), Image.BILINEAR)
    for op in p.ops:
        if op == OP_BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(p.brightness)
        elif op == OP_SATURATION:
            im = ImageEnhance.Color(im).enhance(p.saturation)
        else:
            im = _Augment._hue(im, p.hue)
    if p.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return _Preprocess(size=(S, S))(im)


def test_u8_batch_on_the_cpu_equals_the_classify_transform():
    from PIL import Image
    from yolo.augment import collate_u8
    from yolo.dataset import AugParams, _ClassifyTransform
    S = 64
    cases = ps.input_cases(S)
    assert {len(p.ops) for _, p in cases} == {0, 1, 2, 3} and {p.flip for _, p in cases} == {True, False} and any(p.cw == S for _, p in cases)
    # the flip: last argument, default False; it rides beside the eight tuple entries and survives _replace, comparison and pickling
    import pickle
    q = AugParams(1, 2, 3, 4, (), 1.0, 1.0, 0.0, True)
    assert AugParams(1, 2, 3, 4).flip is False and q.flip is True and q._replace(top=5).flip is True and q._replace(flip=False).flip is False
    assert q != AugParams(1, 2, 3, 4) and q == AugParams(1, 2, 3, 4, flip=True) and tuple(q) == tuple(AugParams(1, 2, 3, 4)) and len(q) == 8
    assert pickle.loads(pickle.dumps(q)) == q and pickle.loads(pickle.dumps(q)).flip is True and "flip=True" in repr(q)
    tf = _ClassifyTransform(S, True)
    want = torch.stack([tf.apply(Image.fromarray(im.numpy()), p) for im, p in cases])
    batch, labels = collate_u8([(im, p, torch.tensor(i % 4)) for i, (im, p) in enumerate(cases)], size=(S, S))
    got = batch.to_tensor()
    assert got.shape == (len(cases), 3, S, S) and labels.tolist() == [i % 4 for i in range(len(cases))] and labels.dtype == torch.int64
    assert torch.equal(got, want)
    assert torch.equal(want, torch.stack([_today(im, p, S) for im, p in cases]))
    assert not torch.equal(got[0], got[1].flip(-1)) and not torch.equal(got[5], got[5].flip(-1))
    # sampled parameters: sample + apply is __call__ on the same draws
    for i, (im, _) in enumerate(cases[:4]):
        pil = Image.fromarray(im.numpy())
        torch.manual_seed(40 + i)
        a = tf(pil)
        torch.manual_seed(40 + i)
        p = tf.sample(*pil.size)
        assert torch.equal(a, tf.apply(pil, p)) and torch.equal(a, collate_u8([(im, p, torch.tensor(0))], size=(S, S))[0].to_tensor()[0])


def test_datasets_without_device_transform_are_unchanged(tmp_path):
    """device_transform=False: the samples and the random stream of the class path that did not change (_Augment.__call__, one rand for the
    flip, _Preprocess), produced here; device_transform=True: the same draws as parameters, and the same tensors through collate_u8"""
    from PIL import Image
    from yolo.augment import collate_u8
    from yolo.dataset import AugParams, ImageFolderClassification, SyntheticClassificationDataset, _Augment
    from yolo.inference import _Preprocess
    S = 64
    for split in ("train", "val"):
        for ci, cls in enumerate(("ant", "bee")):
            d = tmp_path / split / cls
            d.mkdir(parents=True)
            for i in range(2):
                Image.fromarray(ps.image(70 + 9 * i + ci, 90 - 11 * i, 10 * ci + i).numpy(), "RGB").save(d / f"{i}.png")

    def unchanged(pil, train):
        if train:
            pil, _ = _Augment((S, S))(pil, [])
            if float(torch.rand(1).item()) < 0.5:
                pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        return _Preprocess(size=(S, S))(pil)

    flips = 0
    for train in (True, False):
        sets = [(SyntheticClassificationDataset(6, 3, S, seed=2, train=train), SyntheticClassificationDataset(6, 3, S, seed=2, train=train, device_transform=True)),
                (ImageFolderClassification(tmp_path, "train" if train else "val", S), ImageFolderClassification(tmp_path, "train" if train else "val", S, device_transform=True))]
        for host, dev in sets:
            assert host.device_transform is False and dev.device_transform is True
            pil = (lambda i: host.image(i)) if hasattr(host, "image") else (lambda i: Image.open(host.samples[i][0]).convert("RGB"))
            for i in range(len(host)):
                torch.manual_seed(7 + i)
                want, state_want = unchanged(pil(i), train), torch.get_rng_state()
                torch.manual_seed(7 + i)
                (got, label), state_got = host[i], torch.get_rng_state()
                assert torch.equal(got, want) and torch.equal(state_got, state_want) and isinstance(label, int)
                torch.manual_seed(7 + i)
                (u8, p, lab), state_dev = dev[i], torch.get_rng_state()
                assert torch.equal(state_dev, state_want), "the device path draws what the host path draws"
                assert u8.dtype == torch.uint8 and u8.shape[2] == 3 and isinstance(p, AugParams) and int(lab) == label and lab.dtype == torch.int64
                assert torch.equal(collate_u8([(u8, p, lab)], size=(S, S))[0].to_tensor()[0], want)
                if not train:
                    assert p == AugParams(0, 0, u8.shape[0], u8.shape[1])
                flips += bool(p.flip)
    assert 0 < flips < 10
