"""Pretraining for a real run, on the device: uint8 batches into YOLOv1Classifier (pretrain.py --device-augment), yolo.optim.GradAccumulator and
the overlapped reducers on the classifier's two plans, learning from He initialisation, and pretrain.py with all of it switched on.  The
set-ups are tests/pretrain_scale_ref.py's; every child (tests/pretrain_child.py, the command-line tools) runs under its own time limit."""

import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import accum_ref as acr
import launch_ref as lr
import pretrain_scale_ref as ps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
CHILD = os.path.join(ROOT, "tests", "pretrain_child.py")


def _child(args, limit, **extra_env):
    """a fresh child under its own time limit; its exit status is checked before anything else runs"""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra_env)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"{args}: exit status {r.returncode}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def _two_ranks(args, limit, port_base, **extra_env):
    return _child(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                   str(port_base + os.getpid() % 300)] + args, limit, **extra_env)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. U8Batch into the classifier
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 224])
def test_u8_batch_into_the_classifier(S):
    """the cases of the CPU test through yolo_augment_u8: the fp32 batch bit-identical to the host path (_ClassifyTransform.apply), the trunk
    plan's stem buffer filled from the U8Batch bit-identical to the one filled from that fp32 batch, and model(batch) against
    model(batch.to_tensor()) within the bound tests/test_gpu_augment.py sets for two forwards of one input of the detector"""
    from PIL import Image
    from yolo._hip import check, lib, ptr, stream
    from yolo.augment import collate_u8
    from yolo.dataset import _ClassifyTransform
    from yolo.engine import Act
    cases = ps.input_cases(S)
    N = len(cases)
    tf = _ClassifyTransform(S, True)
    want = torch.stack([tf.apply(Image.fromarray(im.numpy()), p) for im, p in cases])
    batch, _ = collate_u8([(im, p, torch.tensor(0)) for im, p in cases], size=(S, S))
    dev = batch.cuda()
    assert [int(d.flags) for d in dev._descs] == [1 if p.flip else 0 for _, p in cases]
    got = dev.to_tensor()
    assert got.is_cuda and got.dtype == torch.float32
    for i, (_, p) in enumerate(cases):
        assert torch.equal(got[i].cpu(), want[i]), f"image {i} {p}: {(got[i].cpu() != want[i]).sum().item()} values differ"
    a, b = Act(N, S, S, 4, 3, got.device), Act(N, S, S, 4, 3, got.device)
    check(lib().yolo_nchw_f32_to_nhwc_bf16(ptr(got), N, 3, S, S, a.p, 4, 3, 3, stream()), "nchw->nhwc4")
    dev.into_act(b)
    assert torch.equal(a.store, b.store)
    m = ps.classifier(4, "kaiming").cuda()
    for mode in (m.eval(), m.train()):
        with torch.no_grad():
            ref = mode(got)
            out = mode(dev)
        assert out.shape == (N, 4) and float(ref.abs().mean()) > 1e-3
        torch.testing.assert_close(out, ref, rtol=0, atol=1e-3 * ref.abs().mean().item())
    # training from the batch: every gradient arrives
    from yolo import SoftmaxCrossEntropy
    loss, parts = SoftmaxCrossEntropy()(m(dev), torch.arange(N, device="cuda") % 4)
    loss.backward()
    assert np.isfinite(parts["total"])
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0.0, n
    # the CPU model takes the batch as its fp32 tensor
    if S == 64:
        cpu = ps.classifier(4, "kaiming").eval()
        with torch.no_grad():
            assert torch.equal(cpu(batch), cpu(want))
    m.cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the accumulator and the reducers on the classifier's two plans
# ---------------------------------------------------------------------------------------------------------------------------------
def _group(m, opt, acc, x, y, K, keep=None):
    from yolo import SoftmaxCrossEntropy
    crit = SoftmaxCrossEntropy()
    for k in range(K):
        opt.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, parts = crit(m(x[2 * k: 2 * k + 2]), y[2 * k: 2 * k + 2])
        loss.backward()
        if keep is not None:
            keep.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
        assert acc.after_backward(parts.device_flag) is (k == K - 1)


def test_accumulator_finds_both_plans_teacher_forced():
    """K = 3 micro-batches of 2 images through GradAccumulator on YOLOv1Classifier: an arena on each plan, no parameter left outside; every
    parameter's folded gradient within accum_chain_ref of the three micro-gradients it was given (cloned after each backward), p.grad still its
    plan's arena view; then SGD(max_grad_norm=10) moves every parameter"""
    from yolo import GradAccumulator
    from yolo.optim import SGD
    K = 3
    m = ps.classifier(4, "kaiming").cuda().train()
    x, y = ps.learn_set("cuda")
    opt = SGD(m.parameters(), lr=ps.LEARN_LR, max_grad_norm=ps.CLIP)
    opt.attach_plan(m.head_plan())
    acc = GradAccumulator(m, K)
    plans = m.hip_plans()
    assert len(acc._arenas) == 2 and not acc._rest and all(p.arena is not None and p.on_grad_ready is None for p in plans)
    assert {id(a[0]) for a in acc._arenas} == {id(p) for p in plans} and all(a[1].numel() == a[0].arena.numel() and not a[2] for a in acc._arenas)
    micro = []
    _group(m, opt, acc, x, y, K, micro)
    torch.cuda.synchronize()
    assert float(acc.skip_if) == 0.0 and not any(p.grad_norm_sq for p in plans)
    spans = [(p.arena.data_ptr(), p.arena.data_ptr() + 4 * p.arena.numel()) for p in plans]
    fails, worst = [], 0.0
    for n, p in m.named_parameters():
        lo, hi = spans[1] if n.startswith("fc.") else spans[0]
        assert lo <= p.grad.data_ptr() < hi, f"{n}: p.grad is not its plan's arena view"
        ref, bnd = acr.accum_chain_ref([mg[n] for mg in micro], K)
        worst = max(worst, lr.check_values(ref, bnd, p.grad, n, fails, "folded"))
        assert not torch.equal(p.grad, micro[-1][n]), f"{n}: the fold did not happen"
    print(f"folded gradients: worst |err| / bound {worst:.3f}")
    assert not fails, "\n".join(fails[:12])
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.skip_if = acc.skip_if
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n}: the step did not move"


def test_accumulated_groups_repeat_bit_for_bit_under_deterministic_mode(monkeypatch):
    """EngineConfig.DETERMINISTIC on both plans: two identical groups of K = 2 from the same weights leave the same folded gradients and the
    same stepped parameters"""
    from yolo import GradAccumulator
    from yolo.config import CONFIG
    from yolo.optim import SGD
    monkeypatch.setattr(CONFIG, "DETERMINISTIC", True)
    x, y = ps.learn_set("cuda")
    K, runs = 2, []
    for _ in range(2):
        m = ps.classifier(4, "kaiming").cuda().train()
        for plan in m.hip_plans():
            plan.cfg = dataclasses.replace(CONFIG, DETERMINISTIC=True)
        opt = SGD(m.parameters(), lr=ps.LEARN_LR, momentum=0.9, max_grad_norm=ps.CLIP)
        opt.attach_plan(m.head_plan())
        acc = GradAccumulator(m, K)
        _group(m, opt, acc, x, y, K)
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        opt.skip_if = acc.skip_if
        opt.step()
        torch.cuda.synchronize()
        runs.append((grads, {n: p.detach().clone() for n, p in m.named_parameters()}))
    for what, a, b in (("folded gradient", runs[0][0], runs[1][0]), ("stepped parameter", runs[0][1], runs[1][1])):
        for n in a:
            assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{what} {n} differs between two identical groups"


def test_two_ranks_one_collective_group_per_k_backward_passes(tmp_path):
    """two ranks on one GPU over gloo (tests/pretrain_child.py ranks), deterministic mode, K = 2, 2 images per micro-batch per rank, the shipped
    path: make_grad_reducer (one overlapped reducer per plan, head first) + GradAccumulator + SGD.step.  No reducer enqueued a bucket during the
    first micro-step, each did during the second; the ranks' gradients and replicas are bit-equal; the gradients lie within accum_ranks_ref's
    bound of the fp64 mean of the four raw micro-gradients"""
    out = tmp_path / "ranks.pt"
    _two_ranks([CHILD, "ranks", str(out)], 300, 30100, YOLO_AMD_DETERMINISTIC="1")
    r = [torch.load(f"{out}.r{k}", weights_only=True) for k in (0, 1)]
    for d in r:
        assert d["reducers"] == ["OverlappedGradAllReduce", "OverlappedGradAllReduce"] and d["deterministic"] is True
        assert d["buckets_after_micro_1"] == [0, 0] and min(d["buckets"]) >= 1, "no bucket during the first micro-step, all of them during the second"
        assert d["skip"] == 0.0
    assert list(r[0]["grads"]) == list(r[1]["grads"]) and len(r[0]["grads"]) >= 22
    for n in r[0]["grads"]:
        assert torch.equal(r[0]["grads"][n].view(torch.int32), r[1]["grads"][n].view(torch.int32)), f"{n}: the ranks' gradients differ"
    for n in r[0]["params"]:
        assert torch.equal(r[0]["params"][n].view(torch.int32), r[1]["params"][n].view(torch.int32)), f"{n}: the replicas drifted apart"
    fails, worst = [], 0.0
    for n, got in r[0]["grads"].items():
        chains = [acr.accum_chain_ref([d["raw"][0][n], d["raw"][1][n]], 2) for d in r]
        ref, bnd = acr.accum_ranks_ref(chains)
        worst = max(worst, lr.check_values(ref, bnd, got, n, fails, "two ranks"))
        assert not torch.equal(got, r[0]["raw"][1][n]), f"{n}: the reduced gradient is rank 0's last micro-gradient"
    print(f"two ranks: worst |err| / bound {worst:.3f} over {len(r[0]['grads'])} tensors")
    assert not fails, "\n".join(fails[:12])


# ---------------------------------------------------------------------------------------------------------------------------------
# A. learning from He initialisation
# ---------------------------------------------------------------------------------------------------------------------------------
def test_learning_from_he_init_on_the_device():
    """the learning run of tests/test_pretrain_scale_cpu.py on the device against the stock CPU curve computed here: the first loss within
    3 %, the last at most 1.25 x the CPU's ("Classification pretraining": bf16 storage lags the fp32 curve by a few steps)"""
    cpu = ps.learning_loop("cpu", "kaiming")
    dev = ps.learning_loop("cuda", "kaiming")
    print(f"learning from He init: device first {dev[0]:.4f} last {dev[-1]:.4f}; stock CPU path first {cpu[0]:.4f} last {cpu[-1]:.4f}")
    assert len(dev) == ps.LEARN_STEPS and np.isfinite(dev).all()
    assert abs(dev[0] - cpu[0]) <= 0.03 * cpu[0], dev[0]
    assert dev[-1] <= 1.25 * cpu[-1], dev


# ---------------------------------------------------------------------------------------------------------------------------------
# the command-line tools
# ---------------------------------------------------------------------------------------------------------------------------------
_CLI = ["--device", "cuda", "--synthetic", "16", "--num-classes", "4", "--image-size", "64", "--init", "kaiming", "--accum-steps", "2", "--device-augment",
        "--deterministic", "--epochs", "1", "--batch-size", "2", "--num-workers", "0"]


def _check(ckdir):
    d = torch.load(ckdir / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert d["init"] == "kaiming" and d["accum_steps"] == 2 and d["deterministic"] is True and d["seed"] == 0 and d["epoch"] == 1
    assert all(bool(torch.isfinite(v).all()) for v in d["model_state_dict"].values())
    assert np.isfinite(d["train_loss"]) and np.isfinite(d["val_loss"]) and 0.0 <= d["val_top1"] <= 1.0
    assert sorted(os.listdir(ckdir)) == ["yolo_best_top1.pth", "yolo_latest.pth"]
    return d


def test_pretrain_cli_one_process_then_train_from_its_checkpoint(tmp_path):
    ck = tmp_path / "one"
    r = _child([os.path.join(PKG, "pretrain.py")] + _CLI + ["--checkpoint-dir", str(ck)], 300)
    assert r.stdout.count("checkpoint saved") == 1 and "done:" in r.stdout
    _check(ck)
    r = _child([os.path.join(PKG, "train.py"), "--device", "cuda", "--backbone", "yolov1", "--backbone-weights", str(ck / "yolo_latest.pth"), "--init", "kaiming",
                "--synthetic", "2", "--batch-size", "2", "--num-workers", "0", "--epochs", "1", "--checkpoint-dir", str(tmp_path / "det")], 600)
    assert "backbone: loaded 40 tensors" in r.stdout
    det = torch.load(tmp_path / "det" / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert det["init"] == "kaiming" and all(bool(torch.isfinite(v).all()) for v in det["model_state_dict"].values())


def test_pretrain_cli_two_ranks(tmp_path):
    """pretrain.py's main() as two ranks on one GPU (tests/pretrain_child.py cli): rank 0 writes each checkpoint once"""
    ck = tmp_path / "two"
    r = _two_ranks([CHILD, "cli"] + _CLI + ["--checkpoint-dir", str(ck)], 300, 30500)
    text = r.stdout + r.stderr
    assert text.count("checkpoint saved") == 1 and text.count("done:") == 1, text[-3000:]
    _check(ck)
