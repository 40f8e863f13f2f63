"""csrc/classify.hip on the GPU -- the global average pool, its backward and the fused softmax cross-entropy, called through the C ABI with guard
bands around every output (tests/elementwise_ref.Guarded, as in test_gpu_layout.py) against the fp64 restatements of tests/classify_ref.py -- then
the modules built on them (GlobalAvgPool, SoftmaxCrossEntropy, YOLOv1Classifier), a deterministic training step and one learning check.

Tolerances
  * pool forward: |err| <= (HW + 2) * 2^-24 * sum|x| / HW per output (an fp32 sum of HW terms plus one multiply); backward: bit for bit.
  * loss / dlogits: 4 x the error of stock torch's own fp32 CPU F.cross_entropy (forward, autograd backward) against the same fp64 formulas on
    the same inputs, measured by `python tests/classify_ref.py` (torch_fp32_error): loss 1.984e-07 relative to max(|ref|, 1), dlogits 5.772e-07
    absolute -> LOSS_TOL, DLOGITS_TOL below (the kernel may order its sums differently from torch, hence the factor).  hits: exact.
  * classifier logits against the stock CPU modules: what tests/test_gpu_model.py:41-43 applies to the whole YOLOv1 forward (relative RMS < 0.03,
    max |err| < 0.15 max|ref|); the Linear weight gradient: the bf16 bound of test_gpu_layers.py:179-181 (_close with k = 8, 1 % outliers).
  * learning check: classify_ref.learning_loop on the stock CPU path gave a first loss of 1.4278 and 0.1469 at step 20 (`python
    tests/classify_ref.py`).  The device run must start within 3 % of the first (the forward tolerance above, on a loss of O(1)) and reach
    1.25 x the CPU's final loss: the CPU curve falls by 6-7 % per step there, so the margin is a lag of three steps for bf16 storage.
"""

import copy
import dataclasses

import numpy as np
import pytest
import torch

import classify_ref as cr
import elementwise_ref as er

pytestmark = pytest.mark.gpu

E_ARG = -1
TORCH_FP32_LOSS_ERR, TORCH_FP32_DLOGITS_ERR = 1.984e-07, 5.772e-07        # measured: python tests/classify_ref.py ("Classification pretraining")
LOSS_TOL, DLOGITS_TOL = 4 * TORCH_FP32_LOSS_ERR, 4 * TORCH_FP32_DLOGITS_ERR
CPU_FIRST_LOSS, CPU_FINAL_LOSS, LEARN_MARGIN = 1.4278, 0.1469, 1.25


def _L():
    from yolo._hip import lib
    return lib()


def _st():
    from yolo._hip import stream
    return stream()


def _ok(rc):
    assert rc == 0, _L().yolo_hip_last_error().decode(errors="replace")


def _guarded(n, fill=7.0):
    return er.Guarded(torch.full((n,), fill, dtype=torch.float32).cuda())


# ---- global average pool ----------------------------------------------------------------------------------------------------------------------

GAP_SHAPES = [(N, C, HW) for N in (1, 3) for C in (8, 1024) for HW in (1, 49, 50, 196)]


@pytest.mark.parametrize("N,C,HW", GAP_SHAPES)
def test_gap_forward(N, C, HW):
    rng = np.random.Generator(np.random.PCG64([N, C, HW]))
    x = (3.0 * rng.standard_normal((N, C, HW))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    runs = []
    for _ in range(2):
        y = _guarded(N * C)
        _ok(_L().yolo_gap_fwd(xd.data_ptr(), N, C, HW, y.ptr, _st()))
        torch.cuda.synchronize()
        assert y.guards_ok(), "guard band overwritten"
        runs.append(y.t.cpu().numpy().reshape(N, C))
    assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)), "two calls differ"
    err = np.abs(runs[0].astype(np.float64) - cr.gap(x))
    bound = cr.gap_bound(x)
    print(f"gap fwd {N}x{C}x{HW}: max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"max err / bound {(err / bound).max():.3f}"


@pytest.mark.parametrize("N,C,HW", GAP_SHAPES)
def test_gap_backward(N, C, HW):
    rng = np.random.Generator(np.random.PCG64([N, C, HW, 1]))
    dy = rng.standard_normal((N, C)).astype(np.float32)
    dx = _guarded(N * C * HW)
    _ok(_L().yolo_gap_bwd(torch.from_numpy(dy).cuda().data_ptr(), N, C, HW, dx.ptr, _st()))
    torch.cuda.synchronize()
    assert dx.guards_ok(), "guard band overwritten"
    assert np.array_equal(dx.t.cpu().numpy().reshape(N, C, HW).view(np.int32), cr.gap_bwd(dy, HW).view(np.int32))


def test_gap_backward_into_an_unaligned_buffer():
    """dx 4 bytes past a 16-B boundary: the 4-B store form, same values, neighbours untouched"""
    N, C, HW = 2, 8, 49
    dy = np.random.Generator(np.random.PCG64(9)).standard_normal((N, C)).astype(np.float32)
    buf = _guarded(N * C * HW + 2)
    _ok(_L().yolo_gap_bwd(torch.from_numpy(dy).cuda().data_ptr(), N, C, HW, buf.ptr + 4, _st()))
    torch.cuda.synchronize()
    got = buf.t.cpu().numpy()
    assert buf.guards_ok() and got[0] == 7.0 and got[-1] == 7.0
    assert np.array_equal(got[1:-1].reshape(N, C, HW), cr.gap_bwd(dy, HW))


def test_gap_rejects_bad_arguments():
    x = torch.zeros(64, device="cuda")
    p = x.data_ptr()
    for fn in (_L().yolo_gap_fwd, _L().yolo_gap_bwd):
        assert fn(None, 1, 8, 8, p, _st()) == E_ARG and fn(p, 1, 8, 8, None, _st()) == E_ARG
        assert fn(p, -1, 8, 8, p, _st()) == E_ARG and fn(p, 1, 0, 8, p, _st()) == E_ARG and fn(p, 1, 8, 0, p, _st()) == E_ARG
    torch.cuda.synchronize()
    assert not bool(x.any())


# ---- softmax cross-entropy ----------------------------------------------------------------------------------------------------------------------

def _xent_call(x, y, eps, want_grad=True):
    """one call through the C ABI with every output between guard bands -> (out [2], dlogits [N][K] | None, hits [N][2], work [N]) as numpy"""
    N, K = x.shape
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    out, hits, work = _guarded(2), _guarded(2 * N), _guarded(2 * N)          # (int32 and f64 outputs ride in fp32 buffers of the same byte size)
    dl = _guarded(N * K) if want_grad else None
    _ok(_L().yolo_softmax_xent_fwd_bwd(xd.data_ptr(), yd.data_ptr(), N, K, float(eps), out.ptr, dl.ptr if want_grad else None, hits.ptr, work.ptr, _st()))
    torch.cuda.synchronize()
    for g, what in ((out, "out"), (hits, "hits"), (work, "work"), (dl, "dlogits")):
        assert g is None or g.guards_ok(), f"{what}: guard band overwritten"
    return (out.t.cpu().numpy(), dl.t.cpu().numpy().reshape(N, K) if want_grad else None, hits.t.view(torch.int32).cpu().numpy().reshape(N, 2),
            work.t.view(torch.float64).cpu().numpy())


@pytest.mark.parametrize("eps", cr.XENT_EPS)
@pytest.mark.parametrize("N,K", cr.XENT_SHAPES)
def test_softmax_xent(N, K, eps):
    worst_l = worst_d = 0.0
    for shift in range(len(cr.KINDS)):
        x, y = cr.xent_case(N, K, shift)
        ref_l, ref_rows, ref_d, ref_h, _ = cr.xent(x, y, eps)
        out, dl, hits, work = _xent_call(x, y, eps)
        out2, dl2, hits2, _ = _xent_call(x, y, eps)
        outf, _, hitsf, _ = _xent_call(x, y, eps, want_grad=False)
        what = f"N={N} K={K} eps={eps} shift={shift}"
        assert np.array_equal(hits, ref_h), what
        assert out[1] == 0.0, what
        el, ed = cr.loss_err(out[0], ref_l), float(np.abs(dl.astype(np.float64) - ref_d).max())
        worst_l, worst_d = max(worst_l, el), max(worst_d, ed)
        assert el <= LOSS_TOL, f"{what}: loss {out[0]!r} vs {ref_l!r}: {el:.3e} > {LOSS_TOL:.3e}"
        assert ed <= DLOGITS_TOL, f"{what}: dlogits error {ed:.3e} > {DLOGITS_TOL:.3e}"
        assert np.abs(work - ref_rows).max() <= 1e-6 * max(1.0, np.abs(ref_rows).max()), f"{what}: row losses"
        assert np.array_equal(out.view(np.int32), out2.view(np.int32)) and np.array_equal(dl.view(np.int32), dl2.view(np.int32)) \
            and np.array_equal(hits, hits2), f"{what}: two calls differ"
        assert np.array_equal(out.view(np.int32), outf.view(np.int32)) and np.array_equal(hits, hitsf), f"{what}: forward only differs"
    print(f"xent N={N} K={K} eps={eps}: loss err {worst_l:.3e} (tol {LOSS_TOL:.3e}), dlogits err {worst_d:.3e} (tol {DLOGITS_TOL:.3e})")


@pytest.mark.parametrize("eps", cr.XENT_EPS)
def test_softmax_xent_invalid_labels(eps):
    for N, K, bad in ((5, 7, {1: -1, 3: 7}), (4, 1000, {0: 1000, 3: -1}), (3, 4099, {1: 1 << 40}), (1, 1, {0: 1})):
        x, y = cr.xent_case(N, K, 0)
        for r, v in bad.items():
            y[r] = v
        ref_l, ref_rows, ref_d, ref_h, flag = cr.xent(x, y, eps)
        out, dl, hits, work = _xent_call(x, y, eps)
        assert flag == 1.0 and out[1] == 1.0
        for r in bad:
            assert not dl[r].any() and not hits[r].any() and work[r] == 0.0, (N, K, r)
        assert np.array_equal(hits, ref_h)
        assert cr.loss_err(out[0], ref_l) <= LOSS_TOL and np.abs(dl.astype(np.float64) - ref_d).max() <= DLOGITS_TOL, (N, K)


def test_softmax_xent_rejects_bad_arguments():
    z = torch.zeros(64, device="cuda")
    p = z.data_ptr()
    good = dict(logits=p, labels=p, N=2, K=5, eps=0.1, out=p, dlogits=p, hits=p, work=p)

    def call(**kw):
        a = {**good, **kw}
        return _L().yolo_softmax_xent_fwd_bwd(a["logits"], a["labels"], a["N"], a["K"], a["eps"], a["out"], a["dlogits"], a["hits"], a["work"], _st())
    for name in ("logits", "labels", "out", "hits", "work"):
        assert call(**{name: None}) == E_ARG, name
    assert call(N=-1) == E_ARG and call(K=0) == E_ARG
    for eps in (-0.1, 1.0, float("nan")):
        assert call(eps=eps) == E_ARG, eps
    torch.cuda.synchronize()
    assert not bool(z.any()), "a rejected call must not launch"


# ---- modules ------------------------------------------------------------------------------------------------------------------------------------

def test_global_avg_pool_module():
    from yolo import GlobalAvgPool
    torch.manual_seed(4)
    x = torch.randn(3, 40, 7, 7)
    gy = torch.randn(3, 40, 1, 1)
    xc, xg = x.clone().requires_grad_(True), x.cuda().requires_grad_(True)
    yc, yg = GlobalAvgPool()(xc), GlobalAvgPool()(xg)
    yc.backward(gy)
    yg.backward(gy.cuda())
    assert yg.shape == (3, 40, 1, 1) and yg.is_cuda
    xs = x.numpy().reshape(3, 40, 49)
    assert (np.abs(yg.detach().cpu().numpy().reshape(3, 40).astype(np.float64) - cr.gap(xs)) <= cr.gap_bound(xs)).all()
    assert (np.abs(yc.detach().numpy().reshape(3, 40).astype(np.float64) - cr.gap(xs)) <= cr.gap_bound(xs)).all()
    assert np.array_equal(xg.grad.cpu().numpy().reshape(3, 40, 49), cr.gap_bwd(gy.numpy().reshape(3, 40), 49))
    torch.testing.assert_close(xg.grad.cpu(), xc.grad, rtol=2.0 ** -22, atol=0.0)       # autograd divides by HW, the kernel multiplies by fp32(1 / HW)


@pytest.mark.parametrize("eps", cr.XENT_EPS)
def test_softmax_cross_entropy_module(eps):
    from yolo import SoftmaxCrossEntropy
    x, y = cr.xent_case(5, 7, 0)
    crit = SoftmaxCrossEntropy(label_smoothing=eps)
    lc = torch.from_numpy(x).clone().requires_grad_(True)
    lg = torch.from_numpy(x).cuda().requires_grad_(True)
    loss_c, parts_c = crit(lc, torch.from_numpy(y))
    loss_g, parts_g = crit(lg, torch.from_numpy(y).cuda())
    (2.0 * loss_c).backward()
    (2.0 * loss_g).backward()
    ref_l, _, ref_d, ref_h, _ = cr.xent(x, y, eps)
    # no explicit synchronisation: reading the parts waits for their copy
    assert set(parts_g.keys()) == {"total", "top1", "top5"} and parts_g.device_flag.is_cuda
    assert parts_g["top1"] == ref_h[:, 0].mean() == parts_c["top1"] and parts_g["top5"] == ref_h[:, 1].mean() == parts_c["top5"]
    assert cr.loss_err(parts_g["total"], ref_l) <= LOSS_TOL and cr.loss_err(loss_g.item(), ref_l) <= LOSS_TOL
    assert np.abs(lg.grad.cpu().numpy().astype(np.float64) - 2.0 * ref_d).max() <= 2.0 * DLOGITS_TOL
    # against the CPU path: the device within 4 x, stock torch within 1 x the measured error of the fp64 value
    assert cr.loss_err(loss_g.item(), loss_c.item()) <= 1.25 * LOSS_TOL
    assert (lg.grad.cpu() - lc.grad).abs().max().item() <= 2.0 * 1.25 * DLOGITS_TOL
    assert float(parts_g.device_flag) == 0.0
    # a label outside [0, K): flagged on the device, raised at the first read, and the optimizer's skip_if takes the flag
    y2 = y.copy()
    y2[0] = 7
    loss2, parts2 = crit(torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y2).cuda())
    assert float(parts2.device_flag) == 1.0 and parts2.device_flag.dtype == torch.float32 and parts2.device_flag.numel() == 1
    with pytest.raises(RuntimeError, match="label out of bounds"):
        parts2["total"]
    with pytest.raises(RuntimeError, match=r"\(N, K\)"):
        crit(torch.zeros(4, 7, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"))


@pytest.fixture(scope="module")
def classifier_step():
    """YOLOv1Classifier(24), batch 2 at 224 x 224: the stock CPU forward once, shared by the tests below"""
    import synth
    m = cr.synth_classifier(24).eval()
    x = torch.from_numpy(synth.synth_images(2, 12, hw=224))
    with torch.no_grad():
        ref = m(x)
    return m, x, ref


def _rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_classifier_forward_and_backward(classifier_step, mode):
    from test_gpu_layers import _close
    from yolo import SoftmaxCrossEntropy
    m_cpu, x, ref = classifier_step
    m = copy.deepcopy(m_cpu).cuda()
    m = m.train() if mode == "train" else m.eval()
    pooled = []
    hook = m.pool.register_forward_hook(lambda _m, _i, out: pooled.append(out.detach()))
    logits = m(x.cuda())
    hook.remove()
    assert logits.shape == (2, 24) and logits.dtype == torch.float32
    r = _rel(logits.detach(), ref)
    print(f"classifier logits ({mode}): relative RMS {r:.4f}, max err / max|ref| {((logits.detach().cpu() - ref).abs().max() / ref.abs().max()).item():.4f}")
    assert r < 0.03, r                                                                       # tests/test_gpu_model.py:41-43
    assert (logits.detach().cpu() - ref).abs().max() < 0.15 * ref.abs().max()
    with torch.no_grad():                                                                    # the inference launches (fused pools, blocked Linear panels)
        plain = m(x.cuda())
    assert not plain.requires_grad and _rel(plain, ref) < 0.03 and (plain.cpu() - ref).abs().max() < 0.15 * ref.abs().max()
    logits.retain_grad()
    loss, parts = SoftmaxCrossEntropy(0.1)(logits, torch.tensor([3, 17], device="cuda"))
    loss.backward()
    assert np.isfinite(parts["total"]) and parts["top5"] in (0.0, 0.5, 1.0)
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0.0, n
    # the Linear layer's weight gradient from the device's own operands: dW[k][c] = sum_n dlogits[n][k] * pooled[n][c]
    dW = logits.grad.double().t() @ pooled[0].double().view(2, 1024)
    _close(m.fc.weight.grad, dW.float(), 8.0, "fc weight gradient", frac=0.01)               # tests/test_gpu_layers.py:179-181
    # the bias gradient is the column sum of the bf16-rounded dlogits: two terms, each within 2^-9 of its value
    assert (m.fc.bias.grad - logits.grad.sum(0)).abs().max().item() <= 2 * 2.0 ** -8 * logits.grad.abs().max().item()


def test_deterministic_step_repeats_bit_for_bit(classifier_step, monkeypatch):
    """EngineConfig.DETERMINISTIC on both plans (and on the optimizer's gradient norm): forward, loss, backward and the fused clip + SGD step from
    the same weights leave the same bits, gradient by gradient and parameter by parameter"""
    from yolo import SoftmaxCrossEntropy
    from yolo.config import CONFIG
    from yolo.optim import SGD
    monkeypatch.setattr(CONFIG, "DETERMINISTIC", True)
    m_cpu, x, _ = classifier_step
    y = torch.tensor([5, 20], device="cuda")
    results = []
    for _ in range(2):
        m = copy.deepcopy(m_cpu).cuda().train()
        for plan in m.hip_plans():
            plan.cfg = dataclasses.replace(CONFIG, DETERMINISTIC=True)
        opt = SGD(m.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
        crit = SoftmaxCrossEntropy(0.1)
        for _step in range(2):
            opt.zero_grad(set_to_none=True)
            loss, parts = crit(m(x.cuda()), y)
            loss.backward()
            opt.skip_if = parts.device_flag
            grads = [p.grad.detach().clone() for p in m.parameters()]
            opt.step()
        torch.cuda.synchronize()
        results.append((loss.detach().clone(), grads, [p.detach().clone() for p in m.parameters()]))
    (la, ga, pa), (lb, gb, pb) = results
    assert torch.equal(la, lb)
    names = [n for n, _ in m.named_parameters()]
    for n, a, b in zip(names, ga, gb):
        assert torch.equal(a, b), f"gradient of {n} differs between two identical steps"
    for n, a, b, p0 in zip(names, pa, pb, m_cpu.parameters()):
        assert torch.equal(a, b), f"{n} differs after two identical steps"
        assert not torch.equal(a.cpu(), p0), f"{n} was not updated"


def test_learning_check():
    losses = cr.learning_loop("cuda")
    print(f"learning check on the device: first loss {losses[0]:.4f}, loss of step {len(losses)} {losses[-1]:.4f} "
          f"(stock CPU path: {CPU_FIRST_LOSS}, {CPU_FINAL_LOSS})")
    assert len(losses) == cr.LEARN_STEPS and np.isfinite(losses).all()
    assert abs(losses[0] - CPU_FIRST_LOSS) <= 0.03 * CPU_FIRST_LOSS, losses[0]
    assert losses[-1] <= LEARN_MARGIN * CPU_FINAL_LOSS, losses


def test_pretrain_cli_on_the_device(tmp_path):
    """pretrain.py on the device: fused SGD with the head plan attached, EMA, the deterministic switch -- one short run, then its checkpoint"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "yolo-v1_amd", "pretrain.py"), "--device", "cuda", "--synthetic", "16", "--num-classes", "4", "--image-size", "64",
           "--epochs", "2", "--batch-size", "8", "--num-workers", "0", "--lr", "1e-3", "--label-smoothing", "0.1", "--ema-decay", "0.9", "--deterministic",
           "--seed", "3", "--checkpoint-dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    ck = torch.load(tmp_path / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert ck["epoch"] == 2 and ck["num_classes"] == 4 and ck["image_size"] == 64 and ck["seed"] == 3 and ck["deterministic"] is True
    assert set(ck["ema_state_dict"]) == set(ck["model_state_dict"]) and ck["ema_updates"] == 4
    assert np.isfinite(ck["train_loss"]) and np.isfinite(ck["val_loss"]) and 0.0 <= ck["val_top1"] <= 1.0 and ck["val_top5"] == 1.0
    assert (tmp_path / "yolo_best_top1.pth").is_file()
    assert any(not torch.equal(ck["ema_state_dict"][k], v) for k, v in ck["model_state_dict"].items()), "the average follows the weights, it is not them"
