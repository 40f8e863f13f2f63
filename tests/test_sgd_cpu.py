"""SGD with momentum without a GPU: tests/sgd_ref.py against an fp32 restatement, yolo.optim.SGD on CPU tensors and torch.optim.SGD behind
clip_grad_norm_ against the fp64 recurrence within its propagated bound (five steps fed back, each step judged from the fp32 state it started
from, as tests/test_gpu_optim.py judges its fed-back steps), state_dict exchange with torch.optim.SGD in both directions, the constructor's
errors, the ABI surface of sgd.hip, and train.py --optimizer sgd on the CPU (one epoch, then a resumed one)."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import elementwise_ref as er
import launch_ref as lr
import sgd_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
LR, MAX_NORM = 1e-3, 10.0
SIZES = (1000, 37, 5)


def _grads(sizes, seed, hi):
    """|g| log-uniform in [1e-6, hi] with random sign (hi = 1e3: global norm far above MAX_NORM, the clip is active; 1e-1: below it)"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
        mag = torch.exp(r() * (np.log(hi) - np.log(1e-6)) + np.log(1e-6))
        out.append((mag * torch.where(r() < 0.5, -1.0, 1.0)).float())
    return out


def test_the_entrys_one_minus_dampening_is_torchs():
    """sgd.hip forms (float)(1.0 - (double)(float)dampening), torch's kernels fp32(1 - dampening): one value for the dampenings tested here"""
    for d in (0.0, 0.1):
        assert sr.sgd_constants(LR, 0.9, d, 0.0)["omd"] == er._f32(1.0 - d)


@pytest.mark.parametrize("norm_sq", [None, (10.0 / 0.37) ** 2], ids=["noclip", "clip0.37"])
@pytest.mark.parametrize("first_step", [0, 1])
@pytest.mark.parametrize("h", sr.HYPERS, ids=sr.hyper_id)
def test_fp32_restatement_lies_inside_the_bound(h, first_step, norm_sq):
    """the recurrence in torch fp32, one rounding per operation, 2^18 elements, |g| from 1e-6 to 1e3: every element of p and buf within the bound,
    and the bound within a few unit roundoffs of the value (median relative bound < 1e-6)"""
    (g,) = _grads([1 << 18], 7, 1e3)
    gen = torch.Generator().manual_seed(8)
    p = torch.randn(g.numel(), generator=gen)
    buf = g * (torch.rand(g.numel(), generator=gen) * 2 - 1)
    kw = dict(h, lr=LR, first_step=first_step, norm_sq=norm_sq, max_norm=MAX_NORM)
    got = sr.sgd1_fp32(p, g, buf, **kw)
    refs, bnds = sr.sgd_ref(p, g, buf, **kw)
    fails = []
    for name, gt, rf, bd in zip(("p", "buf"), got, refs, bnds):
        if name == "buf" and h["momentum"] == 0.0:
            assert gt is None and rf is None and bd is None
            continue
        worst = lr.check_values(rf, bd, gt, name, fails, sr.hyper_id(h))
        print(f"{name}: worst |err| / bound {worst:.3f}")
        assert float((bd / rf.abs().clamp_min(1e-300)).median()) < 1e-6
    assert not fails, "\n".join(fails)


def test_sgd_ref_rejects_a_wrong_recurrence():
    """dampening applied to the buffer instead of the gradient lies far outside the bound"""
    (g,) = _grads([4096], 3, 1e3)
    p, buf = torch.randn(4096), g.flip(0).clone()
    kw = dict(lr=LR, momentum=0.9, dampening=0.1, wd=5e-4, nesterov=False, first_step=0, norm_sq=None, max_norm=MAX_NORM)
    refs, bnds = sr.sgd_ref(p, g, buf, **kw)
    gg = g + np.float32(5e-4) * p
    bad = np.float32(0.9) * np.float32(0.9) * buf + gg
    fails = []
    lr.check_values(refs[1], bnds[1], bad, "buf", fails)
    assert fails


def _five_steps(make_opt, clip_and_step, h, hi):
    """five steps on three CPU tensors with fresh gradients each; every step's p and momentum_buffer against sgd_ref of the state the step began with"""
    torch.manual_seed(0)
    ps = [torch.randn(n, requires_grad=True) for n in SIZES]
    opt = make_opt(ps)
    fails = []
    for step in range(5):
        gs = _grads(SIZES, 50 + step, hi)
        before = [(q.detach().clone(), opt.state[q]["momentum_buffer"].clone() if "momentum_buffer" in opt.state[q] else None) for q in ps]
        for q, g in zip(ps, gs):
            q.grad = g.clone()
        norm_sq, clip = clip_and_step(opt, ps)
        assert (er.clip_ref(norm_sq, MAX_NORM) < 1.0) == (hi > 1.0), "the case must clip exactly when it says so"
        for i, (q, g, (p0, b0)) in enumerate(zip(ps, gs, before)):
            assert (b0 is None) == (step == 0 or h["momentum"] == 0.0)
            refs, bnds = sr.sgd_ref(p0, g, b0, lr=LR, first_step=step == 0, norm_sq=norm_sq, max_norm=MAX_NORM, clip=clip, **h)
            lr.check_values(refs[0], bnds[0], q.detach(), "p", fails, f"step {step} tensor {i}")
            assert not torch.equal(q.detach(), p0), "the step must move the parameter"
            if h["momentum"] != 0.0:
                lr.check_values(refs[1], bnds[1], opt.state[q]["momentum_buffer"], "momentum_buffer", fails, f"step {step} tensor {i}")
            else:
                assert "momentum_buffer" not in opt.state[q]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("hi", [1e3, 1e-1], ids=["clip-active", "clip-inactive"])
@pytest.mark.parametrize("h", sr.HYPERS, ids=sr.hyper_id)
def test_yolo_sgd_on_cpu_tensors_five_steps(h, hi):
    from yolo.optim import SGD

    def step(opt, ps):
        acc = torch.zeros((), dtype=torch.float64)
        for q in ps:                                 # the fp64 sum yolo.optim.grad_norm_sq forms for CPU gradients, in its order
            acc += q.grad.double().pow(2).sum()
        opt.step()
        return float(acc), None
    _five_steps(lambda ps: SGD(ps, lr=LR, momentum=h["momentum"], dampening=h["dampening"], weight_decay=h["wd"], nesterov=h["nesterov"],
                               max_grad_norm=MAX_NORM), step, h, hi)


@pytest.mark.parametrize("hi", [1e3, 1e-1], ids=["clip-active", "clip-inactive"])
@pytest.mark.parametrize("h", sr.HYPERS, ids=sr.hyper_id)
def test_torch_sgd_behind_clip_grad_norm_five_steps(h, hi):
    def step(opt, ps):
        g0 = [q.grad.clone() for q in ps]
        total = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)
        # the coefficient as clip_grad_norm_ forms it from its fp32 total: within one fp32 step of clip_ref of that total (it multiplies a
        # reciprocal where the kernels divide), so the reference takes the coefficient that was applied -- checked here, bit for bit
        coef = torch.clamp(MAX_NORM / (total + 1e-6), max=1.0)
        assert all(torch.equal(q.grad, g * coef) for q, g in zip(ps, g0))
        ours = er.clip_ref(float(total.double()) ** 2, MAX_NORM)
        assert abs(float(coef) - ours) <= float(np.spacing(np.float32(ours)))
        opt.step()
        return float(total.double()) ** 2, float(coef)
    _five_steps(lambda ps: torch.optim.SGD(ps, lr=LR, momentum=h["momentum"], dampening=h["dampening"], weight_decay=h["wd"], nesterov=h["nesterov"]),
                step, h, hi)


def test_without_max_grad_norm_the_cpu_step_is_torchs_bit_for_bit():
    from yolo.optim import SGD
    for h in sr.HYPERS:
        kw = dict(lr=LR, momentum=h["momentum"], dampening=h["dampening"], weight_decay=h["wd"], nesterov=h["nesterov"])
        torch.manual_seed(1)
        a = [torch.randn(n, requires_grad=True) for n in SIZES]
        b = [q.detach().clone().requires_grad_(True) for q in a]
        oa, ob = SGD(a, **kw), torch.optim.SGD(b, **kw)
        for step in range(3):
            for q, r, g in zip(a, b, _grads(SIZES, 70 + step, 1e1)):
                q.grad, r.grad = g.clone(), g.clone()
            oa.step()
            ob.step()
        assert all(torch.equal(q, r) for q, r in zip(a, b)), sr.hyper_id(h)


@pytest.mark.parametrize("direction", ["yolo->torch", "torch->yolo"])
def test_state_dict_round_trip_with_torch_sgd(direction):
    """two steps in one optimizer, its state_dict() loaded into the other kind, one more step in both: the same parameters and buffers"""
    from yolo.optim import SGD
    kw = dict(lr=LR, momentum=0.9, dampening=0.1, weight_decay=5e-4)
    kinds = (SGD, torch.optim.SGD) if direction == "yolo->torch" else (torch.optim.SGD, SGD)
    torch.manual_seed(2)
    a = [torch.randn(n, requires_grad=True) for n in SIZES]
    oa = kinds[0](a, **kw)
    for step in range(2):
        for q, g in zip(a, _grads(SIZES, 80 + step, 1e1)):
            q.grad = g
        oa.step()
    b = [q.detach().clone().requires_grad_(True) for q in a]
    ob = kinds[1](b, lr=0.5)                                     # every hyper-parameter comes from the loaded groups
    import copy
    sd = copy.deepcopy(oa.state_dict())                          # load_state_dict keeps the tensors it is given: the two must not share buffers
    assert set(sd["param_groups"][0]) == set(torch.optim.SGD([torch.zeros(1)], lr=0.1).state_dict()["param_groups"][0])
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values()) and len(sd["state"]) == len(SIZES)
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["lr"] == LR and ob.param_groups[0]["momentum"] == 0.9 and ob.param_groups[0]["dampening"] == 0.1
    for q, r, g in zip(a, b, _grads(SIZES, 90, 1e1)):
        q.grad, r.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
    for q, r in zip(a, b):
        assert torch.equal(q, r) and torch.equal(oa.state[q]["momentum_buffer"], ob.state[r]["momentum_buffer"])
    # before the first step neither kind has state
    assert kinds[0]([torch.zeros(3, requires_grad=True)], **kw).state_dict()["state"] == {}


@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_constructor_raises_what_torch_raises(bad):
    from yolo.optim import SGD
    msgs = []
    for kind in (torch.optim.SGD, SGD):
        with pytest.raises(ValueError) as e:
            kind([torch.zeros(3, requires_grad=True)], **{"lr": 0.1, **bad})
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    SGD([torch.zeros(3, requires_grad=True)], lr=0.0, momentum=0.9, nesterov=True, max_grad_norm=10.0)      # legal in both


def test_skip_if_on_the_cpu_updates_nothing():
    from yolo.optim import SGD
    p = torch.randn(100, requires_grad=True)
    opt = SGD([p], lr=0.1, momentum=0.9)
    p.grad = torch.ones(100)
    p0 = p.detach().clone()
    opt.skip_if = torch.tensor(1.0)
    opt.step()
    assert torch.equal(p.detach(), p0) and "momentum_buffer" not in opt.state[p] and opt.skip_if is None
    opt.step()
    assert torch.equal(p.detach(), p0 - 0.1) and torch.equal(opt.state[p]["momentum_buffer"], torch.ones(100))


def test_every_sgd_entry_is_declared_bound_and_called_by_the_gpu_test():
    """every YOLO_API entry sgd.hip defines is in the header, in the binding, and named by tests/test_gpu_sgd.py; the struct mirrors the C layout"""
    import ctypes
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "sgd.hip")) as f:
        entries = set(re.findall(r"YOLO_API int (yolo_\w+)", f.read()))
    assert entries == {"yolo_sgd_step", "yolo_sgd_step_multi", "yolo_sgd_step_multi_bg"}
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_sgd.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
        doc = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "trainer.py:79-95" in doc, f"{name}: the reference lines it stands beside"
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header)
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(yolo_sgd_tensor), ' \
            'offsetof(yolo_sgd_tensor, p), offsetof(yolo_sgd_tensor, g), offsetof(yolo_sgd_tensor, buf), offsetof(yolo_sgd_tensor, p_bf16), offsetof(yolo_sgd_tensor, n));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = _hip.SgdTensor
    assert got == [ctypes.sizeof(T), T.p.offset, T.g.offset, T.buf.offset, T.p_bf16.offset, T.n.offset]


def test_sgd_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call, so they can be exercised without a device (as tests/test_abi.py does for yolo_decode)"""
    import ctypes
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    x = (ctypes.c_float * 64)()
    a = ctypes.addressof(x)
    a += -a % 16
    h = lambda **kw: (kw.get("lr", 1e-3), kw.get("momentum", 0.9), kw.get("dampening", 0.0), kw.get("wd", 0.0), kw.get("nesterov", 0), 0, None, 10.0)
    one = lambda p=a, g=a, buf=a, n=8, pb=None, **kw: L.yolo_sgd_step(p, g, buf, n, *h(**kw), pb, None, None)
    assert one(lr=-1.0) == _hip.E_ARG and "yolo_sgd_step" in L.yolo_hip_last_error().decode()
    assert one(momentum=-0.5) == _hip.E_ARG and one(wd=-1.0) == _hip.E_ARG
    assert one(nesterov=1, momentum=0.0) == _hip.E_ARG and one(nesterov=1, dampening=0.1) == _hip.E_ARG
    assert one(p=None) == _hip.E_ARG and one(g=None) == _hip.E_ARG and one(buf=None) == _hip.E_ARG and one(n=-1) == _hip.E_ARG
    assert one(p=a + 4) == _hip.E_UNSUPPORTED and one(buf=a + 8) == _hip.E_UNSUPPORTED and one(pb=a + 2) == _hip.E_UNSUPPORTED
    assert one(n=0) == 0 and one(n=0, buf=None, momentum=0.0) == 0                      # nothing to launch
    T = _hip.SgdTensor
    ok = (T * 2)(T(a, a, a, None, 0), T(a, a, a, None, 0))
    for fn, extra in ((L.yolo_sgd_step_multi, ()), (L.yolo_sgd_step_multi_bg, (4,))):
        call = lambda tab, count, **kw: fn(tab, count, *h(**kw), None, *extra, None)
        assert call(None, 2) == _hip.E_ARG and call(ok, -1) == _hip.E_ARG and call(ok, 2, lr=-1.0) == _hip.E_ARG
        assert call(ok, 2, nesterov=1, dampening=0.5) == _hip.E_ARG
        assert call((T * 2)(T(a, a, a, None, 0), T(a, None, a, None, 8)), 2) == _hip.E_ARG and "tensor 1" in L.yolo_hip_last_error().decode()
        assert call((T * 2)(T(a, a + 4, a, None, 8), T(a, a, a, None, 0)), 2) == _hip.E_UNSUPPORTED and "tensor 0" in L.yolo_hip_last_error().decode()
        assert call((T * 2)(T(a, a, a, None, 0), T(a, a, a, a + 2, 8)), 2) == _hip.E_UNSUPPORTED and "shadow 1" in L.yolo_hip_last_error().decode()
        assert call(ok, 2) == 0 and call(ok, 0) == 0                                    # empty tensors, empty table: legal, nothing to launch
    for wg in (0, -1, 257):
        assert L.yolo_sgd_step_multi_bg(ok, 2, *h(), None, wg, None) == _hip.E_ARG
    assert L.yolo_sgd_step_multi_bg((T * 49)(*[T(a, a, a, None, 0)] * 49), 49, *h(), None, 4, None) == _hip.E_ARG


def test_train_cli_sgd_on_the_cpu_one_epoch_then_resume(tmp_path):
    """train.py --optimizer sgd --synthetic N --device cpu: torch.optim.SGD with the paper's momentum, a checkpoint whose optimizer state holds the
    momentum buffers, and a resumed second epoch that goes on from them"""
    ck = tmp_path / "ck"
    common = [sys.executable, os.path.join(PKG, "train.py"), "--device", "cpu", "--optimizer", "sgd", "--backbone", "yolov1", "--batch-size", "2",
              "--num-workers", "0", "--synthetic", "2", "--checkpoint-dir", str(ck)]

    def run(extra):
        r = subprocess.run(common + extra, cwd=str(tmp_path), capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, f"{extra}\n--- stdout\n{r.stdout[-2000:]}\n--- stderr\n{r.stderr[-4000:]}"
        assert "done:" in r.stdout
        return torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True, mmap=True)

    st = run(["--epochs", "1"])
    group = st["optimizer_state_dict"]["param_groups"][0]
    assert st["epoch"] == 1 and group["momentum"] == 0.9 and group["weight_decay"] == 5e-4 and group["nesterov"] is False
    state = st["optimizer_state_dict"]["state"]
    assert len(state) == 52 and all(set(s) == {"momentum_buffer"} and bool(torch.isfinite(s["momentum_buffer"]).all()) for s in state.values())
    w1 = {k: v.clone() for k, v in st["model_state_dict"].items() if v.numel() < (1 << 20)}
    del st, state
    (ck / "yolo_best.pth").unlink()                                  # 2 GB each: keep the temporary directory small
    st2 = run(["--epochs", "2", "--resume", str(ck / "yolo_latest.pth")])
    assert st2["epoch"] == 2
    assert any(not torch.equal(st2["model_state_dict"][k], v) for k, v in w1.items())          # the resumed epoch trained
    r = subprocess.run(common[:2] + ["--optimizer", "rmsprop"], capture_output=True, text=True)
    assert r.returncode != 0 and "--optimizer" in r.stderr
