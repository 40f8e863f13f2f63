"""LARS without a GPU: tests/lars_ref.py against its own fp32 restatement and against wrong recurrences, yolo.optim.LARS on CPU tensors against
"trust-scaled gradients into torch.optim.SGD" written out here, adapt=False against yolo.optim.SGD bit for bit, the constructor's errors, skip_if,
the state_dict round trip, lars_param_groups, the ABI surface of lars.hip and the host-side refusals of its entries, pretrain.py / train.py
--optimizer lars on the CPU, and the learning-rate warm-up of both epoch loops seen through an optimizer step pre-hook."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import elementwise_ref as er
import lars_ref as lf
import launch_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")
LR, MAX_NORM, ETA, EPS = 1e-2, 10.0, 1e-3, 1e-8
SIZES = (1000, 37, 5)
ENTRIES = {"yolo_lars_norm_slots", "yolo_lars_norms_multi", "yolo_lars_step", "yolo_lars_step_multi", "yolo_lars_step_multi_bg"}


def _grads(sizes, seed, hi):
    """|g| log-uniform in [1e-3, hi] with random sign (hi = 1e3: global norm far above MAX_NORM, the clip is active; 1e-1: below it)"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
        mag = torch.exp(r() * (np.log(hi) - np.log(1e-3)) + np.log(1e-3))
        out.append((mag * torch.where(r() < 0.5, -1.0, 1.0)).float())
    return out


def _sums(p, g):
    return float(p.double().pow(2).sum()), float(g.double().pow(2).sum())


# ---- the reference itself ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1027, 65535, 65536, 65537, 2 * 65536 + 5])
def test_norm_order_restatement_is_within_its_derived_bound(n):
    """the order restatement against math.fsum of the exact squares: one fp32 rounding per square, one per pair sum, all terms positive -> 2^-22
    relative (the fp64 accumulation adds below 2^-40)"""
    rng = np.random.default_rng(n)
    x = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    got, exact = lf.norm_order_ref(x), lf.exact_sumsq(x)
    assert abs(got - exact) <= 2.0 ** -22 * exact
    if n:
        assert got != 0.0
    # the order matters at the last bits: a plain fp64 dot is not the restatement for the large sizes (else this file would restate nothing)
    assert lf.g_total_ref([1.0, 2.0, 3.0, 4.0, 5.0, 0.5]) == 6.5


def test_norm_order_restatement_groups_like_the_kernel():
    """a case whose value depends on the grouping: (1 + 2^-24-ish) squares where fp32 pair sums round differently from a left-to-right fp32 sum"""
    x = np.array([4096.0, 1.0, 1.0, 1.0, 3.0], dtype=np.float32)
    # float4: fp32(4096^2 + 1) = 16777216 (the 1 is lost), fp32(1 + 1) = 2 -> 16777218; tail: + 9
    assert lf.norm_order_ref(x) == 16777216.0 + 2.0 + 9.0
    assert lf.exact_sumsq(x) == 16777216.0 + 3.0 + 9.0


@pytest.mark.parametrize("norm_sq", [None, (10.0 / 0.37) ** 2], ids=["noclip", "clip0.37"])
@pytest.mark.parametrize("first_step", [0, 1])
@pytest.mark.parametrize("h", lf.HYPERS, ids=lf.hyper_id)
def test_fp32_restatement_lies_inside_the_bound(h, first_step, norm_sq):
    (g,) = _grads([1 << 16], 7, 1e3)
    gen = torch.Generator().manual_seed(8)
    p = torch.randn(g.numel(), generator=gen)
    buf = g * (torch.rand(g.numel(), generator=gen) * 2 - 1) * 1e-3
    kw = dict(h, lr=LR, eta=ETA, eps=EPS, first_step=first_step, norm_sq=norm_sq, max_norm=MAX_NORM, norms=_sums(p, g))
    got = lf.lars1_fp32(p, g, buf, **kw)
    refs, bnds = lf.lars_ref(p, g, buf, **kw)
    fails = []
    for name, gt, rf, bd in zip(("p", "buf"), got, refs, bnds):
        if name == "buf" and h["momentum"] == 0.0:
            assert gt is None and rf is None and bd is None
            continue
        worst = lr.check_values(rf, bd, gt, name, fails, lf.hyper_id(h))
        print(f"{name}: worst |err| / bound {worst:.3f}")
        assert float((bd / rf.abs().clamp_min(1e-300)).median()) < 2e-6
    assert not fails, "\n".join(fails)


def test_trust_ref_cases():
    kw = dict(clip=1.0, eta=ETA, wd=5e-4, eps=EPS)
    assert lf.trust_ref(0.0, 4.0, **kw) == 1.0 and lf.trust_ref(4.0, 0.0, **kw) == 1.0 and lf.trust_ref(4.0, 9.0, adapt=False, **kw) == 1.0
    want = er._f32(ETA) * 2.0 / (3.0 + er._f32(5e-4) * 2.0 + er._f32(EPS))
    assert lf.trust_ref(4.0, 9.0, **kw) == er._f32(want)
    assert lf.trust_ref(4.0, 9.0, clip=0.5, eta=ETA, wd=0.0, eps=0.0) == er._f32(er._f32(ETA) * 2.0 / 1.5)


@pytest.mark.parametrize("wrong", ["trust-before-decay", "lr-inside-momentum"])
def test_lars_ref_rejects_a_wrong_recurrence(wrong):
    (g,) = _grads([4096], 3, 1e1)
    p, buf = torch.randn(4096), g.flip(0).clone() * 1e-3
    norms = _sums(p, g)
    kw = dict(lr=LR, momentum=0.9, wd=5e-2, eta=ETA, eps=EPS, first_step=0, norm_sq=None, max_norm=MAX_NORM, norms=norms)
    refs, bnds = lf.lars_ref(p, g, buf, **kw)
    trust = np.float32(lf.trust_ref(*norms, clip=1.0, eta=ETA, wd=5e-2, eps=EPS))
    f = np.float32
    if wrong == "trust-before-decay":
        gg = g * trust + f(5e-2) * p
        bad_buf = f(0.9) * buf + gg
        bad_p = p - f(LR) * bad_buf
    else:
        gg = (g + f(5e-2) * p) * trust
        bad_buf = f(0.9) * buf + f(LR) * gg
        bad_p = p - bad_buf
    fails = []
    lr.check_values(refs[1], bnds[1], bad_buf, "buf", fails)
    assert fails
    fails = []
    lr.check_values(refs[0], bnds[0], bad_p, "p", fails)
    assert fails


# ---- yolo.optim.LARS on CPU tensors --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hi", [1e3, 1e-1], ids=["clip-active", "clip-inactive"])
@pytest.mark.parametrize("h", [h for h in lf.HYPERS if h["adapt"]], ids=lf.hyper_id)
def test_lars_on_cpu_tensors_five_steps_against_trust_scaled_sgd(h, hi):
    """five steps on three CPU tensors: the same gradients, clipped, regularised and scaled by the trust ratio HERE (in double, independently of the
    optimizer's code), go into torch.optim.SGD(weight_decay=0); every step's p and momentum_buffer of both lie within lars_ref's bound of the state
    the step began with"""
    from yolo.optim import LARS
    torch.manual_seed(0)
    ps = [torch.randn(n, requires_grad=True) for n in SIZES]
    qs = [q.detach().clone().requires_grad_(True) for q in ps]
    opt = LARS(ps, lr=LR, momentum=h["momentum"], weight_decay=h["wd"], eta=ETA, eps=EPS, max_grad_norm=MAX_NORM)
    sgd = torch.optim.SGD(qs, lr=LR, momentum=h["momentum"], weight_decay=0.0)
    fails = []
    for step in range(5):
        gs = _grads(SIZES, 50 + step, hi)
        before = [(q.detach().clone(), opt.state[q]["momentum_buffer"].clone() if "momentum_buffer" in opt.state[q] else None) for q in ps]
        norm_sq = float(sum(g.double().pow(2).sum() for g in gs))
        clip = er.clip_ref(norm_sq, MAX_NORM)
        assert (clip < 1.0) == (hi > 1.0), "the case must clip exactly when it says so"
        for q, r, g in zip(ps, qs, gs):
            q.grad = g.clone()
            wn, gn = float(r.detach().double().norm()), clip * float(g.double().norm())
            trust = ETA * wn / (gn + h["wd"] * wn + EPS)
            r.grad = ((g.double() * clip + h["wd"] * r.detach().double()) * trust).float()
        opt.step()
        sgd.step()
        for i, (q, r, g, (p0, b0)) in enumerate(zip(ps, qs, gs, before)):
            refs, bnds = lf.lars_ref(p0, g, b0, lr=LR, momentum=h["momentum"], wd=h["wd"], eta=ETA, eps=EPS, first_step=step == 0, norm_sq=norm_sq,
                                     max_norm=MAX_NORM, norms=_sums(p0, g))
            lr.check_values(refs[0], bnds[0], q.detach(), "p", fails, f"step {step} tensor {i}")
            assert not torch.equal(q.detach(), p0), "the step must move the parameter"
            # the independent path starts every step from ITS OWN state, which follows ours within rounding: a few bounds of slack over five steps
            assert float((r.detach().double() - q.detach().double()).abs().max()) <= 8 * (step + 1) * float(bnds[0].max())
            if h["momentum"] != 0.0:
                lr.check_values(refs[1], bnds[1], opt.state[q]["momentum_buffer"], "momentum_buffer", fails, f"step {step} tensor {i}")
            else:
                assert "momentum_buffer" not in opt.state[q]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("max_norm", [None, MAX_NORM])
def test_adapt_false_is_yolo_sgd_bit_for_bit(max_norm):
    from yolo.optim import LARS, SGD
    for momentum in (0.0, 0.9):
        for wd in (0.0, 5e-4):
            torch.manual_seed(1)
            a = [torch.randn(n, requires_grad=True) for n in SIZES]
            b = [q.detach().clone().requires_grad_(True) for q in a]
            oa = LARS([{"params": a, "adapt": False}], lr=LR, momentum=momentum, weight_decay=wd, eta=123.0, eps=0.5, max_grad_norm=max_norm)
            ob = SGD(b, lr=LR, momentum=momentum, weight_decay=wd, max_grad_norm=max_norm)
            for step in range(3):
                for q, r, g in zip(a, b, _grads(SIZES, 70 + step, 1e3)):
                    q.grad, r.grad = g.clone(), g.clone()
                oa.step()
                ob.step()
            assert all(torch.equal(q, r) for q, r in zip(a, b)), (momentum, wd)
            if momentum:
                assert all(torch.equal(oa.state[q]["momentum_buffer"], ob.state[r]["momentum_buffer"]) for q, r in zip(a, b))


@pytest.mark.parametrize("bad", [dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(eta=-1e-3), dict(eps=-1e-8)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_constructor_errors(bad):
    from yolo.optim import LARS
    with pytest.raises(ValueError):
        LARS([torch.zeros(3, requires_grad=True)], **{"lr": 0.1, **bad})
    LARS([torch.zeros(3, requires_grad=True)], lr=0.0, momentum=0.0, weight_decay=0.0, eta=0.0, eps=0.0, max_grad_norm=10.0)      # legal


def test_skip_if_on_the_cpu_updates_nothing():
    from yolo.optim import LARS
    p = torch.randn(100, requires_grad=True)
    opt = LARS([p], lr=0.1, momentum=0.9)
    p.grad = torch.ones(100)
    p0 = p.detach().clone()
    opt.skip_if = torch.tensor(1.0)
    opt.step()
    assert torch.equal(p.detach(), p0) and "momentum_buffer" not in opt.state[p] and opt.skip_if is None and float(opt.last_skip) == 1.0
    opt.step()
    assert not torch.equal(p.detach(), p0) and "momentum_buffer" in opt.state[p] and opt.last_skip is None


def test_state_dict_round_trip_through_a_fresh_lars():
    import copy
    from yolo.optim import LARS
    torch.manual_seed(2)
    a = [torch.randn(n, requires_grad=True) for n in SIZES]
    groups = lambda ps: [{"params": ps[:2], "weight_decay": 5e-4}, {"params": ps[2:], "weight_decay": 0.0, "adapt": False}]
    oa = LARS(groups(a), lr=LR, momentum=0.9, eta=2e-3, eps=1e-9, max_grad_norm=MAX_NORM)
    for step in range(2):
        for q, g in zip(a, _grads(SIZES, 80 + step, 1e1)):
            q.grad = g
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values()) and len(sd["state"]) == len(SIZES)
    assert [g["adapt"] for g in sd["param_groups"]] == [True, False]
    b = [q.detach().clone().requires_grad_(True) for q in a]
    ob = LARS(groups(b), lr=0.5, max_grad_norm=MAX_NORM)                    # every hyper-parameter comes from the loaded groups
    ob.load_state_dict(sd)
    g0 = ob.param_groups[0]
    assert (g0["lr"], g0["momentum"], g0["eta"], g0["eps"], g0["weight_decay"]) == (LR, 0.9, 2e-3, 1e-9, 5e-4) and ob.param_groups[1]["adapt"] is False
    for q, r, g in zip(a, b, _grads(SIZES, 90, 1e1)):
        q.grad, r.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
    for q, r in zip(a, b):
        assert torch.equal(q, r) and torch.equal(oa.state[q]["momentum_buffer"], ob.state[r]["momentum_buffer"])
    assert LARS([torch.zeros(3, requires_grad=True)], lr=0.1).state_dict()["state"] == {}


def test_lars_param_groups_split_by_ndim():
    from yolo import YOLOv1Classifier
    from yolo.optim import LARS, lars_param_groups
    model = YOLOv1Classifier(4, batch_norm=True)
    groups = lars_param_groups(model, 5e-4)
    assert len(groups) == 2
    small = {id(p) for p in model.parameters() if p.ndim <= 1}
    assert {id(p) for p in groups[1]["params"]} == small and small and all(p.ndim > 1 for p in groups[0]["params"])
    assert len(groups[0]["params"]) + len(groups[1]["params"]) == len(list(model.parameters()))
    assert groups[0]["weight_decay"] == 5e-4 and "adapt" not in groups[0]
    assert groups[1]["weight_decay"] == 0.0 and groups[1]["adapt"] is False
    opt = LARS(groups, lr=0.1)
    assert [g["adapt"] for g in opt.param_groups] == [True, False]


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------------------------

def test_every_lars_entry_is_declared_bound_and_called_by_the_gpu_test():
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "lars.hip")) as f:
        entries = set(re.findall(r"YOLO_API int (yolo_\w+)", f.read()))
    assert entries == ENTRIES
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_lars.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
        doc = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "trainer.py:79-95" in doc, f"{name}: the reference lines it stands beside"
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header)
    fields = ["p", "g", "buf", "p_bf16", "norms", "n", "adapt"]
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(){printf("%zu", sizeof(yolo_lars_tensor));' + \
            "".join(f'printf(" %zu", offsetof(yolo_lars_tensor, {k}));' for k in fields) + 'printf("\\n");return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = _hip.LarsTensor
    assert [k for k, _ in T._fields_] == fields
    assert got == [ctypes.sizeof(T)] + [getattr(T, k).offset for k in fields]


def _lib():
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    return _hip.lib()


def test_lars_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call: made-up addresses, never dereferenced"""
    from yolo import _hip
    L = _lib()
    err = lambda: L.yolo_hip_last_error().decode(errors="replace")
    a, nrm = 0x1000000, 0x2000000
    # ---- yolo_lars_norm_slots
    n3 = (ctypes.c_long * 3)(0, 65536, 65537)
    out = ctypes.c_long(-1)
    assert L.yolo_lars_norm_slots(n3, 3, ctypes.byref(out)) == 0 and out.value == 2 * (0 + 1 + 2)
    assert L.yolo_lars_norm_slots(n3, 0, ctypes.byref(out)) == 0 and out.value == 0
    assert L.yolo_lars_norm_slots(None, 3, ctypes.byref(out)) == _hip.E_ARG and L.yolo_lars_norm_slots(n3, 3, None) == _hip.E_ARG
    assert L.yolo_lars_norm_slots(n3, -1, ctypes.byref(out)) == _hip.E_ARG
    assert L.yolo_lars_norm_slots((ctypes.c_long * 2)(4, -1), 2, ctypes.byref(out)) == _hip.E_ARG and "tensor 1" in err()
    # ---- yolo_lars_norms_multi
    V = lambda *v: (ctypes.c_void_p * len(v))(*v)
    N = lambda *v: (ctypes.c_long * len(v))(*v)
    norms = lambda p=V(a, a), g=V(a, a), n=N(8, 8), count=2, scratch=a, slots=4, out=nrm, tot=nrm + 64: \
        L.yolo_lars_norms_multi(p, g, n, count, scratch, slots, out, tot, None)
    assert norms(p=None) == _hip.E_ARG and norms(g=None) == _hip.E_ARG and norms(n=None) == _hip.E_ARG and norms(out=None) == _hip.E_ARG
    assert norms(count=-1) == _hip.E_ARG and norms(slots=-1) == _hip.E_ARG and "yolo_lars_norms_multi" in err()
    assert norms(p=V(a, None)) == _hip.E_ARG and "tensor 1" in err()
    assert norms(g=V(None, a)) == _hip.E_ARG and "tensor 0" in err()
    assert norms(n=N(8, -2)) == _hip.E_ARG and "tensor 1" in err()
    assert norms(p=V(a + 4, a)) == _hip.E_UNSUPPORTED and "tensor 0" in err() and norms(g=V(a, a + 8)) == _hip.E_UNSUPPORTED and "tensor 1" in err()
    assert norms(out=nrm + 4) == _hip.E_UNSUPPORTED and norms(tot=nrm + 4) == _hip.E_UNSUPPORTED
    assert norms(slots=3) == _hip.E_ARG and "scratch" in err() and norms(scratch=None) == _hip.E_ARG and norms(scratch=a + 4) == _hip.E_ARG
    assert norms(count=0, tot=None) == 0                                          # nothing to store, nothing to launch
    # ---- the step entries
    h = lambda **kw: (kw.get("lr", 1e-3), kw.get("momentum", 0.9), kw.get("wd", 0.0), kw.get("eta", 1e-3), kw.get("eps", 1e-8), 0, None, 10.0)
    one = lambda p=a, g=a, buf=a, n=8, nr=nrm, adapt=1, pb=None, **kw: L.yolo_lars_step(p, g, buf, n, nr, adapt, *h(**kw), pb, None, None)
    assert one(lr=-1.0) == _hip.E_ARG and "yolo_lars_step" in err()
    assert one(momentum=-0.5) == _hip.E_ARG and one(wd=-1.0) == _hip.E_ARG and one(eta=-1.0) == _hip.E_ARG and one(eps=-1.0) == _hip.E_ARG
    assert one(p=None) == _hip.E_ARG and one(g=None) == _hip.E_ARG and one(buf=None) == _hip.E_ARG and one(n=-1) == _hip.E_ARG
    assert one(nr=None) == _hip.E_ARG and "norms" in err()
    assert one(p=a + 4) == _hip.E_UNSUPPORTED and one(buf=a + 8) == _hip.E_UNSUPPORTED and one(pb=a + 2) == _hip.E_UNSUPPORTED
    assert one(nr=nrm + 4) == _hip.E_UNSUPPORTED
    assert one(n=0) == 0 and one(n=0, buf=None, momentum=0.0) == 0 and one(n=0, nr=None, adapt=0) == 0          # nothing to launch
    T = _hip.LarsTensor
    ok = (T * 2)(T(a, a, a, None, nrm, 0, 1), T(a, a, a, None, None, 0, 0))
    for fn, extra in ((L.yolo_lars_step_multi, ()), (L.yolo_lars_step_multi_bg, (4,))):
        call = lambda tab, count, **kw: fn(tab, count, *h(**kw), None, *extra, None)
        assert call(None, 2) == _hip.E_ARG and call(ok, -1) == _hip.E_ARG and call(ok, 2, lr=-1.0) == _hip.E_ARG
        assert call(ok, 2, eta=-1.0) == _hip.E_ARG and call(ok, 2, eps=-1.0) == _hip.E_ARG
        assert call((T * 2)(T(a, a, a, None, nrm, 0, 1), T(a, None, a, None, nrm, 8, 1)), 2) == _hip.E_ARG and "tensor 1" in err()
        assert call((T * 2)(T(a, a, a, None, nrm, 0, 1), T(a, a, a, None, None, 8, 1)), 2) == _hip.E_ARG and "tensor 1" in err()
        assert call((T * 2)(T(a, a + 4, a, None, nrm, 8, 1), T(a, a, a, None, nrm, 0, 1)), 2) == _hip.E_UNSUPPORTED and "tensor 0" in err()
        assert call((T * 2)(T(a, a, a, None, nrm, 0, 1), T(a, a, a, a + 2, nrm, 8, 1)), 2) == _hip.E_UNSUPPORTED and "shadow 1" in err()
        assert call(ok, 2) == 0 and call(ok, 0) == 0                                # empty tensors, empty table: legal, nothing to launch
    for wg in (0, -1, 257):
        assert L.yolo_lars_step_multi_bg(ok, 2, *h(), None, wg, None) == _hip.E_ARG
    assert L.yolo_lars_step_multi_bg((T * 49)(*[T(a, a, a, None, nrm, 0, 1)] * 49), 49, *h(), None, 4, None) == _hip.E_ARG


NULL, NEGATIVE, MISALIGNED = "null pointer", "negative size", "pointer + 4"


@pytest.mark.parametrize("entry", ["yolo_lars_norms_multi", "yolo_lars_step_multi"])
def test_a_bad_tensor_behind_the_first_launch_refuses_the_whole_call(entry):
    """a 100-tensor table is three launches (YOLO_MT_MAX = 48): a bad gradient at index 48 or 99 refuses the call before the first of them"""
    from yolo import _hip
    L = _lib()
    COUNT = 100
    want = {NULL: _hip.E_ARG, NEGATIVE: _hip.E_ARG, MISALIGNED: _hip.E_UNSUPPORTED}
    for where in (48, 99):
        for bad, code in want.items():
            rows = []
            for i in range(COUNT):
                p, g, b = (0x1000000 * (k + 1) + 256 * i for k in range(3))
                spoil = bad if i == where else None
                rows.append((p, None if spoil == NULL else g + 4 if spoil == MISALIGNED else g, b, -1 if spoil == NEGATIVE else 16))
            if entry == "yolo_lars_norms_multi":
                rc = L.yolo_lars_norms_multi((ctypes.c_void_p * COUNT)(*[r[0] for r in rows]), (ctypes.c_void_p * COUNT)(*[r[1] for r in rows]),
                                             (ctypes.c_long * COUNT)(*[r[3] for r in rows]), COUNT, 0xA000000, 1000, 0xB000000, 0xC000000, None)
            else:
                tab = (_hip.LarsTensor * COUNT)(*[_hip.LarsTensor(p, g, b, None, 0xB000000 + 16 * i, n, 1) for i, (p, g, b, n) in enumerate(rows)])
                rc = L.yolo_lars_step_multi(tab, COUNT, 0.1, 0.9, 0.0, 1e-3, 1e-8, 0, None, 0.0, None, None)
            msg = L.yolo_hip_last_error().decode(errors="replace")
            assert rc == code, f"{entry}: {bad} at {where}: code {rc} ({msg})"
            assert entry in msg and re.search(rf"\b{where}\b", msg), f"{entry}: {bad} at {where}: {msg}"


# ---- the command-line tools ----------------------------------------------------------------------------------------------------------------------------

def _run(args, timeout=900, ok=True):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, f"{args}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def test_pretrain_cli_lars_on_the_cpu_one_epoch_then_resume(tmp_path):
    ck = tmp_path / "ck"
    common = [os.path.join(PKG, "pretrain.py"), "--device", "cpu", "--synthetic", "8", "--num-classes", "4", "--image-size", "64", "--batch-size", "2",
              "--num-workers", "0", "--optimizer", "lars", "--warmup-steps", "3", "--batch-norm", "--checkpoint-dir", str(ck)]
    r = _run(common + ["--epochs", "1"])
    assert "done:" in r.stdout
    st = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    groups = st["optimizer_state_dict"]["param_groups"]
    assert st["epoch"] == 1 and len(groups) == 2
    assert groups[0]["adapt"] is True and groups[0]["weight_decay"] == 5e-4 and groups[0]["eta"] == 1e-3 and groups[0]["momentum"] == 0.9
    assert groups[1]["adapt"] is False and groups[1]["weight_decay"] == 0.0
    assert groups[0]["lr"] == 1e-2 and groups[1]["lr"] == 1e-2, "the checkpoint holds the scheduled rate, not a warmed one"
    state = st["optimizer_state_dict"]["state"]
    n_params = len(groups[0]["params"]) + len(groups[1]["params"])
    assert len(state) == n_params and all(set(s) == {"momentum_buffer"} and bool(torch.isfinite(s["momentum_buffer"]).all()) for s in state.values())
    w1 = {k: v.clone() for k, v in st["model_state_dict"].items()}
    r = _run(common + ["--epochs", "2", "--resume", str(ck / "yolo_latest.pth")])
    st2 = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert st2["epoch"] == 2 and any(not torch.equal(st2["model_state_dict"][k], v) for k, v in w1.items())
    assert all(bool(torch.isfinite(v).all()) for v in st2["model_state_dict"].values() if v.is_floating_point())


@pytest.mark.parametrize("cli", ["train.py", "pretrain.py"])
def test_lars_with_nesterov_is_an_argparse_error(cli):
    r = _run([os.path.join(PKG, cli), "--device", "cpu", "--optimizer", "lars", "--nesterov", "--synthetic", "2"], ok=False)
    assert r.returncode == 2 and "--nesterov" in r.stderr


# ---- the warm-up, through both epoch loops -------------------------------------------------------------------------------------------------------------

class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(12, 4)
        self.gain = torch.nn.Parameter(torch.ones(4))

    def forward(self, x):
        return self.fc(x.flatten(1)) * self.gain


def _criterion(out, target):
    loss = (out - target).pow(2).mean()
    return loss, {k: float(loss.detach()) for k in ("total", "coord", "conf_obj", "conf_noobj", "class", "top1", "top5")}


def _epochs(loop, warmup_steps, accum, tmp_path, batches=4):
    """two epochs of `loop` on a tiny model, the second as a resumed run (a fresh call with start_epoch=2, the optimizer and scheduler reloaded from
    their state): -> [(learning rates the step pre-hook saw, one per group)] per optimizer step, the rates the scheduler held per epoch"""
    from yolo.optim import LARS, lars_param_groups
    from yolo.training import classify, trainer
    mod = {"detector": trainer, "classifier": classify}[loop]
    torch.manual_seed(0)
    data = [(torch.randn(2, 3, 2, 2), torch.randn(2, 4)) for _ in range(batches)]
    seen, scheduled = [], []

    def build():
        model = _Tiny()
        opt = LARS(lars_param_groups(model, 5e-4), lr=0.5, momentum=0.9, max_grad_norm=10.0)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1)
        opt.register_step_pre_hook(lambda o, a, k: seen.append(tuple(g["lr"] for g in o.param_groups)))
        return model, opt, sch

    extra = {}
    if warmup_steps:
        extra["warmup_steps"] = warmup_steps
    if accum > 1:
        extra["accum_steps"] = accum
    model, opt, sch = build()
    scheduled.append(opt.param_groups[0]["lr"])
    mod.train(model, data, data[:1], _criterion, opt, sch, "cpu", 1, tmp_path, save_frequency=100, start_epoch=1, **extra)
    state = (model.state_dict(), opt.state_dict(), sch.state_dict())
    model, opt, sch = build()                                                   # the resumed process
    model.load_state_dict(state[0])
    opt.load_state_dict(state[1])
    sch.load_state_dict(state[2])
    scheduled.append(opt.param_groups[0]["lr"])
    mod.train(model, data, data[:1], _criterion, opt, sch, "cpu", 2, tmp_path, save_frequency=100, start_epoch=2, **extra)
    return seen, scheduled


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("loop", ["detector", "classifier"])
def test_warmup_scales_the_scheduled_rate_and_continues_after_a_resume(loop, accum, tmp_path):
    """4 optimizer steps per epoch (with accumulation: 8 batches), N = 6: the warm-up ends inside the resumed epoch, whose scheduled rate
    MultiStepLR has already cut by 10 -- the multiplier applies on top of it, for every group, and the scheduler never sees a warmed rate"""
    per_epoch, N = 4, 6
    seen, scheduled = _epochs(loop, N, accum, tmp_path, batches=4 * accum)
    assert scheduled == [0.5, pytest.approx(0.05)] and len(seen) == 2 * per_epoch
    for k, rates in enumerate(seen):
        base = scheduled[k // per_epoch]
        want = base * (k + 1) / N if k < N else base
        assert rates == (pytest.approx(want, rel=1e-12), pytest.approx(want, rel=1e-12)), (k, rates, want)
    assert seen[N - 1][0] == pytest.approx(scheduled[1], rel=1e-12), "the last warmed step runs at the scheduled rate"
    assert all(r[0] == scheduled[1] for r in seen[N:]) and len(seen[N:]) == 2, "behind the warm-up the hook sees the scheduler's own value"
    assert seen[0][0] < seen[1][0] and seen[per_epoch][0] < scheduled[1]


@pytest.mark.parametrize("loop", ["detector", "classifier"])
def test_without_warmup_the_hook_sees_only_scheduler_values(loop, tmp_path):
    seen, scheduled = _epochs(loop, 0, 1, tmp_path)
    assert [r[0] for r in seen] == [scheduled[0]] * 4 + [scheduled[1]] * 4 and all(r[0] == r[1] for r in seen)
