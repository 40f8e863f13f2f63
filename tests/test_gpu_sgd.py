"""The three SGD entries of csrc/sgd.hip, called through the C ABI as tests/test_gpu_optim.py calls the Adam entries, against tests/sgd_ref.py:
every element of p and of the momentum buffer within the bound propagated through the fp32 recurrence, the bf16 shadow equal to the rounding of
the p the kernel stored, every written buffer between guard bands of a NaN pattern, the gradient untouched.  The kernels write every a * b + c
as an explicit fused multiply-add with contraction otherwise off, so the single, multi-tensor and background forms must agree BIT FOR BIT: that is
asserted in every case (the Adam entries only report it).  Gradients have 1e-6 <= |g| <= 1e3, as in the Adam tests.  The last test runs
yolo.optim.SGD on the YOLOv1 model with the Linear layers' update on the second stream."""

import ctypes

import numpy as np
import pytest
import torch

import elementwise_ref as er
import launch_ref as lr
import sgd_ref as sr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LR, MAX_NORM = 1e-3, 10.0
PAPER = dict(momentum=0.9, dampening=0.0, nesterov=False, wd=5e-4)
Guarded = er.Guarded
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1027, 8191, 8192, 8193, 16384 + 1, 3 * 8192 + 4232, 65535, 65536, 65537]      # the Adam tests' grid
ENTRIES = [("single", 0), ("multi", 0), ("bg", 1), ("bg", 128)]

_BELOW = float(np.nextafter(np.float32(10.0), np.float32(0.0)))
_BELOW2 = float(np.nextafter(np.float32(_BELOW), np.float32(0.0)))
NORMS = {"null": None, "small": 1.0, "at": 100.0, "at+3ulp": float(np.nextafter(np.nextafter(np.nextafter(100.0, 200.0), 200.0), 200.0)),
         "at-3ulp": float(np.nextafter(np.nextafter(np.nextafter(100.0, 0.0), 0.0), 0.0)), "c==1": _BELOW ** 2, "c>1": _BELOW2 ** 2,
         "0.37": (10.0 / 0.37) ** 2}                                                                                # test_gpu_optim.py's table


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


def _inputs(sizes, seed):
    """per tensor p, g, buf fp32 on the device: |g| log-uniform in [1e-6, 1e3] with random sign, buf a previous state of that scale"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in sizes:
        r = lambda: torch.rand(n, generator=gen, dtype=torch.float64, device="cuda")
        mag = torch.exp(r() * (np.log(1e3) - np.log(1e-6)) + np.log(1e-6))
        g = (mag * torch.where(r() < 0.5, -1.0, 1.0)).float()
        buf = (mag * (r() * 2 - 1)).float()
        p = torch.randn(n, generator=gen, dtype=torch.float32, device="cuda")
        out.append((p, g, buf))
    return out


def _gbuf(g):
    """gradient (read only) between guard bands, with a valid pointer even when empty"""
    G = Guarded(g)
    t = G.t
    t._base_ptr = G.ptr
    t._keep = G
    return t


def _run(entry, wg, bufs, h, first, norm, skip):
    """one pass over bufs = [(P, g, B, PB or None)] (Guarded, g from _gbuf) through one entry; the return code must be 0"""
    from yolo._hip import SgdTensor
    L, st = _lib(), _stream()
    nptr = ctypes.c_void_p(norm.data_ptr()) if norm is not None else None
    sptr = ctypes.c_void_p(skip.data_ptr()) if skip is not None else None
    hy = (LR, h["momentum"], h["dampening"], h["wd"], int(h["nesterov"]), int(first), nptr, MAX_NORM)
    if entry == "single":
        for P, g, B, PB in bufs:
            rc = L.yolo_sgd_step(P.ptr, g._base_ptr, B.ptr, P.n, *hy, PB.ptr if PB else None, sptr, st)
            assert rc == 0, _last_error()
        return
    tab = (SgdTensor * len(bufs))(*[SgdTensor(P.ptr, g._base_ptr, B.ptr, PB.ptr if PB else None, P.n) for P, g, B, PB in bufs])
    if entry == "multi":
        rc = L.yolo_sgd_step_multi(tab, len(bufs), *hy, sptr, st)
    else:
        rc = L.yolo_sgd_step_multi_bg(tab, len(bufs), *hy, sptr, wg, st)
    assert rc == 0, _last_error()


def _judge(tag, bufs, starts, h, first, norm_sq, fails):
    """bufs after one pass that began at starts = [(p0, g0, b0)]: values within the bound, shadows, guard bands -> worst |err| / bound"""
    worst = 0.0
    for i, ((P, g, B, PB), (p0, g0, b0)) in enumerate(zip(bufs, starts)):
        where = f"{tag}: tensor {i} (n={P.n})"
        for X, name in ((P, "p"), (B, "buf"), (PB, "shadow")):
            if X is not None and not X.guards_ok():
                fails.append(f"{where}: guard band of {name} overwritten")
        if not P.n:
            continue
        (rp, rb), (bp, bb) = sr.sgd_ref(p0, g0, b0, lr=LR, first_step=first, norm_sq=norm_sq, max_norm=MAX_NORM, **h)
        worst = max(worst, lr.check_values(rp, bp, P.t, "p", fails, where))
        if rb is not None:
            worst = max(worst, lr.check_values(rb, bb, B.t, "momentum_buffer", fails, where))
        elif not torch.equal(B.t.view(torch.int32), b0.view(torch.int32)):
            fails.append(f"{where}: momentum == 0 but buf was written")
        if PB is not None and not torch.equal(PB.t.view(torch.int16), sr.bf16_bits(P.t)):
            fails.append(f"{where}: bf16 shadow != bf16(p)")
    return worst


def _check_case(sizes, shadow, h, first, norm_sq, seed, entries=ENTRIES, skip_zero=False, what=""):
    """all entries on the same inputs: each within the reference's bound on its own, and all of them the same bits"""
    ins = _inputs(sizes, seed)
    norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda") if norm_sq is not None else None
    gs = [_gbuf(g) for _, g, _ in ins]
    skip = torch.zeros(1, device="cuda") if skip_zero else None
    fails, results = [], {}
    for entry, wg in entries:
        if entry == "bg" and len(sizes) > 48:
            continue
        tag = f"{what} {entry}" + (f"[{wg}]" if entry == "bg" else "")
        bufs = [(Guarded(p), g, Guarded(b), Guarded(torch.zeros(p.numel(), dtype=BF, device="cuda"), BF) if sh else None)
                for (p, _, b), g, sh in zip(ins, gs, shadow)]
        _run(entry, wg, bufs, h, first, norm, skip)
        torch.cuda.synchronize()
        worst = _judge(tag, bufs, ins, h, first, norm_sq, fails)
        results[(entry, wg)] = [torch.cat([b[0].t, b[2].t]).view(torch.int32) for b in bufs]
        print(f"{tag}: worst |err| / bound {worst:.3f}")
    for (_, g, _), G in zip(ins, gs):
        if not torch.equal(g, G) or not G._keep.guards_ok():
            fails.append(f"{what}: a gradient was written")
    keys = list(results)
    for k in keys[1:]:
        if not all(torch.equal(a, b) for a, b in zip(results[keys[0]], results[k])):
            fails.append(f"{what}: {k} and {keys[0]} differ in some bits")
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("first", [0, 1])
def test_all_sizes_one_table(first):
    """every edge size in one table (the empty tensor first), shadow on every second tensor, clipped: chunk boundaries +-1, a partial chunk at
    beg > 0 (16385, 3*8192+4232), float4 bodies with tails of 1-3"""
    _check_case(SIZES, [i % 2 == 1 for i in range(len(SIZES))], PAPER, first, NORMS["0.37"], 11, what=f"sizes first={first}")


def test_single_tensors():
    """each size as a table of its own (chunk count below / above the workgroup count), shadow on the scalar tails"""
    for n in SIZES[1:]:
        _check_case([n], [True], PAPER, 0, NORMS["0.37"], 100 + n, what=f"n={n}")


def test_large_tensor():
    """2^24 + 3 elements: 2049 chunks for every workgroup count, a 3-element tail behind the last full chunk"""
    _check_case([(1 << 24) + 3], [True], PAPER, 0, NORMS["0.37"], 12, what="2^24+3")


@pytest.mark.parametrize("where", ["first", "middle", "last", "all-but-one"])
def test_empty_tensors_in_a_table(where):
    sizes = {"first": [0, 0, 8193, 5], "middle": [5, 0, 8193, 0, 0, 100], "last": [8192, 1027, 0, 0], "all-but-one": [0, 0, 3, 0]}[where]
    _check_case(sizes, [True] * len(sizes), PAPER, 0, NORMS["0.37"], 13, what=f"empty {where}")


@pytest.mark.parametrize("count", [1, 47, 48, 49, 100])
def test_table_lengths(count):
    """the multi entry splits at YOLO_MT_MAX = 48 tensors per launch; the background entry takes at most 48 and must reject more"""
    from yolo._hip import E_ARG, SgdTensor
    pool = [5, 8193, 1, 1027, 0, 4, 8192, 3 * 8192 + 4232, 3]
    sizes = [pool[i % len(pool)] for i in range(count)]
    _check_case(sizes, [i % 3 == 0 for i in range(count)], PAPER, count % 2, NORMS["0.37"], 14 + count, entries=[("multi", 0), ("bg", 1), ("bg", 128)],
                what=f"{count} tensors")
    if count > 48:
        x = torch.zeros(64, device="cuda")
        tab = (SgdTensor * count)(*[SgdTensor(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 4) for _ in range(count)])
        rc = _lib().yolo_sgd_step_multi_bg(tab, count, LR, 0.9, 0.0, 0.0, 0, 0, None, MAX_NORM, None, 4, _stream())
        assert rc == E_ARG and "yolo_sgd_step_multi_bg" in _last_error()
        torch.cuda.synchronize()
        assert not bool(x.any()), "a rejected call must not launch"


_GRID = [(h, first) for h in sr.HYPERS for first in (0, 1)]


@pytest.mark.parametrize("idx", range(len(_GRID)), ids=[f"{sr.hyper_id(h)}-first{f}" for h, f in _GRID])
def test_hyper_parameters(idx):
    """momentum 0 / 0.9, dampening 0 / 0.1, nesterov on / off, weight decay 0 / 5e-4, first step or not; the norm cases rotate through the grid (so
    the clip is active in some and not in others) and every second case passes a zero skip_flag"""
    h, first = _GRID[idx]
    name = list(NORMS)[idx % len(NORMS)]
    _check_case([8193, 4, 1027, 3 * 8192 + 4232], [True, False, True, False], h, first, NORMS[name], 200 + idx, skip_zero=bool(idx % 2),
                what=f"{sr.hyper_id(h)} first={first} norm={name}")


@pytest.mark.parametrize("clip", ["active", "inactive"])
@pytest.mark.parametrize("h", sr.HYPERS, ids=sr.hyper_id)
def test_hyper_parameters_clip_on_and_off(h, clip):
    """every hyper-parameter combination with the clip active (0.37) and inactive (norm below max_norm)"""
    _check_case([8193, 5, 1024], [True, True, False], h, 0, NORMS["0.37" if clip == "active" else "small"], 260, what=f"{sr.hyper_id(h)} clip {clip}")


@pytest.mark.parametrize("name", list(NORMS))
def test_clip_coefficient_cases(name):
    """norm_sq NULL, clip > 1 (no scaling), max_norm^2 +- 3 fp64 ulps, the fp32 totals for which c is exactly 1 and just above, a real clip of 0.37"""
    _check_case([8193, 5, 1024], [True, True, False], PAPER, 0, NORMS[name], 300, what=f"norm {name}")


def test_momentum_zero_takes_a_null_buffer():
    """without momentum the kernels never form an address from buf: NULL is legal there (and only there)"""
    from yolo._hip import E_ARG, SgdTensor
    L, st = _lib(), _stream()
    h = dict(momentum=0.0, dampening=0.0, nesterov=False, wd=5e-4)
    (p, g, _), = _inputs([8193], 31)
    for entry in ("single", "multi", "bg"):
        P, G = Guarded(p), _gbuf(g)
        tab = (SgdTensor * 1)(SgdTensor(P.ptr, G._base_ptr, None, None, P.n))
        hy = (LR, 0.0, 0.0, 5e-4, 0, 0, None, MAX_NORM)
        rc = (L.yolo_sgd_step(P.ptr, G._base_ptr, None, P.n, *hy, None, None, st) if entry == "single" else
              L.yolo_sgd_step_multi(tab, 1, *hy, None, st) if entry == "multi" else L.yolo_sgd_step_multi_bg(tab, 1, *hy, None, 4, st))
        assert rc == 0, _last_error()
        torch.cuda.synchronize()
        (rp, _), (bp, _) = sr.sgd_ref(p, g, None, lr=LR, first_step=0, norm_sq=None, max_norm=MAX_NORM, **h)
        fails = []
        lr.check_values(rp, bp, P.t, "p", fails, entry)
        assert not fails and P.guards_ok(), fails
        assert L.yolo_sgd_step_multi(tab, 1, LR, 0.9, 0.0, 5e-4, 0, 0, None, MAX_NORM, None, st) == E_ARG


def test_three_steps_fed_back():
    """steps 1-3 on the kernel's own outputs (first_step on the first), each checked against the reference of that step's stored inputs"""
    sizes = [8193, 3, 3 * 8192 + 4232, 0, 1027]
    norm_sq = NORMS["0.37"]
    final = {}
    for h in (PAPER, dict(momentum=0.9, dampening=0.0, nesterov=True, wd=5e-4), dict(momentum=0.9, dampening=0.1, nesterov=False, wd=0.0)):
        for entry, wg in ENTRIES:
            ins = _inputs(sizes, 400)
            bufs = [(Guarded(p), _gbuf(g), Guarded(b), Guarded(torch.zeros(p.numel(), dtype=BF, device="cuda"), BF)) for p, g, b in ins]
            norm = torch.tensor([norm_sq], dtype=torch.float64, device="cuda")
            fails = []
            for step in (1, 2, 3):
                before = [(P.t.clone(), g.clone(), B.t.clone()) for P, g, B, _ in bufs]
                _run(entry, wg, bufs, h, step == 1, norm, None)
                torch.cuda.synchronize()
                _judge(f"{sr.hyper_id(h)} {entry}[{wg}] step {step}", bufs, before, h, step == 1, norm_sq, fails)
                assert all(not torch.equal(P.t, p0) for (P, _, _, _), (p0, _, _) in zip(bufs, before) if P.n), "the step must move the parameter"
            assert not fails, "\n".join(fails)
            final[(sr.hyper_id(h), entry, wg)] = [torch.cat([P.t, B.t]).view(torch.int32) for P, _, B, _ in bufs]
        first = final[(sr.hyper_id(h),) + ENTRIES[0]]
        for entry, wg in ENTRIES[1:]:
            assert all(torch.equal(a, b) for a, b in zip(first, final[(sr.hyper_id(h), entry, wg)])), f"{entry}[{wg}] differs from {ENTRIES[0]} after three steps"


@pytest.mark.parametrize("entry,wg", ENTRIES)
@pytest.mark.parametrize("first", [0, 1])
def test_skip_flag(entry, wg, first):
    """*skip_flag != 0: p, buf and the shadow keep their bytes; == 0: updated (the other tests check those values)"""
    sizes = [8193, 5, 0, 3 * 8192 + 4232]
    ins = _inputs(sizes, 500)
    norm = torch.tensor([NORMS["0.37"]], dtype=torch.float64, device="cuda")
    for flag in (1.0, -0.5, float("nan"), 0.0):
        bufs = [(Guarded(p), _gbuf(g), Guarded(b), Guarded(torch.full((p.numel(),), 3.0, dtype=BF, device="cuda"), BF)) for p, g, b in ins]
        raw = [[X.raw.clone() for X in (P, B, PB)] for P, _, B, PB in bufs]
        _run(entry, wg, bufs, PAPER, first, norm, torch.tensor([flag], device="cuda"))
        torch.cuda.synchronize()
        for (P, g, B, PB), r0, (p, _, b) in zip(bufs, raw, ins):
            kept = all(torch.equal(X.raw, r) for X, r in zip((P, B, PB), r0))                  # the whole allocations, guard bands included
            if not P.n:
                assert kept
                continue
            moved = not torch.equal(P.t, p) and not torch.equal(B.t, b) and torch.equal(PB.t.view(torch.int16), sr.bf16_bits(P.t))
            assert (kept if flag != 0.0 else moved), f"skip_flag {flag}: tensor of {P.n}"
            assert all(X.guards_ok() for X in (P, B, PB))


def test_sgd_entries_reject_bad_arguments():
    """the documented codes, each checked on the host before any launch: nothing may change"""
    from yolo._hip import E_ARG, E_UNSUPPORTED, SgdTensor
    L, st = _lib(), _stream()
    x = [torch.ones(64, device="cuda") for _ in range(3)]
    sh = torch.zeros(64, dtype=BF, device="cuda")
    p, g, b = (t.data_ptr() for t in x)
    hy = lambda **kw: (kw.get("lr", LR), kw.get("momentum", 0.9), kw.get("dampening", 0.0), kw.get("wd", 5e-4), kw.get("nesterov", 0), kw.get("first", 0),
                       None, MAX_NORM)
    one = lambda **kw: L.yolo_sgd_step(kw.get("p", p), kw.get("g", g), kw.get("b", b), kw.get("n", 16), *hy(**kw), kw.get("pb"), None, st)
    assert one(lr=-1.0) == E_ARG and "yolo_sgd_step" in _last_error()
    assert one(momentum=-0.1) == E_ARG and one(wd=-1e-4) == E_ARG
    assert one(nesterov=1, momentum=0.0) == E_ARG and one(nesterov=1, dampening=0.1) == E_ARG and "Nesterov" in _last_error()
    assert one(n=-1) == E_ARG and one(p=None) == E_ARG and one(g=None) == E_ARG and one(b=None) == E_ARG and one(b=None, first=1) == E_ARG
    assert one(p=p + 4) == E_UNSUPPORTED and one(g=g + 8) == E_UNSUPPORTED and one(b=b + 4) == E_UNSUPPORTED
    assert one(pb=sh.data_ptr() + 2) == E_UNSUPPORTED and "8-B" in _last_error()
    T = lambda **kw: SgdTensor(kw.get("p", p), kw.get("g", g), kw.get("b", b), kw.get("pb"), kw.get("n", 16))
    for fn, extra in ((L.yolo_sgd_step_multi, ()), (L.yolo_sgd_step_multi_bg, (4,))):
        call = lambda tab, count, **kw: fn(tab, count, *hy(**kw), None, *extra, st)
        ok = (SgdTensor * 2)(T(), T())
        assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG
        assert call(ok, 2, lr=-1.0) == E_ARG and call(ok, 2, momentum=-1.0) == E_ARG and call(ok, 2, wd=-1.0) == E_ARG
        assert call(ok, 2, nesterov=1, momentum=0.0) == E_ARG and call(ok, 2, nesterov=1, dampening=0.1) == E_ARG
        assert call((SgdTensor * 2)(T(), T(p=None)), 2) == E_ARG and "tensor 1" in _last_error()
        assert call((SgdTensor * 2)(T(), T(b=None)), 2) == E_ARG and call((SgdTensor * 2)(T(), T(n=-3)), 2) == E_ARG
        assert call((SgdTensor * 2)(T(g=g + 4), T()), 2) == E_UNSUPPORTED and "tensor 0" in _last_error()
        assert call((SgdTensor * 2)(T(), T(b=b + 8)), 2) == E_UNSUPPORTED and "tensor 1" in _last_error()
        # the refused tensor is the LAST of the table: the valid ones in front of it must not have been launched either
        assert call((SgdTensor * 2)(T(), T(pb=sh.data_ptr() + 2)), 2) == E_UNSUPPORTED and "shadow 1" in _last_error()
    ok = (SgdTensor * 2)(T(), T())
    for wg in (0, -1, 257):
        assert L.yolo_sgd_step_multi_bg(ok, 2, *hy(), None, wg, st) == E_ARG
    # 49 tensors through the multi entry, the 49th refused: the first launch (48 tensors) must not have happened
    many = (SgdTensor * 49)(*([T()] * 48 + [T(g=g + 4)]))
    assert L.yolo_sgd_step_multi(many, 49, *hy(), None, st) == E_UNSUPPORTED and "tensor 48" in _last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in x) and not bool(sh.any())


def test_yolo_sgd_on_the_model_with_the_background_pass():
    """yolo.optim.SGD (the paper's recipe, clip 10) on YOLOv1 with attach_plan(plan, overlap=True), two train steps on synthetic data: the Linear
    layers' bf16 forward operands in the plan equal the cast of their fp32 masters bit for bit and the engine's cache accepts them; parameters and
    momentum buffers equal, BIT FOR BIT, those of the same two steps taken by a second optimizer with overlap=False (foreground launches only) on a
    copy of the model -- the same kernel arithmetic in both forms.

    "The same two steps" means the same gradients: the conv weight gradients are summed with fp32 atomics and differ from run to run (DESIGN.md:
    training is not deterministic), so the second optimizer is handed the first model's gradient tensors, and the squared-norm hints its plan's
    backward left for them, instead of running a backward pass of its own.  (What remains: each optimizer sums the squares of the other gradients
    with fp64 atomics of its own; a different order moves the fp64 sum by ~1e-16 relative, which changes the fp32 clip coefficient about once in
    1e8 runs.)"""
    import copy
    import synth
    from yolo import YOLOLoss, YOLOv1
    from yolo.optim import SGD
    torch.manual_seed(6)
    mA = YOLOv1().cuda().train()
    mB = copy.deepcopy(mA)
    start = [p.detach().clone() for p in mA.parameters()]
    kw = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
    oA, oB = SGD(mA.parameters(), **kw), SGD(mB.parameters(), **kw)
    planA, planB = mA.hip_plan(), mB.hip_plan()
    oA.attach_plan(planA, overlap=True)
    oB.attach_plan(planB, overlap=False)
    assert oA.deferred and not oB.deferred and len(oA.bf16_shadow) == len(oB.bf16_shadow) >= 2
    x = torch.from_numpy(synth.synth_images(2, 3)).cuda()
    tgt = torch.from_numpy(synth.synth_targets(2, 4)).cuda()
    crit = YOLOLoss()
    for step in range(2):
        oA.zero_grad(set_to_none=True)
        loss, parts = crit(mA(x), tgt)              # the forward waits for the previous step's background pass in front of the Linear layers
        loss.backward()
        hints = dict(planA.grad_norm_sq)
        assert hints, "the backward pass leaves the squared norm of the big Linear's gradient"
        for p, q in zip(mA.parameters(), mB.parameters()):
            q.grad = p.grad
            if id(p) in hints:
                planB.grad_norm_sq[id(q)] = hints[id(p)]
        oA.skip_if = oB.skip_if = parts.device_flag
        oB.step()
        oA.step()
        assert oA._pending is not None and oB._pending is None
        assert float(parts["total"]) > 0
    oA.synchronize()
    torch.cuda.synchronize()
    for m, o, plan in ((mA, oA, planA), (mB, oB, planB)):
        fc = [li for li, L in enumerate(plan.layers) if L.kind == "fc"]
        assert len(fc) == len(o.bf16_shadow)
        for li in fc:
            L = plan.layers[li]
            shadow = o.bf16_shadow[id(L.weight)][0]
            key, wf = plan._pf[li]
            assert wf is shadow and key == plan._wkey(L.weight), "the engine's cache must accept the optimizer's shadow"
            assert torch.equal(shadow.view(-1).view(torch.int16), sr.bf16_bits(L.weight.detach().view(-1))), "bf16 operand != bf16(master)"
    n_first = 0
    for p, q, p0 in zip(mA.parameters(), mB.parameters(), start):
        assert not torch.equal(p.detach(), p0), "two steps must move every parameter"
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), "background and foreground updates differ"
        bA, bB = oA.state[p]["momentum_buffer"], oB.state[q]["momentum_buffer"]
        assert torch.equal(bA.view(torch.int32), bB.view(torch.int32)) and bool(torch.isfinite(bA).all())
        n_first += 1
    assert n_first == 52
