"""Gradient accumulation without a GPU: tests/accum_ref.py's bounds against an fp32 emulation of the kernel, yolo.optim.GradAccumulator on CPU
tensors against the gradient of the concatenated batch, training.train_epoch(accum_steps=K) (steps, EMA updates, the dropped incomplete group,
the group's skip flag), two ranks over gloo (one all-reduce per K backward passes), the mute switch and the pre_reduce hook of
OverlappedGradAllReduce on a fake plan with recorded streams, the host-side argument checks of accum.hip, and train.py --accum-steps on the CPU."""

import os
import re
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import accum_ref as acr
import launch_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-v1_amd")


def _tiny_model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(8 * 14 * 14, 7 * 7 * 30))


def _data(n, seed=7):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import synth
    return torch.from_numpy(synth.synth_normal((n, 3, 14, 14), seed)), torch.from_numpy(synth.synth_targets(n, 3))


def _emulate(x, y, alpha):
    """what the kernel stores: the fp64 value (exact product, one addition well inside fp64) rounded to fp32 once"""
    v = alpha * x.double()
    return (v if y is None else v + y.double()).float()


def _full_batch(x, t):
    """[(fp32 gradient of the whole batch in one backward pass, atol)] per parameter of _tiny_model.  The fp32 full-batch gradient is itself a
    rounded sum (196 pixels x N images per conv weight) in another order than the micro-batches'; its own error, measured against the same
    backward pass in fp64, is the absolute slack: twice its largest value per tensor (one share for either side), next to rtol 1e-5"""
    sys.path.insert(0, PKG)
    from yolo import YOLOLoss
    m32, m64 = _tiny_model(), _tiny_model().double()
    YOLOLoss()(m32(x).view(-1, 7, 7, 30), t)[0].backward()
    YOLOLoss()(m64(x.double()).view(-1, 7, 7, 30), t.double())[0].backward()
    return [(p.grad, 2.0 * float((p.grad.double() - q.grad).abs().max())) for p, q in zip(m32.parameters(), m64.parameters())]


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 64])
def test_the_bound_holds_for_a_correctly_rounded_fma(K):
    """same-sign and near-cancelling x, y: every element of the emulation inside accum_ref's bound, with and without y; the bound is one
    unit roundoff of the value, not more"""
    gen = torch.Generator().manual_seed(11)
    alpha = acr.accum_alpha(K)
    x = torch.randn(1 << 16, generator=gen)
    same = x.abs() * torch.rand(1 << 16, generator=gen)
    x_pos = x.abs()
    cancel = (-alpha * x.double()).float() * (1.0 + 1e-3 * torch.randn(1 << 16, generator=gen))      # alpha x + y loses ~10 bits
    fails = []
    for tag, xx, yy in (("same sign", x_pos, same), ("cancelling", x, cancel), ("no y", x, None)):
        ref, bnd = acr.accum_ref(xx, yy, alpha)
        worst = lr.check_values(ref, bnd, _emulate(xx, yy, alpha), "accum", fails, f"K={K} {tag}")
        print(f"K={K} {tag}: worst |err| / bound {worst:.3f}")
        assert float((bnd / ref.abs().clamp_min(1e-300)).max()) <= 1.01 * 2.0 ** -24 * (1 + 1e-12)
    assert not fails, fails


@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_the_chain_bound_holds(K):
    """the stored fp32 chain (each link rounded once, fed its own fp32 predecessor) inside accum_chain_ref's propagated bound"""
    gen = torch.Generator().manual_seed(K)
    alpha = acr.accum_alpha(K)
    base = torch.randn(1 << 15, generator=gen)
    grads = [base * (1.0 if k % 2 == 0 else -1.0) * (1.0 + 1e-3 * torch.randn(1 << 15, generator=gen)) for k in range(K)]    # partial sums cancel
    a = _emulate(grads[0], None, alpha)
    for g in grads[1:]:
        a = _emulate(g, a, alpha)
    ref, bnd = acr.accum_chain_ref(grads, K)
    fails = []
    worst = lr.check_values(ref, bnd, a, "chain", fails, f"K={K}")
    print(f"K={K}: worst |err| / bound {worst:.3f}")
    assert not fails, fails
    mean = torch.stack([g.double() for g in grads]).mean(0)
    assert float((ref - mean).abs().max()) <= 2.0 ** -23 * float(torch.stack([g.double().abs() for g in grads]).sum(0).max())   # alpha = fp32(1/K)


def test_alpha_is_formed_in_double_and_narrowed_once():
    from yolo.optim import accum_alpha
    for K in (1, 2, 3, 4, 7, 64):
        assert acr.accum_alpha(K) == accum_alpha(K) == float(torch.tensor(1.0 / K, dtype=torch.float64).float())
    assert acr.accum_alpha(1) == 1.0 and acr.accum_alpha(2) == 0.5 and acr.accum_alpha(3) != 1.0 / 3.0


# ---------------------------------------------------------------------------------------------------------------------------------
# GradAccumulator on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_accumulated_gradient_is_the_gradient_of_the_concatenated_batch(K):
    sys.path.insert(0, PKG)
    from yolo import GradAccumulator, YOLOLoss
    x, t = _data(2 * K)
    crit = YOLOLoss()
    whole = _full_batch(x, t)
    model = _tiny_model()
    acc = GradAccumulator(model, K)
    made, answers = [], []
    for k in range(K):
        model.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, _ = crit(model(x[2 * k: 2 * k + 2]).view(-1, 7, 7, 30), t[2 * k: 2 * k + 2])
        loss.backward()
        made = [p.grad for p in model.parameters()]
        answers.append(acc.after_backward())
    assert answers == [False] * (K - 1) + [True]
    for p, (want, atol), g in zip(model.parameters(), whole, made):
        assert p.grad is g, "the fold goes INTO the gradient autograd made: p.grad stays that tensor"
        torch.testing.assert_close(p.grad, want, rtol=1e-5, atol=atol)
        assert K > 1 or torch.equal(p.grad, want)
    if K == 1:
        assert not acc._acc and not acc._arenas and not acc._rest, "steps == 1 allocates nothing"
    else:
        assert len(acc._acc) == 4 and not acc._arenas
    # a second group through the same object: the accumulators are overwritten, not added to
    for k in range(K):
        model.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, _ = crit(model(x[2 * k: 2 * k + 2]).view(-1, 7, 7, 30), t[2 * k: 2 * k + 2])
        loss.backward()
        last = acc.after_backward()
    assert last
    for p, (want, atol) in zip(model.parameters(), whole):
        torch.testing.assert_close(p.grad, want, rtol=1e-5, atol=atol)
    with pytest.raises(ValueError):
        GradAccumulator(model, 0)


def test_group_flag_is_the_maximum_of_the_micro_batches_flags():
    sys.path.insert(0, PKG)
    from yolo import GradAccumulator
    model = nn.Linear(4, 2)
    acc = GradAccumulator(model, 3)
    for group, flags in enumerate(([0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [None, None, None])):
        for f in flags:
            model.zero_grad(set_to_none=True)
            acc.before_backward()
            model(torch.ones(1, 4)).sum().backward()
            done = acc.after_backward(None if f is None else torch.tensor([f]))
        assert done
        assert (acc.skip_if is None) if flags[0] is None else float(acc.skip_if) == max(flags), group


# ---------------------------------------------------------------------------------------------------------------------------------
# train_epoch(accum_steps=K)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Parts(dict):
    device_flag = None


class _Criterion:
    """YOLOLoss whose parts carry a device_flag like the GPU loss's LossParts; every call's parts are kept"""

    def __init__(self, flag_at=None):
        sys.path.insert(0, PKG)
        from yolo import YOLOLoss
        self.inner, self.calls, self.flag_at = YOLOLoss(), [], flag_at

    def __call__(self, pred, target):
        loss, parts = self.inner(pred, target)
        parts = _Parts(parts)
        parts.device_flag = torch.tensor([1.0 if len(self.calls) == self.flag_at else 0.0])
        self.calls.append(parts)
        return loss, parts


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.body = _tiny_model()

    def forward(self, x):
        return self.body(x).view(-1, 7, 7, 30)


def _counting_sgd(params):
    from yolo.optim import SGD

    class Counting(SGD):
        seen = None

        def step(self, closure=None):
            type(self).seen = (type(self).seen or []) + [None if self.skip_if is None else float(self.skip_if)]
            return super().step(closure)
    return Counting(params, lr=0.05, max_grad_norm=10.0)


@pytest.mark.parametrize("K", [2, 3])
def test_train_epoch_steps_once_per_group_and_drops_the_incomplete_one(K):
    """7 batches: 7 // K optimizer steps and EMA updates; the returned means cover the applied groups only; the parameters are those of a hand-written
    loop over the complete groups"""
    sys.path.insert(0, PKG)
    from torch.utils.data import DataLoader, TensorDataset
    from yolo import GradAccumulator, ModelEMA, training
    x, t = _data(14, 9)
    loader = DataLoader(TensorDataset(x, t), batch_size=2)
    assert len(loader) == 7
    model, crit = _Net(), _Criterion()
    opt = _counting_sgd(model.parameters())
    ema = ModelEMA(model, decay=0.5, optimizer=opt)
    out = training.train_epoch(model, loader, crit, opt, "cpu", 1, ema=ema, accum_steps=K)
    steps = 7 // K
    assert len(type(opt).seen) == steps and ema.updates == steps and len(crit.calls) == 7
    assert type(opt).seen == [0.0] * steps, "the group's flag reaches the optimizer, zero for valid targets"
    for k in ("total", "coord", "conf_obj", "conf_noobj", "class"):
        want = sum(float(p[k]) for p in crit.calls[: steps * K]) / (steps * K)
        assert out[k] == pytest.approx(want, rel=1e-6), k
    # the same by hand
    ref, crit2 = _Net(), _Criterion()
    opt2 = _counting_sgd(ref.parameters())
    acc = GradAccumulator(ref, K)
    ref.train()
    for b, (xb, tb) in enumerate(loader):
        if b >= steps * K:
            break
        opt2.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, _ = crit2(ref(xb), tb)
        loss.backward()
        if acc.after_backward():
            opt2.step()
    for p, q in zip(model.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    moved = _Net()
    assert all(not torch.equal(p, q) for p, q in zip(model.parameters(), moved.parameters()))


def test_train_epoch_hands_a_flagged_micro_batch_to_the_optimizer():
    """a device_flag set on the second of three micro-batches reaches optimizer.skip_if non-zero: the step and the EMA update are cancelled, the
    next group's are not"""
    sys.path.insert(0, PKG)
    from torch.utils.data import DataLoader, TensorDataset
    from yolo import ModelEMA, training
    x, t = _data(12, 9)
    loader = DataLoader(TensorDataset(x, t), batch_size=2)
    model, crit = _Net(), _Criterion(flag_at=1)
    opt = _counting_sgd(model.parameters())
    ema = ModelEMA(model, decay=0.5, optimizer=opt)
    start = [p.detach().clone() for p in model.parameters()]
    seen_after_first = []
    inner_step = opt.step

    def step(closure=None):
        r = inner_step(closure)
        if not seen_after_first:
            seen_after_first.append([p.detach().clone() for p in model.parameters()])
        return r
    opt.step = step
    training.train_epoch(model, loader, crit, opt, "cpu", 1, ema=ema, accum_steps=3)
    assert type(opt).seen == [1.0, 0.0]
    assert all(torch.equal(a, b) for a, b in zip(start, seen_after_first[0])), "the flagged group's step updates nothing"
    assert ema.updates == 1 and all(not torch.equal(a, p) for a, p in zip(start, model.parameters()))


def test_accum_steps_one_is_the_loop_without_the_option():
    """accum_steps=1: no accumulator is built, the parameters are bit-equal to a call without the keyword"""
    sys.path.insert(0, PKG)
    from torch.utils.data import DataLoader, TensorDataset
    from yolo import training
    x, t = _data(6, 9)
    loader = DataLoader(TensorDataset(x, t), batch_size=2)
    got = []
    for kw in ({}, {"accum_steps": 1}):
        model = _Net()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        training.train_epoch(model, loader, _Criterion(), opt, "cpu", 1, **kw)
        assert not hasattr(model, "_yolo_grad_accumulator")
        got.append([p.detach().clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*got))


# ---------------------------------------------------------------------------------------------------------------------------------
# two ranks over gloo
# ---------------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    for p in (ROOT, PKG, os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from yolo import GradAccumulator, YOLOLoss
    from yolo.parallel import broadcast_parameters, make_grad_reducer
    model = _tiny_model()
    broadcast_parameters(model)
    red = make_grad_reducer(model, "cpu")
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    dist.all_reduce = counted
    x, t = _data(8)
    crit = YOLOLoss()
    counts = {}
    for K in (1, 2):
        acc = GradAccumulator(model, K, red)
        calls[0] = 0
        per_micro = []
        for k in range(K):
            lo = (rank * 2 + k) * 2 if K == 2 else rank * 4          # K = 2: micro-batches of 2 images; K = 1: the rank's 4 images at once
            n = 2 if K == 2 else 4
            model.zero_grad(set_to_none=True)
            acc.before_backward()
            loss, _ = crit(model(x[lo: lo + n]).view(-1, 7, 7, 30), t[lo: lo + n])
            loss.backward()
            done = acc.after_backward()
            per_micro.append((calls[0], done))
        counts[K] = per_micro
        grads = [p.grad.numpy().copy() for p in model.parameters()]
    dist.all_reduce = real
    q.put((rank, counts, grads))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_all_reduce_per_group():
    """K = 2 over gloo: as many dist.all_reduce calls per optimizer step as K = 1 and none during the first micro-batch; both ranks end with
    equal gradients, the full-batch gradient of all four micro-batches"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, counts, _ in res:
        (n1, done1), = counts[1]
        (first, d0), (n2, d1) = counts[2]
        assert done1 and not d0 and d1
        assert n1 > 0 and first == 0 and n2 == n1, counts
    whole = _full_batch(*_data(8))
    for _, _, grads in res:
        for g, (want, atol) in zip(grads, whole):
            torch.testing.assert_close(torch.from_numpy(g), want, rtol=1e-5, atol=atol)
    for a, b in zip(res[0][2], res[1][2]):
        assert (a == b).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# OverlappedGradAllReduce: the mute switch and the pre_reduce hook, on a fake plan with recorded streams
# ---------------------------------------------------------------------------------------------------------------------------------
class _ArenaPlan:
    """engine.Plan as the reducer and the accumulator see it, on the CPU: a gradient arena holding every gradient of a tiny model in the order
    backward produces them (last layer first), the callbacks and the squared-norm hint.  ``backward_into_arena`` follows the schedule of
    Plan.backward: the side stream waits for the main one, weight gradients are produced and announced on the side stream, the main stream
    joins, on_backward_done runs from the main stream."""

    MAIN, SIDE = 0x1000, 0x2000

    def __init__(self, model):
        self.params = list(model.parameters())
        rev = list(reversed(self.params))
        order = [p for p in rev if p.dim() > 1] + [p for p in rev if p.dim() == 1]      # the weights, then the bias region (attach_grad_arena)
        self.views, off = {}, 0
        for p in order:
            self.views[id(p)] = (off, off + p.numel())
            off += p.numel()
        self.arena = torch.zeros(off)
        self.on_grad_ready = self.on_backward_done = self.on_stream_wait = None
        self.grad_norm_sq = {}
        self.cur = self.MAIN
        self.events = []

    def backward_into_arena(self, loss):
        grads = torch.autograd.grad(loss, self.params)
        for p, g in zip(self.params, grads):
            lo, hi = self.views[id(p)]
            self.arena[lo:hi].copy_(g.reshape(-1))
            p.grad = self.arena[lo:hi].view_as(p)
        self.micro = self.arena.clone()                 # this pass's own gradient, before any callback folds into it
        big = self.params[-2]
        self.grad_norm_sq[id(big)] = ((big.grad.data_ptr(), tuple(big.grad.shape)), big.grad._version, big.grad.double().pow(2).sum())
        note = self.on_stream_wait
        if note is not None:
            note(self.SIDE, self.MAIN)                  # _on_side_stream.__enter__
        self.cur = self.SIDE
        for p in reversed(self.params):
            if p.dim() > 1 and self.on_grad_ready is not None:
                self.on_grad_ready(*self.views[id(p)])  # (bias gradients are final only at the join)
        self.cur = self.MAIN
        if note is not None:
            note(self.MAIN, self.SIDE)                  # _finish_backward
        if self.on_backward_done is not None:
            self.on_backward_done()


def test_muted_passes_announce_nothing_and_the_armed_pass_folds_in_front_of_each_collective(monkeypatch):
    """K = 3 through OverlappedGradAllReduce (gloo, world size 1): the backward passes 1 and 2 leave no piece, no log entry and no collective; on the
    third every bucket's pre_reduce comes immediately before its collective, from a stream that passes _check_ordered, and the pre_reduce ranges
    tile [0, numel) exactly once; p.grad ends as the mean of the three micro-gradients, still a view of the arena, the norm hint dropped and the
    arena's version bumped"""
    sys.path.insert(0, PKG)
    from yolo import GradAccumulator, YOLOLoss
    from yolo.parallel import OverlappedGradAllReduce
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(41500 + os.getpid() % 2000)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        model = _tiny_model()
        plan = _ArenaPlan(model)
        red = OverlappedGradAllReduce(plan, "cpu", bucket_bytes=4 * 3000, stream_id=lambda: plan.cur)
        red.log = []
        acc = GradAccumulator(model, 3, red)
        assert red.pre_reduce is not None and len(acc._arenas) == 1 and not acc._rest
        events = []
        fold = red.pre_reduce

        def pre(lo, hi):
            red._check_ordered(lo, hi, plan.cur)        # raises if this stream does not hold the range
            events.append(("fold", lo, hi, plan.cur))
            fold(lo, hi)
        red.pre_reduce = pre
        real = dist.all_reduce

        def all_reduce(tensor, *a, **k):
            lo = (tensor.data_ptr() - plan.arena.data_ptr()) // 4
            events.append(("reduce", lo, lo + tensor.numel(), plan.cur))
            return real(tensor, *a, **k)
        monkeypatch.setattr(dist, "all_reduce", all_reduce)
        x, t = _data(6)
        crit = YOLOLoss()
        micro = []
        for k in range(3):
            acc.before_backward()
            loss, _ = crit(model(x[2 * k: 2 * k + 2]).view(-1, 7, 7, 30), t[2 * k: 2 * k + 2])
            plan.backward_into_arena(loss)
            micro.append(plan.micro)
            if k < 2:
                assert red.muted and not events and not red.log and not red._pieces and not red._waits and not red._handles
                assert acc.after_backward() is False
                assert not events, "the accumulation itself communicates nothing"
            else:
                assert not red.muted
                ptrs = [p.grad.data_ptr() for p in model.parameters()]
                v0 = plan.arena._version
                assert acc.after_backward() is True
        folds = [e for e in events if e[0] == "fold"]
        assert len(folds) >= 2 and any(e[3] == plan.SIDE for e in folds) and folds[-1][3] == plan.MAIN
        covered = 0
        for e in folds:
            assert e[1] == covered and e[2] > e[1]
            covered = e[2]
        assert covered == plan.arena.numel(), "the pre_reduce ranges tile the arena exactly once"
        assert len(events) == 2 * len(folds)
        for f, r in zip(events[0::2], events[1::2]):
            assert f[0] == "fold" and r[0] == "reduce" and f[1:] == r[1:], "every fold immediately in front of its own collective, on its stream"
        assert [(lo, hi, cur) for lo, hi, cur, _ in red.log] == [e[1:] for e in folds]
        ref, bnd = acr.accum_chain_ref(micro, 3)
        torch.testing.assert_close(plan.arena.double(), ref, rtol=1e-5, atol=1e-7)        # (torch's CPU ops round the product too: no fma bound here)
        assert [p.grad.data_ptr() for p in model.parameters()] == ptrs
        assert not plan.grad_norm_sq and plan.arena._version > v0
        # an unordered fold is caught where the collective would be: a range produced on the side stream, reduced from main without a wait
        acc.before_backward(); acc.micro = 2; red.muted = False
        plan.cur = plan.SIDE
        red._ready(0, 10)
        plan.cur = plan.MAIN
        with pytest.raises(RuntimeError, match="has not waited"):
            red._reduce(0, 10)
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------------------
# the ABI surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_accum_entry_is_declared_bound_and_called_by_the_gpu_test():
    sys.path.insert(0, PKG)
    from yolo import _hip
    with open(os.path.join(PKG, "csrc", "accum.hip")) as f:
        src = f.read()
    entries = set(re.findall(r"YOLO_API int (yolo_\w+)", src))
    assert entries == {"yolo_grad_accum", "yolo_grad_accum_multi"}
    assert "fmaf(alpha, x, y)" in src[:src.index("#include")], "the header comment states the formula"
    assert "__shared__" not in src and "asm" not in src, "no LDS, no inline assembly"
    with open(os.path.join(ROOT, "include", "yolo_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tests", "test_gpu_accum.py")) as f:
        called = set(re.findall(r"\.(yolo_\w+)\b", f.read()))
    for name in entries:
        assert re.search(rf"\bint {name}\(", header) and name in _hip._SIGS and name in called, name
    assert re.search(r"#define YOLO_HIP_ABI_VERSION 2\b", header) and _hip.ABI_VERSION == 2


def test_accum_entries_refuse_bad_arguments_on_the_host():
    """the argument checks run before any HIP call, so they can be exercised without a device; the pointers are never dereferenced"""
    sys.path.insert(0, PKG)
    from yolo import _hip
    if not _hip.available():
        import __graft_entry__ as g
        g.build()
    L = _hip.lib()
    E_ARG, E_UNS, T = _hip.E_ARG, _hip.E_UNSUPPORTED, _hip.AccumTensor
    d, x, y = 0x10000, 0x20000, 0x30000            # 16-B aligned, 64 KB apart
    one = lambda **k: L.yolo_grad_accum(k.get("d", d), k.get("x", x), k.get("y", y), k.get("n", 16), k.get("a", 0.5), None, None)
    err = lambda: L.yolo_hip_last_error()
    assert one(d=None) == E_ARG and b"yolo_grad_accum" in err() and b"null" in err()
    assert one(x=None) == E_ARG and one(n=-1) == E_ARG and b"negative" in err()
    for a in (float("nan"), float("inf"), -float("inf")):
        assert one(a=a) == E_ARG and b"not finite" in err(), a
    for k in ("d", "x", "y"):
        assert one(**{k: {"d": d, "x": x, "y": y}[k] + 4}) == E_UNS and b"16-B" in err(), k
    assert one(d=x + 32) == E_UNS and b"overlaps x" in err()         # half a tensor into x
    assert one(d=y - 32) == E_UNS and b"overlaps y" in err()
    ok = (T * 2)(T(d, x, y, 16), T(d + 4096, x + 4096, None, 16))
    call = lambda tab, count, a=0.5: L.yolo_grad_accum_multi(tab, count, a, None, None)
    assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG and call(ok, 2, a=float("nan")) == E_ARG
    assert call((T * 2)(T(d, x, y, 16), T(None, x, y, 16)), 2) == E_ARG and b"tensor 1" in err()
    assert call((T * 2)(T(d, x, y, 16), T(d, x, y, -2)), 2) == E_ARG
    assert call((T * 2)(T(d, x + 8, y, 16), T(d, x, y, 16)), 2) == E_UNS and b"tensor 0" in err()
    assert call((T * 2)(T(d, x, y, 16), T(d, d + 16, None, 16)), 2) == E_UNS and b"tensor 1" in err() and b"overlaps x" in err()
    assert call(ok, 0) == 0, "an empty table is legal and launches nothing"


def _run(args, **kw):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600, **kw)


def test_train_py_accum_steps_on_the_cpu(tmp_path):
    """train.py --accum-steps 2 on the CPU: 8 images in batches of 2 -> two optimizer steps, the checkpoint records accum_steps; K < 1 is an
    argparse error; without the option the checkpoint has no such key"""
    base = [os.path.join(PKG, "train.py"), "--synthetic", "8", "--batch-size", "2", "--backbone", "yolov1", "--device", "cpu", "--num-workers", "0",
            "--epochs", "1"]
    r = _run(base + ["--accum-steps", "0"])
    assert r.returncode == 2 and "--accum-steps" in r.stderr
    ck = tmp_path / "ck"
    r = _run(base + ["--accum-steps", "2", "--seed", "0", "--checkpoint-dir", str(ck)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert d["accum_steps"] == 2 and d["seed"] == 0
    steps = {int(s["step"]) for s in d["optimizer_state_dict"]["state"].values()}
    assert steps == {2}
    plain = tmp_path / "plain"
    r = _run(base + ["--seed", "0", "--checkpoint-dir", str(plain)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = torch.load(plain / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert "accum_steps" not in d and {int(s["step"]) for s in d["optimizer_state_dict"]["state"].values()} == {4}
