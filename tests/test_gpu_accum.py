"""The two gradient-accumulation entries of csrc/accum.hip, called through the C ABI as tests/test_gpu_ema.py calls the EMA entries, against
tests/accum_ref.py: the three uses of a K-step group (store: y = NULL; accumulate: dst = y; fold: dst = x) through the single and the multi-tensor
form, every written element within the bound of the one fp32 rounding, every written tensor between guard bands of a NaN pattern (4096 floats in
front of and behind it), every read-only tensor untouched, all forms and a repeated launch the same bits.  Then yolo.optim.GradAccumulator on the
YOLOv1 model (teacher-forced against the micro-gradients it was given), under EngineConfig.DETERMINISTIC and between two ranks in child
processes (tests/accum_child.py), and train.py --accum-steps."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

import accum_ref as acr
import launch_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "accum_child.py")
SIZES = [0, 1, 3, 255, 256, 257, 65536 + 5, (1 << 20) + 3]
POOL = [5, 8193, 1, 1027, 0, 4, 8192, 3 * 8192 + 4232, 3, 0]
TABLE50 = [POOL[i % len(POOL)] for i in range(50)]            # crosses YOLO_MT_MAX = 48; empty tensors inside and at the end of a launch
GROUPS = [1, 2, 3, 64]                                        # alpha = fp32(1 / K): 1.0, 0.5, fp32(1/3), fp32(1/64)
USES = ("store", "accumulate", "fold")
BAND = 4096                                                   # floats of NaN pattern in front of and behind every tensor
PAT = 0x7FC00D1E


def _lib():
    from yolo._hip import lib
    return lib()


def _stream():
    from yolo._hip import stream
    return stream()


def _last_error():
    return _lib().yolo_hip_last_error().decode(errors="replace")


class Banded:
    """a copy of `src` between two 4096-float bands of a NaN pattern inside one allocation (16-B aligned, valid pointer for an empty tensor)"""

    def __init__(self, src):
        self.n = src.numel()
        self.raw = torch.full((self.n + 2 * BAND,), PAT, dtype=torch.int32, device=src.device)
        self.t = self.raw.view(torch.float32)[BAND: BAND + self.n]
        self.t.copy_(src)
        self.ptr = self.raw.data_ptr() + 4 * BAND

    def bands_ok(self):
        return bool((self.raw[:BAND] == PAT).all()) and bool((self.raw[BAND + self.n:] == PAT).all())


@pytest.fixture(scope="module")
def inputs():
    """{table name: [(x, y, old)]} fp32 on the device -- the micro-gradient, the accumulator so far (same sign, or cancelling x / 3 to ~10 bits)
    and what a separate dst holds before the call -- and a cache of the references per (table, alpha, with y): computed once, never written"""
    gen = torch.Generator(device="cuda").manual_seed(23)
    out = {}
    for name, sizes in (("sizes", SIZES), ("table50", TABLE50)):
        tab = []
        for i, n in enumerate(sizes):
            x = torch.randn(n, generator=gen, device="cuda")
            if i % 2:
                y = -acr.accum_alpha(3) * x * (1.0 + 1e-3 * torch.randn(n, generator=gen, device="cuda"))
            else:
                y = x.sign() * torch.rand(n, generator=gen, device="cuda")
            tab.append((x, y, torch.randn(n, generator=gen, device="cuda")))
        out[name] = tab
    return out, {}


def _refs(inputs, name, alpha, with_y):
    tabs, cache = inputs
    key = (name, alpha, with_y)
    if key not in cache:
        cache[key] = [acr.accum_ref(x, y if with_y else None, alpha) for x, y, _ in tabs[name]]
    return cache[key]


def _operands(use, data):
    """Banded (D, X, Y) lists of one use -- D the written tensors, which ARE the Y of `accumulate` and the X of `fold`; Y is None for `store`"""
    if use == "store":
        return [Banded(o) for _, _, o in data], [Banded(x) for x, _, _ in data], None
    if use == "accumulate":
        Y = [Banded(y) for _, y, _ in data]
        return Y, [Banded(x) for x, _, _ in data], Y
    X = [Banded(x) for x, _, _ in data]
    return X, X, [Banded(y) for _, y, _ in data]


def _run(form, D, X, Y, alpha, skip=None):
    """one pass through one launch form; the return code must be 0"""
    from yolo._hip import AccumTensor
    L, st = _lib(), _stream()
    sptr = ctypes.c_void_p(skip.data_ptr()) if skip is not None else None
    yp = [y.ptr for y in Y] if Y is not None else [None] * len(D)
    if form == "single":
        for d, x, y in zip(D, X, yp):
            assert L.yolo_grad_accum(d.ptr, x.ptr, y, d.n, alpha, sptr, st) == 0, _last_error()
        return
    tab = (AccumTensor * len(D))(*[AccumTensor(d.ptr, x.ptr, y, d.n) for d, x, y in zip(D, X, yp)])
    assert L.yolo_grad_accum_multi(tab, len(D), alpha, sptr, st) == 0, _last_error()


@pytest.mark.parametrize("K", GROUPS)
@pytest.mark.parametrize("name", ["sizes", "table50"])
def test_three_uses_two_forms_within_the_bound_and_bit_equal(inputs, name, K):
    """every use through every launch form on the same inputs: within the reference's bound, guard bands intact, read-only operands untouched;
    the single form, the multi form and a repeated multi launch the same bits"""
    alpha = acr.accum_alpha(K)
    data = inputs[0][name]
    fails = []
    for use in USES:
        refs = _refs(inputs, name, alpha, use != "store")
        results = []
        for form in ("single", "multi", "multi"):                 # the multi form twice: the repeat launch, on fresh copies
            tag = f"{name} alpha={alpha} {use} {form}"
            D, X, Y = _operands(use, data)
            _run(form, D, X, Y, alpha)
            torch.cuda.synchronize()
            worst = 0.0
            for i, (d, (ref, bnd), (x0, y0, _)) in enumerate(zip(D, refs, data)):
                where = f"{tag}: tensor {i} (n={d.n})"
                if not (d.bands_ok() and X[i].bands_ok() and (Y is None or Y[i].bands_ok())):
                    fails.append(f"{where}: a guard band was overwritten")
                if X[i] is not d and not torch.equal(X[i].t.view(torch.int32), x0.view(torch.int32)):
                    fails.append(f"{where}: x was written")
                if Y is not None and Y[i] is not d and not torch.equal(Y[i].t.view(torch.int32), y0.view(torch.int32)):
                    fails.append(f"{where}: y was written")
                if d.n:
                    worst = max(worst, lr.check_values(ref, bnd, d.t, "accum", fails, where))
                    if alpha == 1.0 and use == "store" and not torch.equal(d.t.view(torch.int32), x0.view(torch.int32)):
                        fails.append(f"{where}: alpha = 1 without y must copy x")
            print(f"{tag}: worst |err| / bound {worst:.3f}")
            results.append([d.t.view(torch.int32).clone() for d in D])
        for r in results[1:]:
            if not all(torch.equal(a, b) for a, b in zip(results[0], r)):
                fails.append(f"{name} alpha={alpha} {use}: the launch forms differ in some bits")
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("form", ["single", "multi"])
def test_skip_flag(inputs, form):
    """*skip_flag != 0: dst keeps its bytes, guard bands included; == 0: written"""
    data = inputs[0]["sizes"]
    for use in USES:
        for flag in (1.0, -0.5, float("nan"), 0.0):
            D, X, Y = _operands(use, data)
            raw = [d.raw.clone() for d in D]
            _run(form, D, X, Y, 0.5, torch.tensor([flag], device="cuda"))
            torch.cuda.synchronize()
            for d, r0 in zip(D, raw):
                kept = torch.equal(d.raw, r0)
                assert kept if (flag != 0.0 or not d.n) else (not kept and d.bands_ok()), f"{use}: skip_flag {flag}: tensor of {d.n}"


def test_accum_entries_reject_bad_arguments():
    """the documented codes, each checked on the host before any launch: nothing may change"""
    from yolo._hip import E_ARG, E_UNSUPPORTED, AccumTensor as T
    L, st = _lib(), _stream()
    a, b, c = torch.ones(256, device="cuda"), torch.full((256,), 2.0, device="cuda"), torch.full((256,), 3.0, device="cuda")
    d, x, y = a.data_ptr(), b.data_ptr(), c.data_ptr()
    one = lambda **k: L.yolo_grad_accum(k.get("d", d), k.get("x", x), k.get("y", y), k.get("n", 16), k.get("a", 0.5), None, st)
    assert one(d=None) == E_ARG and one(x=None) == E_ARG and one(n=-1) == E_ARG and "yolo_grad_accum" in _last_error()
    for alpha in (float("nan"), float("inf"), -float("inf")):
        assert one(a=alpha) == E_ARG and "not finite" in _last_error(), alpha
    assert one(d=d + 4) == E_UNSUPPORTED and one(x=x + 4) == E_UNSUPPORTED and one(y=y + 4) == E_UNSUPPORTED and "16-B" in _last_error()
    # dst overlapping x (or y) by half a tensor: neither the in-place use nor disjoint
    assert one(d=x + 32) == E_UNSUPPORTED and "overlaps x" in _last_error()
    assert one(d=d, x=d + 32) == E_UNSUPPORTED and one(d=y + 32) == E_UNSUPPORTED and "overlaps y" in _last_error()
    ok = (T * 2)(T(d, x, y, 16), T(d + 512, x + 512, None, 16))
    call = lambda tab, count, alpha=0.5: L.yolo_grad_accum_multi(tab, count, alpha, None, st)
    assert call(None, 2) == E_ARG and call(ok, -1) == E_ARG and call(ok, 2, alpha=float("nan")) == E_ARG and call(ok, 2, alpha=float("inf")) == E_ARG
    assert call((T * 2)(T(d, x, y, 16), T(None, x, y, 16)), 2) == E_ARG and "tensor 1" in _last_error()
    assert call((T * 2)(T(d, x, y, 16), T(d + 512, None, y, 16)), 2) == E_ARG and call((T * 2)(T(d, x, y, 16), T(d + 512, x + 512, y, -2)), 2) == E_ARG
    # the refused tensor is the LAST of the table: the valid one in front of it must not have been launched either
    assert call((T * 2)(T(d, x, y, 16), T(d + 512, x + 516, y, 16)), 2) == E_UNSUPPORTED and "tensor 1" in _last_error()
    assert call((T * 2)(T(d, x, y, 16), T(d + 512, d + 512 + 32, None, 16)), 2) == E_UNSUPPORTED and "overlaps x" in _last_error()
    # 49 tensors, the 49th refused: the first launch (48 tensors) must not have happened
    many = (T * 49)(*[T(d + 16 * i, x + 16 * i, y + 16 * i, 4) for i in range(49)])
    many[48] = T(d + 16 * 48, x + 16 * 48 + 4, None, 4)
    assert call(many, 49) == E_UNSUPPORTED and "tensor 48" in _last_error()
    torch.cuda.synchronize()
    assert bool((a == 1).all()) and bool((b == 2).all()) and bool((c == 3).all()), "a refused call must not launch"


@pytest.mark.parametrize("form", ["single", "multi"])
def test_chain_of_four_in_place(form):
    """K = 4 as GradAccumulator runs it: the first call stores into the accumulator (which holds garbage), two accumulate in place, the last folds
    into the fourth micro-gradient's own memory -- within accum_chain_ref's bound, the accumulator and the earlier micro-gradients as they were"""
    gen = torch.Generator(device="cuda").manual_seed(4)
    sizes = [3 * 8192 + 4232, 257, 0, 8192]
    alpha = acr.accum_alpha(4)
    base = [torch.randn(n, generator=gen, device="cuda") for n in sizes]
    grads = [[b * (1.0 if k % 2 == 0 else -1.0) * (1.0 + 1e-3 * torch.randn(b.numel(), generator=gen, device="cuda")) for b in base] for k in range(4)]
    G = [[Banded(g) for g in micro] for micro in grads]
    A = [Banded(torch.full((n,), float("nan"), device="cuda")) for n in sizes]       # needs no clearing
    _run(form, A, G[0], None, alpha)
    _run(form, A, G[1], A, alpha)
    _run(form, A, G[2], A, alpha)
    before_fold = [a.t.clone() for a in A]
    _run(form, G[3], G[3], A, alpha)
    torch.cuda.synchronize()
    fails = []
    for i, n in enumerate(sizes):
        ref, bnd = acr.accum_chain_ref([grads[k][i] for k in range(4)], 4)
        assert all(G[k][i].bands_ok() for k in range(4)) and A[i].bands_ok()
        assert torch.equal(A[i].t, before_fold[i]) and all(torch.equal(G[k][i].t, grads[k][i]) for k in range(3))
        if n:
            worst = lr.check_values(ref, bnd, G[3][i].t, "chain", fails, f"{form}: tensor {i} (n={n})")
            print(f"{form}: tensor {i}: worst |err| / bound {worst:.3f}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------------------
# GradAccumulator on the YOLOv1 model
# ---------------------------------------------------------------------------------------------------------------------------------
def _build():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import synth
    from yolo import YOLOv1
    m = YOLOv1()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.yolov1_state_dict().items()}, strict=True)
    return m.cuda().eval()                      # eval: no dropout, so that every pass sees the same network


def test_model_teacher_forced_chain_and_the_step_behind_it():
    """K = 3 micro-batches of 2 images through GradAccumulator on the fused YOLOv1: every parameter's folded gradient within accum_chain_ref of the
    three micro-gradients it was given (cloned after each backward -- exact whatever the conv kernels round), p.grad still the arena view, the
    plan's norm hint gone; Adam(max_grad_norm=10) then moves the biases exactly as a second Adam does on a second model whose .grad was set to
    the folded gradients"""
    import synth
    from yolo import GradAccumulator, YOLOLoss
    from yolo.optim import Adam
    K = 3
    m = _build()
    plan = m.hip_plan()
    opt = Adam(m.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(plan)
    acc = GradAccumulator(m, K)
    assert plan.arena is not None and len(acc._arenas) == 1 and not acc._rest and plan.on_grad_ready is None
    assert acc._arenas[0][1].numel() == plan.arena.numel()
    x = torch.from_numpy(synth.synth_images(2 * K, 23)).cuda()
    t = torch.from_numpy(synth.synth_targets(2 * K, 41, max_obj=3)).cuda()
    crit = YOLOLoss()
    micro, ptrs = [], None
    for k in range(K):
        opt.zero_grad(set_to_none=True)
        acc.before_backward()
        loss, parts = crit(m(x[2 * k: 2 * k + 2]), t[2 * k: 2 * k + 2])
        loss.backward()
        micro.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
        ptrs = {n: p.grad.data_ptr() for n, p in m.named_parameters()}
        if k == K - 1:
            assert plan.grad_norm_sq, "the backward pass leaves FC1's norm hint: the test below must see it dropped"
        assert acc.after_backward(parts.device_flag) is (k == K - 1)
    torch.cuda.synchronize()
    assert not plan.grad_norm_sq
    assert float(acc.skip_if) == 0.0
    fails, worst = [], 0.0
    lo, hi = plan.arena.data_ptr(), plan.arena.data_ptr() + 4 * plan.arena.numel()
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() == ptrs[n] and lo <= p.grad.data_ptr() < hi, f"{n}: p.grad is no longer the arena view"
        ref, bnd = acr.accum_chain_ref([mg[n] for mg in micro], K)
        worst = max(worst, lr.check_values(ref, bnd, p.grad, n, fails, "folded"))
        assert not torch.equal(p.grad, micro[-1][n]), f"{n}: the fold did not happen"
        del ref, bnd
    print(f"folded gradients: worst |err| / bound {worst:.3f}")
    assert not fails, "\n".join(fails[:12])
    # the step: a second model with the same weights, .grad set to the folded gradients, no plan attached (hence no hints)
    twin = _build()
    for (n, p), q in zip(m.named_parameters(), twin.parameters()):
        q.grad = p.grad.detach().clone()
    del micro
    opt2 = Adam(twin.parameters(), lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    before = {n: p.detach().clone() for n, p in m.named_parameters() if p.dim() == 1}
    opt.skip_if = acc.skip_if
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    for (n, p), q in zip(m.named_parameters(), twin.parameters()):
        if p.dim() == 1:
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), f"{n}: the step behind the fold differs"
            assert not torch.equal(p.detach(), before[n]), f"{n}: the step did not move"


def _child(args, limit, **extra_env):
    """a fresh child under its own time limit; its exit status is checked before anything else runs"""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra_env)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, f"{args}: exit status {r.returncode}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-4000:]}"
    return r


def test_same_bits_under_deterministic_mode(tmp_path):
    """tests/accum_child.py det, YOLO_AMD_DETERMINISTIC=1: the same three micro-steps twice from the same weights -- bit-equal folded gradients
    and bit-equal parameters after the step"""
    out = tmp_path / "det.txt"
    _child([CHILD, "det", str(out)], 300, YOLO_AMD_DETERMINISTIC="1")
    assert out.read_text().splitlines()[-1] == "det: folded gradients and stepped parameters bit-equal over 52 tensors"


def test_two_ranks_one_all_reduce_per_group(tmp_path):
    """two ranks on one GPU over gloo (tests/accum_child.py ranks, started by torch.distributed.run), deterministic mode, K = 2, 2 images per
    micro-batch per rank, the shipped path: make_grad_reducer + GradAccumulator + Adam.step.  The reducer is the overlapped one and enqueued no
    bucket during the first micro-step; the replicas end bit-identical; the saved gradients lie within the chain bound (charged the cross-rank
    addition and the 1 / world multiplication) of the fp64 mean of the four raw micro-gradients, which each rank took from a second model
    instance without an arena"""
    out = tmp_path / "ranks.pt"
    port = 30500 + os.getpid() % 300
    _child(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
            CHILD, "ranks", str(out)], 600, YOLO_AMD_DETERMINISTIC="1")
    r = [torch.load(f"{out}.r{k}", weights_only=True) for k in (0, 1)]
    for d in r:
        assert d["reducer"] == "OverlappedGradAllReduce" and d["deterministic"] is True
        assert d["buckets_after_micro_1"] == 0 and d["buckets"] >= 2, "no bucket during the first micro-step, all of them during the second"
        assert d["skip"] == 0.0
    assert list(r[0]["grads"]) == list(r[1]["grads"]) and len(r[0]["grads"]) >= 26       # the 26 biases and the small weights
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


def test_train_py_accum_steps(tmp_path):
    """train.py --accum-steps 2 on the device: 8 synthetic images in batches of 2 -> two optimizer steps; the checkpoint records accum_steps"""
    ck = tmp_path / "ck"
    _child([os.path.join(ROOT, "yolo-v1_amd", "train.py"), "--device", "cuda", "--backbone", "yolov1", "--synthetic", "8", "--batch-size", "2",
            "--accum-steps", "2", "--epochs", "1", "--seed", "0", "--checkpoint-dir", str(ck)], 600)
    d = torch.load(ck / "yolo_latest.pth", map_location="cpu", weights_only=True)
    assert d["accum_steps"] == 2 and d["seed"] == 0
    assert {int(s["step"]) for s in d["optimizer_state_dict"]["state"].values()} == {2}
