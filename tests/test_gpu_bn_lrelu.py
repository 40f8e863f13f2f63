"""BatchNorm variant of the YOLOv1 network on the device: the two entries of bn.hip (yolo_batchnorm_train_fwd_lrelu, yolo_batchnorm_bwd_lrelu)
against the fp64 references of tests/bn_lrelu_ref.py, the fused pool against the unfused launches, engine.BNPlan unit by unit with teacher forcing,
the folded eval() path bit for bit against the plain network, a learning run against the stock CPU curve, and a training step of YOLOv1."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_lrelu_ref as br
import launch_ref as lr
import pretrain_scale_ref as ps

pytestmark = pytest.mark.gpu
SLOPE = 0.1


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _q(x):
    """straight-through bf16 rounding: where the GPU path stores a tensor"""
    return x + (_bf(x) - x).detach()


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def _clean(a):
    """the halo ring and the guard bands of an Act hold what they held: zeros"""
    v, h = a.view(), a.halo
    ring = float(v[:, :h].abs().max()) + float(v[:, -h:].abs().max()) + float(v[:, :, :h].abs().max()) + float(v[:, :, -h:].abs().max())
    lo = a.t.storage_offset()
    return ring == 0.0 and float(a.store[:lo].abs().max()) == 0.0 and float(a.store[lo + a.t.numel():].abs().max()) == 0.0


class _Case:
    """operands of one layer on the device: z with the given |mean| / std per channel, affine parameters, running statistics, scratch"""

    def __init__(self, N, H, W, C, ratio, seed=0):
        from yolo import engine
        from yolo._hip import BN_ACC_REPLICAS
        self.shape = (N, H, W, C)
        dev = self.dev = torch.device("cuda")
        g = self.g = torch.Generator(device=dev).manual_seed(N * C + int(ratio) + seed)
        std = torch.rand(C, device=dev, generator=g) + 0.5
        sign = torch.where(torch.rand(C, device=dev, generator=g) < 0.5, -1.0, 1.0)
        self.za = engine.Act(N, H, W, C, 1, dev)
        self.za.interior().copy_((sign * ratio * std + std * torch.randn(N, H, W, C, device=dev, generator=g)).to(torch.bfloat16))
        self.z0 = self.za.store.clone()
        self.gamma, self.beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.5
        self.rm0, self.rv0 = torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5
        self.acc = torch.zeros(BN_ACC_REPLICAS * 2 * C, dtype=torch.float64, device=dev)
        self.ss, self.coef = torch.empty(2 * C, device=dev), torch.empty(3 * C, device=dev)

    def out(self, pool):
        from yolo import engine
        N, H, W, C = self.shape
        a = engine.Act(N, H // 2 if pool else H, W // 2 if pool else W, C, 1, self.dev)
        a.interior().fill_(float("nan"))
        return a

    def fwd(self, out, pool, frozen=False):
        """-> (rc, running_mean, running_var, save)"""
        from yolo._hip import lib, ptr, stream
        N, H, W, C = self.shape
        rm, rv = self.rm0.clone(), self.rv0.clone()
        save = torch.full((4 * C,), float("nan"), device=self.dev)
        rc = lib().yolo_batchnorm_train_fwd_lrelu(self.za.p, N, H, W, C, 1, ptr(self.gamma), ptr(self.beta), 1e-5, 0.1, ptr(rm), ptr(rv), SLOPE, 1 if pool else 0,
                                                  ptr(self.acc), ptr(self.ss), out.p, 1, ptr(save), 2 if frozen else 0, stream())
        torch.cuda.synchronize()
        return rc, rm, rv, save

    def bwd(self, ga, save, pool, dz, strides, frozen=False):
        from yolo._hip import check, lib, ptr, stream
        N, H, W, C = self.shape
        dg, db = torch.full((C,), float("nan"), device=self.dev), torch.full((C,), float("nan"), device=self.dev)
        check(lib().yolo_batchnorm_bwd_lrelu(ga.p, 1, self.za.p, 1, N, H, W, C, ptr(self.gamma), ptr(save), SLOPE, 1 if pool else 0, dz.p, *strides,
                                             1 if frozen else 0, ptr(dg), ptr(db), ptr(self.acc), ptr(self.coef), stream()), "yolo_batchnorm_bwd_lrelu")
        torch.cuda.synchronize()
        assert float(self.acc.abs().max()) == 0.0, "acc2c is zero on return"
        return dg, db


# (N, H, W, C): one pooled pixel; 24 channel groups (16 idle threads per workgroup); an odd map (pool2 = 1 is refused); a typical pooled map;
# the pixel-axis grid cap of 2048 workgroups (un-pooled: 2 pixel lanes per workgroup, 138368 pixels)
SHAPES = [(1, 2, 2, 64), (2, 6, 10, 192), (64, 7, 7, 1024), (3, 14, 18, 1024), (4, 184, 188, 1024)]
CASES = [(s, r, p, False, 1) for s in SHAPES for r in (1.0, 10.0) for p in (0, 1) if not (p and (s[1] % 2 or s[2] % 2))]
CASES += [((3, 14, 18, 1024), 1.0, 1, True, 1), ((2, 6, 10, 192), 1.0, 0, True, 1),      # frozen: running statistics, no batch terms
          ((2, 6, 10, 192), 1.0, 0, False, 2)]                                            # dz zero-stuffed on the input grid of a stride-2 conv


@pytest.mark.parametrize("shape,ratio,pool,frozen,stride", CASES)
def test_entries_within_fp64_bounds(shape, ratio, pool, frozen, stride):
    """an unfused forward launch gives the device's decisions (mask = stored y > 0, arg-max of the stored y); then the launch under test, forward and
    backward, element by element within the bounds of bn_lrelu_ref"""
    from yolo import engine
    N, H, W, C = shape
    P = N * H * W
    c = _Case(N, H, W, C, ratio)
    tag = f"N {N} {H}x{W} C {C} |mean|/std {ratio} pool2 {pool} frozen {frozen} stride {stride}"
    fails, worst = [], {}
    ya = c.out(False)
    rc, rm, rv, save = c.fwd(ya, False, frozen)
    assert rc == 0 and float(c.acc.abs().max()) == 0.0
    assert torch.equal(c.za.store, c.z0), "z is kept"
    assert _clean(ya)
    z = c.za.interior().double()
    if frozen:
        mean, var = c.rm0.double(), c.rv0.double()
        dm = dv = torch.zeros_like(mean)
        assert torch.equal(rm, c.rm0) and torch.equal(rv, c.rv0), "running statistics untouched"
    else:
        mean, var, dm, dv = lr.bn_stats_ref(z.reshape(P, C), lr.bn_lane_pixels(P, C))
        new_m, bm, new_v, bv = lr.bn_running_ref(c.rm0, c.rv0, mean, var, dm, dv, 0.1, P)
        worst["running"] = max(lr.check_values(new_m, bm, rm, "running_mean", fails, tag), lr.check_values(new_v, bv, rv, "running_var", fails, tag))
    mask = ya.interior() > 0
    R = br.fwd_ref(z, mean, var, dm, dv, c.gamma, c.beta, 1e-5, SLOPE, mask=mask)
    worst["y"] = lr.check_values(R.y, R.bnd, ya.interior(), "y", fails, tag)
    worst["save"] = lr.check_values(R.save.reshape(-1), R.save_bnd.reshape(-1), save, "save_mean_invstd", fails, tag)
    sel = None
    if pool:
        sel = br.first_argmax(ya.interior().double())
        yp = c.out(True)
        rc, rm2, rv2, save = c.fwd(yp, True, frozen)
        assert rc == 0 and float(c.acc.abs().max()) == 0.0 and torch.equal(c.za.store, c.z0) and _clean(yp)
        Rp = br.fwd_ref(z, mean, var, dm, dv, c.gamma, c.beta, 1e-5, SLOPE, mask=mask, sel=sel, pool=True)
        worst["pooled y"] = lr.check_values(Rp.y, Rp.bnd, yp.interior(), "pooled y", fails, tag)
        worst["save (pool2)"] = lr.check_values(R.save.reshape(-1), R.save_bnd.reshape(-1), save, "save_mean_invstd (pool2)", fails, tag)
    elif H % 2 or W % 2:
        from yolo._hip import E_UNSUPPORTED
        yp = engine.Act(N, H // 2, W // 2, C, 1, c.dev)
        assert c.fwd(yp, True, frozen)[0] == E_UNSUPPORTED, "pool2 = 1 on an odd map is refused"
        assert float(yp.store.abs().max()) == 0.0 and float(c.acc.abs().max()) == 0.0, "and launches nothing"
    # backward
    ga = c.out(pool)
    ga.interior().copy_(torch.randn(ga.interior().shape, device=c.dev, generator=c.g).to(torch.bfloat16))
    dz = engine.Act(N, H * stride, W * stride, C, 1, c.dev)
    if stride == 1:
        dz.interior().fill_(float("nan"))
    dg, db = c.bwd(ga, save, pool, dz, (dz.img_stride, stride * dz.row_stride, stride * dz.px_stride, dz.interior_off()), frozen)
    Pd = P // 4 if pool else P
    B = br.bwd_ref(ga.interior().double(), z, c.gamma, save.view(4, C), lr.bn_lane_pixels(Pd, C), SLOPE, mask, sel, frozen)
    worst["dz"] = lr.check_values(B.dz, B.bnd, dz.interior()[:, ::stride, ::stride].contiguous(), "dz", fails, tag)
    worst["dgamma"] = lr.check_values(B.dgamma, B.dgamma_bnd, dg, "dgamma", fails, tag)
    worst["dbeta"] = lr.check_values(B.dbeta, B.dbeta_bnd, db, "dbeta", fails, tag)
    assert _clean(dz) and _clean(ga) and torch.equal(c.za.store, c.z0)
    if stride == 2:
        assert float(dz.interior()[:, 1::2].abs().max()) == 0.0 and float(dz.interior()[:, :, 1::2].abs().max()) == 0.0, "odd rows / columns stay zero"
    print(f"\n{tag}: worst |err| / bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()), flush=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [(2, 6, 10, 192), (3, 14, 18, 1024)])
def test_fused_pool_against_unfused_launches(shape):
    """pool2 = 1 against pool2 = 0 + yolo_maxpool2_fwd, and against yolo_maxpool2_bwd_lrelu(slope = 1) + pool2 = 0 backward, on the same inputs: the
    pooled y bit-equal; dz, dgamma, dbeta within the sum of the two paths' bounds (their summation grids differ)"""
    from yolo import engine
    from yolo._hip import PoolDesc, check, lib, stream
    N, H, W, C = shape
    P = N * H * W
    c = _Case(N, H, W, C, 1.0, seed=7)
    ya, yu, yf = c.out(False), c.out(True), c.out(True)
    rc, _, _, save = c.fwd(ya, False)
    assert rc == 0
    pd = PoolDesc(N, H, W, C, 1, 1)
    check(lib().yolo_maxpool2_fwd(ctypes.byref(pd), ya.p, yu.p, stream()), "yolo_maxpool2_fwd")
    rc, _, _, save_f = c.fwd(yf, True)
    assert rc == 0 and torch.equal(save.view(torch.int32), save_f.view(torch.int32))
    assert torch.equal(yu.store.view(torch.int16), yf.store.view(torch.int16)), "the pooled y is bit-equal"
    ga = c.out(True)
    ga.interior().copy_(torch.randn(ga.interior().shape, device=c.dev, generator=c.g).to(torch.bfloat16))
    gy, dzu, dzf = (engine.Act(N, H, W, C, 1, c.dev) for _ in range(3))
    check(lib().yolo_maxpool2_bwd_lrelu(ctypes.byref(pd), ya.p, ga.p, 1.0, gy.p, stream()), "yolo_maxpool2_bwd_lrelu")
    st = (dzu.img_stride, dzu.row_stride, dzu.px_stride, dzu.interior_off())
    dgu, dbu = c.bwd(gy, save, False, dzu, st)
    dgf, dbf = c.bwd(ga, save, True, dzf, st)
    z, mask = c.za.interior().double(), ya.interior() > 0
    sel = br.first_argmax(ya.interior().double())
    assert torch.equal(gy.interior().double(), br.scatter(ga.interior().double(), sel)), "the unfused pool backward routes to the same positions"
    Bu = br.bwd_ref(gy.interior().double(), z, c.gamma, save.view(4, C), lr.bn_lane_pixels(P, C), SLOPE, mask)
    Bf = br.bwd_ref(ga.interior().double(), z, c.gamma, save.view(4, C), lr.bn_lane_pixels(P // 4, C), SLOPE, mask, sel)
    for what, a, b, bound in (("dz", dzf.interior(), dzu.interior(), Bu.bnd + Bf.bnd), ("dgamma", dgf, dgu, Bu.dgamma_bnd + Bf.dgamma_bnd),
                              ("dbeta", dbf, dbu, Bu.dbeta_bnd + Bf.dbeta_bnd)):
        ratio = ((a.double() - b.double()).abs() / bound).max()
        print(f"{shape} fused vs unfused {what}: worst |difference| / (sum of bounds) {float(ratio):.3g}")
        assert float(ratio) <= 1.0 and bool(torch.isfinite(a).all()), what


# ---------------------------------------------------------------------------------------------------------------------------------
# the executor, unit by unit
# ---------------------------------------------------------------------------------------------------------------------------------
def _stack():
    from yolo.models import _conv_act
    torch.manual_seed(3)
    mods = (_conv_act(3, 64, 7, 2, 3, bn=True) + [nn.MaxPool2d(2, 2)] + _conv_act(64, 192, 3, 1, 1, bn=True) + [nn.MaxPool2d(2, 2)]
            + _conv_act(192, 128, 1, bn=True) + _conv_act(128, 256, 3, 1, 1, bn=True) + [nn.MaxPool2d(2, 2)]
            + _conv_act(256, 256, 3, 2, 1, bn=True) + _conv_act(256, 256, 3, 1, 1, bn=True))
    t = nn.Sequential(*mods)
    for m in t.modules():
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.normal_(m.bias, 0.0, 0.2)
    return t


@pytest.mark.parametrize("mode,hw", [("train", (64, 96)), ("eval", (64, 96)), ("train", (72, 104)), ("eval", (72, 104))])
def test_chain_backward_unit_by_unit(mode, hw):
    """engine.BNPlan on 7x7/s2 + pool, 3x3 + pool, 1x1, 3x3 + pool, 3x3/s2, 3x3 with teacher forcing: every unit gets the device's own input and
    incoming gradient, the CPU side (stock modules, bf16-rounded weights) rounds where the device stores.  (64, 96): every pool fused, the stem map
    32 x 48 takes the direct weight-gradient kernel; (72, 104): the 9 x 13 map takes the unfused pool, the 36 x 52 stem map the generic path.
    The measured worst relative L2 values are printed, and recorded below and in DESIGN.md."""
    from yolo import engine
    stack = _stack()
    if mode == "eval":
        torch.manual_seed(5)
        for m in stack.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    gpu = copy.deepcopy(stack).cuda()
    gpu = gpu.train() if mode == "train" else gpu.eval()
    plan = engine.BNPlan.from_modules(gpu)
    plan.trace = []
    N = 8
    torch.manual_seed(11)
    x = torch.randn(N, 3, *hw)
    out = engine.BNTrainFunction.apply(plan, mode == "eval", x.cuda(), *plan.params)
    h, w = hw[0] // 32, hw[1] // 32
    assert out.shape == (N, 256, h, w)
    out.backward(torch.randn_like(out))
    torch.cuda.synchronize()
    params = dict(gpu.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    fused = [k[0][0] for k in plan._bufs if isinstance(k[0], tuple) and k[0][1] == "yp"]
    assert fused == ([] if hw == (64, 96) else [3]), "which units took the unfused pool"
    tr = {(i, what): g for (i, what, g) in plan.trace}
    cpu = copy.deepcopy(stack)
    cpu = cpu.train() if mode == "train" else cpu.eval()
    with torch.no_grad():
        for m in cpu.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(_bf(m.weight))
    units, mods, i = [], list(cpu), 0
    while i < len(mods):
        pool = i + 3 < len(mods) and isinstance(mods[i + 3], nn.MaxPool2d)
        units.append((i, mods[i], mods[i + 1], pool))
        i += 4 if pool else 3

    def buf(key):
        return plan._bufs[[k for k in plan._bufs if k[0] == key][0]]

    worst = {}
    for u, (mi, conv, bn, pool) in enumerate(units):
        if u == 0:
            xin = _bf(x).clone()
        else:
            prev = (u - 1, "yp") if [k for k in plan._bufs if k[0] == (u - 1, "yp")] else (u - 1, "y")
            xin = buf(prev).interior().float().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        cpu.zero_grad()
        y = _q(torch.nn.functional.leaky_relu(bn(_q(conv(xin))), SLOPE))
        if pool:
            y = torch.nn.functional.max_pool2d(y, 2)
        got = buf((u, "yp") if [k for k in plan._bufs if k[0] == (u, "yp")] else (u, "y")).interior().float().cpu().permute(0, 3, 1, 2)
        assert _rel(got, y) < 0.02, ("forward", u, _rel(got, y))
        y.backward(tr[(u, "gout")].cpu())
        if u > 0:
            worst[("gx", u)] = _rel(tr[(u, "gx")], xin.grad)
        for n, p in ((f"{mi}.weight", conv.weight), (f"{mi + 1}.weight", bn.weight), (f"{mi + 1}.bias", bn.bias)):
            worst[(n,)] = _rel(params[n].grad, p.grad)
        g_bn = dict(gpu.named_buffers())
        for n, b in ((f"{mi + 1}.running_mean", bn.running_mean), (f"{mi + 1}.running_var", bn.running_var)):
            if mode == "train":
                assert _rel(g_bn[n], b) < 1e-3 and not torch.equal(b, dict(stack.named_buffers())[n]), n          # updated, as stock torch updates them
            else:
                assert torch.equal(g_bn[n].cpu(), dict(stack.named_buffers())[n]), n                               # untouched
        assert int(g_bn[f"{mi + 1}.num_batches_tracked"]) == (1 if mode == "train" else 0)
    stem = {k: v for k, v in worst.items() if k[0] in ("0.weight", "1.weight", "1.bias")}
    rest = {k: v for k, v in worst.items() if k not in stem}
    print(f"\n{mode} {hw}: worst relative L2  stem {max(stem.values()):.4f}  units {max(rest.values()):.4f}  "
          + "  ".join(f"{'.'.join(map(str, k))} {v:.4f}" for k, v in worst.items()), flush=True)
    # measured on an MI355X: units 0.0023 - 0.0032 (train) / 0.0023 (eval), stem 0.0017 - 0.0021; the data gradients sit at 0.0023 - 0.0024 in every
    # unit (the bf16 rounding of the stored gradient), the weight gradients vary with the samples per channel.  test_trunk_backward_block_by_block allows a
    # whole bottleneck 0.04 and the ResNet stem 0.03; one unit is far below that, so the bounds are 2 x the measured worst
    assert max(rest.values()) < 0.0064, {k: round(v, 4) for k, v in rest.items() if v >= 0.0064}
    assert max(stem.values()) < 0.0042, {k: round(v, 4) for k, v in stem.items() if v >= 0.0042}


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def test_eval_inference_is_the_plain_network_with_folded_weights_bit_for_bit():
    from yolo import YOLOv1, YOLOv1Backbone, engine
    torch.manual_seed(0)
    model = YOLOv1(backbone=YOLOv1Backbone(batch_norm=True))
    with torch.no_grad():
        for m in model.backbone.features:
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.8, 1.6)
                m.bias.normal_(0.0, 0.2)
    model = model.cuda().eval()
    plain = YOLOv1().cuda().eval()
    with torch.no_grad():
        src = list(model.backbone.features)
        dst = [m for m in plain.backbone.features if isinstance(m, nn.Conv2d)]
        pairs = [(src[i], src[i + 1]) for i in range(len(src)) if isinstance(src[i], nn.Conv2d)]
        assert len(pairs) == len(dst) == 24
        for (conv, bn), d in zip(pairs, dst):
            w, b = engine.ResNetPlan._fold(conv, bn)
            d.weight.copy_(w)
            d.bias.copy_(b)
        plain.head.load_state_dict(model.head.state_dict())
        x = torch.randn(2, 3, 448, 448, device="cuda")
        assert model._fusable()
        got, want = model(x), plain(x)
        assert got.shape == (2, 7, 7, 30) and bool(torch.isfinite(got).all())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the same plan on the same operands"
        assert [(L.kind, L.Cout, L.K, L.stride) for L in model.hip_plan().layers] == [(L.kind, L.Cout, L.K, L.stride) for L in plain.hip_plan().layers]
        img = torch.randint(0, 256, (2, 300, 400, 3), dtype=torch.uint8, device="cuda")
        g8, w8 = model.forward_uint8(img), plain.forward_uint8(img)
        assert g8.shape == (2, 7, 7, 30) and torch.equal(g8.view(torch.int32), w8.view(torch.int32))
        # the folded operands follow a buffer that changes
        model.backbone.features[1].running_mean.add_(0.25)
        assert not torch.equal(model(x), got)


def _bn_learning_loop(device):
    from yolo import SoftmaxCrossEntropy, YOLOv1Classifier
    x, y = ps.learn_set(device)
    torch.manual_seed(0)
    m = YOLOv1Classifier(4, batch_norm=True).to(device).train()
    if device == "cuda":
        from yolo.optim import SGD
        opt = SGD(m.parameters(), lr=ps.LEARN_LR, max_grad_norm=ps.CLIP)
    else:
        opt = torch.optim.SGD(m.parameters(), lr=ps.LEARN_LR)
    crit, losses = SoftmaxCrossEntropy(), []
    for _ in range(ps.LEARN_STEPS):
        opt.zero_grad(set_to_none=True)
        loss, parts = crit(m(x), y)
        loss.backward()
        if device != "cuda":
            torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=ps.CLIP)
        opt.step()
        losses.append(parts)
    return [p["total"] for p in losses]


def test_learning_from_the_default_initialisation_on_the_device():
    """YOLOv1Classifier(4, batch_norm=True), PyTorch's default initialisation, the 8-image batch, plain SGD lr 1e-3, clip 10, 30 steps on the device
    against the stock CPU curve computed here (the CPU's: 1.3859 -> 0.0720; the plain network stays at ln 4 = 1.386): the margins of
    test_learning_from_he_init_on_the_device -- first loss within 3 %, last at most 1.25 x the CPU's"""
    cpu = _bn_learning_loop("cpu")
    dev = _bn_learning_loop("cuda")
    print(f"learning with BatchNorm: device first {dev[0]:.4f} last {dev[-1]:.4f}; stock CPU path first {cpu[0]:.4f} last {cpu[-1]:.4f}")
    assert len(dev) == ps.LEARN_STEPS and np.isfinite(dev).all()
    assert abs(dev[0] - cpu[0]) <= 0.03 * cpu[0], dev[0]
    assert dev[-1] <= 1.25 * cpu[-1], dev


def test_training_step_of_yolov1_and_the_refused_cases(monkeypatch):
    from yolo import GradAccumulator, YOLOLoss, YOLOv1, YOLOv1Backbone, engine
    from yolo.config import CONFIG
    from yolo.dataset import SyntheticYOLODataset
    from yolo.optim import SGD
    torch.manual_seed(5)
    model = YOLOv1(backbone=YOLOv1Backbone(batch_norm=True)).cuda().train()
    ds = SyntheticYOLODataset(4, seed=0)
    x = torch.stack([ds[i][0] for i in range(4)]).cuda()
    t = torch.stack([ds[i][1] for i in range(4)]).cuda()
    crit = YOLOLoss()
    opt = SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4, max_grad_norm=10.0)
    plans = model.hip_plans()
    assert not model._fusable() and len(plans) == 1 and plans[0] is model.head_plan() and [L.kind for L in plans[0].layers] == ["flatten", "fc", "fc"]
    opt.attach_plan(model.head_plan())
    acc = GradAccumulator(model, 2)
    head_ids = {id(p) for p in model.head.parameters()}
    assert len(acc._arenas) == 1 and acc._arenas[0][0] is plans[0] and {id(p) for p in acc._rest} == {id(p) for p in model.backbone.parameters()}
    losses = []
    for step in range(4):
        opt.zero_grad(set_to_none=True)
        group = 0.0
        for k in range(2):
            acc.before_backward()
            loss, parts = crit(model(x[2 * k: 2 * k + 2]), t[2 * k: 2 * k + 2])
            loss.backward()
            if step == 0:
                assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
                lo, hi = plans[0].arena.data_ptr(), plans[0].arena.data_ptr() + 4 * plans[0].arena.numel()
                # the head's Linear layers ran on the engine: their gradients are views of its plan's arena, which only Plan.backward writes
                assert all(lo <= p.grad.data_ptr() < hi for p in model.parameters() if id(p) in head_ids)
            assert acc.after_backward(getattr(parts, "device_flag", None)) is (k == 1)
            group += float(loss.detach()) / 2
        opt.skip_if = acc.skip_if
        opt.step()
        losses.append(group)
    print("YOLOv1 with a BatchNorm backbone, 4 steps:", [round(v, 4) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(int(m.num_batches_tracked) == 8 for m in model.backbone.features if isinstance(m, nn.BatchNorm2d))
    # refused, each with its message
    l1, _ = crit(model(x[:2]), t[:2])
    l2, _ = crit(model(x[:2]), t[:2])
    with pytest.raises(RuntimeError, match="one forward in flight"):
        l1.backward()
    l2.backward()
    with pytest.raises(NotImplementedError, match="no gradient with respect to its input"):
        model(x[:2].clone().requires_grad_(True))
    monkeypatch.setattr(CONFIG, "DETERMINISTIC", True)
    with pytest.raises(NotImplementedError, match="DETERMINISTIC does not cover a BatchNorm backbone"):
        model(x[:2])
    monkeypatch.setattr(CONFIG, "DETERMINISTIC", False)
    # eval() with gradients: running statistics, nothing updated
    model.eval()
    before = {n: b.clone() for n, b in model.named_buffers()}
    loss, _ = crit(model(x[:2]), t[:2])
    loss.backward()
    assert all(torch.equal(b, before[n]) for n, b in model.named_buffers())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.backbone.parameters())
    assert engine.BNPlan is type(model.backbone._bn.bn_plan)
