"""Trainable ResNet trunk on the HIP engine (the reference's default run: ResNetBackbone(pretrained=True, freeze=False),
src/train.py:144; SURVEY 8a rows a4 x a12).  The building blocks are checked against stock torch on the CPU
(BatchNorm backward with and without the ReLU mask, MaxPool2d(3,2,1) backward), and the whole backward pass block by
block with teacher forcing: every bottleneck gets the GPU's own block input and incoming gradient, so bf16 noise does not
compound through 16 blocks of batch-statistics BatchNorm (see test_frozen_resnet_backbone_in_training_mode)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


@pytest.mark.parametrize("relu,stride,from_z,frozen", [(True, 1, False, False), (False, 1, False, False), (True, 2, False, False), (True, 1, True, False),
                                                        (True, 1, True, True), (False, 2, False, True)])
def test_batchnorm_backward_matches_autograd(relu, stride, from_z, frozen):
    from yolo import engine
    from yolo._hip import lib, check, ptr, stream
    torch.manual_seed(0)
    N, H, W, C = 4, 10, 12, 64
    z = _bf(torch.randn(N, C, H, W) * 1.5 + 0.3)
    dy = _bf(torch.randn(N, C, H, W))
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    zc = z.clone().requires_grad_(True)
    gc, bc = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm0, rv0 = torch.randn(C) * 0.4, torch.rand(C) + 0.5          # frozen: eval() mode, these ARE the statistics and stay as they are
    if frozen:
        yc = torch.nn.functional.batch_norm(zc, rm0, rv0, gc, bc, False, 0.1, 1e-5)
    else:
        yc = torch.nn.functional.batch_norm(zc, None, None, gc, bc, True, 0.1, 1e-5)
    if relu:
        yc = torch.relu(yc)
    yc.backward(dy)

    dev = torch.device("cuda")
    st = stream()
    za, ya, ga = engine.Act(N, H, W, C, 1, dev), engine.Act(N, H, W, C, 1, dev), engine.Act(N, H, W, C, 1, dev)
    za.interior().copy_(z.permute(0, 2, 3, 1).to(torch.bfloat16))
    ga.interior().copy_(dy.permute(0, 2, 3, 1).to(torch.bfloat16))
    from yolo._hip import BN_ACC_REPLICAS
    acc = torch.zeros(BN_ACC_REPLICAS * 2 * C, dtype=torch.float64, device=dev)
    ss = torch.empty(2 * C, dtype=torch.float32, device=dev)
    save = torch.empty(4 * C, dtype=torch.float32, device=dev)
    rm, rv = (rm0.to(dev), rv0.to(dev)) if frozen else (torch.zeros(C, device=dev), torch.ones(C, device=dev))
    g_d, b_d = gamma.to(dev), beta.to(dev)
    check(lib().yolo_batchnorm_train_fwd(za.p, N, H, W, C, 1, ptr(g_d), ptr(b_d), 1e-5, 0.1, ptr(rm), ptr(rv), None, 0, 1 if relu else 0, ptr(acc), ptr(ss),
                                         ya.p, 1, ptr(save), 2 if frozen else 0, st))
    if frozen:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
        assert lib().yolo_batchnorm_train_fwd(za.p, N, H, W, C, 1, ptr(g_d), ptr(b_d), 1e-5, 0.1, None, None, None, 0, 1, ptr(acc), ptr(ss), ya.p, 1, ptr(save), 2, st) != 0
    assert torch.equal(za.interior().float().cpu(), z.permute(0, 2, 3, 1))                 # z kept
    assert _rel(ya.interior().permute(0, 3, 1, 2), yc) < 0.01
    dz = engine.Act(N, H * stride, W * stride, C, 1, dev)
    dgam, dbet = torch.empty(C, device=dev), torch.empty(C, device=dev)
    coef = torch.empty(3 * C, device=dev)
    check(lib().yolo_batchnorm_bwd(ga.p, 1, ya.p if (relu and not from_z) else None, 1, za.p, 1, N, H, W, C, ptr(g_d), ptr(save), dz.p, dz.img_stride,
                                   stride * dz.row_stride, stride * dz.px_stride, dz.interior_off(), 1, (1 if from_z else 0) | (2 if frozen else 0), ptr(dgam), ptr(dbet),
                                   ptr(acc), ptr(coef), st))
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    got = dz.interior()[:, ::stride, ::stride, :].permute(0, 3, 1, 2)
    assert _rel(got, zc.grad) < 0.01, _rel(got, zc.grad)
    if stride == 2:
        assert float(dz.interior()[:, 1::2, :, :].abs().max()) == 0.0 and float(dz.interior()[:, :, 1::2, :].abs().max()) == 0.0
    assert _rel(dgam, gc.grad) < 0.005 and _rel(dbet, bc.grad) < 0.005
    mask = (yc > 0).float() if relu else torch.ones_like(dy)
    assert torch.equal(ga.interior().float().cpu().permute(0, 3, 1, 2), _bf(dy * mask)) or _rel(ga.interior().permute(0, 3, 1, 2), dy * mask) < 0.003


# (N, H, W, C, |mean| / std, relu, residual): the grid of bn.hip's reductions (pixel lanes per workgroup = 256 // min(C/8, 256), ~32 pixels per lane,
# at most 2048 workgroups along the pixels) at its edges
BN_EDGES = [(1, 3, 5, 64, 1.0, True, False),          # 15 pixels: fewer than the 32 pixel lanes of one workgroup
            (64, 7, 7, 2048, 1.0, True, False),       # one lane per workgroup, grid stride 98 > a 7x7 map (PixIter's image step sn > 0)
            (64, 7, 7, 64, 10.0, False, False),       # grid stride 128 > 49
            (2, 185, 187, 2048, 1.0, True, True),     # odd 185 x 187 map, 2048 workgroups (the cap), 34 pixels per lane: unrolled rounds + a tail
            (8, 28, 28, 256, 1.0, True, False), (8, 28, 28, 256, 10.0, True, False), (8, 28, 28, 256, 30.0, True, True),
            (2, 185, 187, 2048, 30.0, True, False)]


@pytest.mark.parametrize("N,H,W,C,ratio,relu,res", BN_EDGES)
def test_batchnorm_launches_within_fp64_bounds(N, H, W, C, ratio, relu, res):
    """one forward (batch statistics, running statistics, save_mean_invstd, output into a second buffer) and one backward (ReLU mask from y, masked dy
    stored back) against launch_ref's fp64 references, element by element within bounds derived from the kernels' arithmetic"""
    import launch_ref as lr
    from yolo import engine
    from yolo._hip import BN_ACC_REPLICAS, check, lib, ptr, stream
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(N * C + int(ratio))
    P = N * H * W
    std = torch.rand(C, device=dev, generator=g) + 0.5
    sign = torch.where(torch.rand(C, device=dev, generator=g) < 0.5, -1.0, 1.0)
    za, ya, ra, ga, dz = (engine.Act(N, H, W, C, 1, dev) for _ in range(5))
    za.interior().copy_((sign * ratio * std + std * torch.randn(N, H, W, C, device=dev, generator=g)).to(torch.bfloat16))
    ra.interior().copy_(torch.randn(N, H, W, C, device=dev, generator=g).to(torch.bfloat16))
    gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.5
    rm0, rv0 = torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    acc = torch.zeros(BN_ACC_REPLICAS * 2 * C, dtype=torch.float64, device=dev)
    ss, save = torch.empty(2 * C, device=dev), torch.full((4 * C,), float("nan"), device=dev)
    ya.interior().fill_(float("nan"))
    st = stream()
    check(lib().yolo_batchnorm_train_fwd(za.p, N, H, W, C, 1, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(rm), ptr(rv), ra.p if res else None, 1,
                                         1 if relu else 0, ptr(acc), ptr(ss), ya.p, 1, ptr(save), 0, st))
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    zz = za.interior().double().reshape(P, C)
    L = lr.bn_lane_pixels(P, C)
    mean, var, dm, dv = lr.bn_stats_ref(zz, L)
    R = lr.bn_fwd_ref(zz, mean, var, dm, dv, gamma, beta, 1e-5, ra.interior().double().reshape(P, C) if res else None, relu)
    fails, worst = [], {}
    tag = f"N {N} {H}x{W} C {C} |mean|/std {ratio}"
    worst["y"] = lr.check_values(R.y, R.bnd, ya.interior().reshape(P, C), "y", fails, tag)
    worst["save"] = lr.check_values(R.save.reshape(-1), R.save_bnd.reshape(-1), save, "save_mean_invstd", fails, tag)
    new_m, bm, new_v, bv = lr.bn_running_ref(rm0, rv0, mean, var, dm, dv, 0.1, P)
    worst["running"] = max(lr.check_values(new_m, bm, rm, "running_mean", fails, tag), lr.check_values(new_v, bv, rv, "running_var", fails, tag))
    assert float(ya.view()[:, 0].abs().max()) == 0.0 and float(ya.view()[:, :, -1].abs().max()) == 0.0          # halo untouched
    # backward
    ga.interior().copy_(torch.randn(N, H, W, C, device=dev, generator=g).to(torch.bfloat16))
    dy0 = ga.interior().double().reshape(P, C)
    dz.interior().fill_(float("nan"))
    dgam, dbet = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    coef = torch.empty(3 * C, device=dev)
    check(lib().yolo_batchnorm_bwd(ga.p, 1, ya.p if relu else None, 1, za.p, 1, N, H, W, C, ptr(gamma), ptr(save), dz.p, dz.img_stride, dz.row_stride,
                                   dz.px_stride, dz.interior_off(), 1, 0, ptr(dgam), ptr(dbet), ptr(acc), ptr(coef), st))
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    B = lr.bn_bwd_ref(dy0, zz, gamma, save.view(4, C), L, ya.interior().reshape(P, C) > 0 if relu else None)
    worst["dz"] = lr.check_values(B.dz, B.bnd, dz.interior().reshape(P, C), "dz", fails, tag)
    worst["dgamma"] = lr.check_values(B.dgamma, B.dgamma_bnd, dgam, "dgamma", fails, tag)
    worst["dbeta"] = lr.check_values(B.dbeta, B.dbeta_bnd, dbet, "dbeta", fails, tag)
    worst["masked dy"] = lr.check_values(B.g, torch.zeros_like(B.g), ga.interior().reshape(P, C), "masked dy", fails, tag)
    assert float(dz.view()[:, 0].abs().max()) == 0.0 and float(dz.view()[:, :, -1].abs().max()) == 0.0
    print(f"\n{tag}: worst |err| / bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()), flush=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H,W", [(16, 20), (15, 19), (7, 8)])
def test_maxpool3s2_backward_matches_autograd(H, W):
    from yolo import engine
    from yolo._hip import lib, check, stream, PoolDesc
    torch.manual_seed(1)
    N, C = 3, 16
    x = _bf(torch.relu(torch.randn(N, C, H, W)))
    x[:, :, 3:7, 4:8] = 0.0                 # ties: a window of equal values gives its gradient to the first position
    xc = x.clone().requires_grad_(True)
    yc = torch.nn.functional.max_pool2d(xc, 3, 2, 1)
    dy = _bf(torch.randn_like(yc))
    yc.backward(dy)
    dev = torch.device("cuda")
    xa, ga, dx = engine.Act(N, H, W, C, 1, dev), engine.Act(N, (H + 1) // 2, (W + 1) // 2, C, 1, dev), engine.Act(N, H, W, C, 1, dev)
    xa.interior().copy_(x.permute(0, 2, 3, 1).to(torch.bfloat16))
    ga.interior().copy_(dy.permute(0, 2, 3, 1).to(torch.bfloat16))
    pd = PoolDesc(N, H, W, C, 1, 1)
    check(lib().yolo_maxpool3s2_bwd(ctypes.byref(pd), xa.p, ga.p, dx.p, 1, stream()))
    got = dx.interior().float().cpu().permute(0, 3, 1, 2)
    assert torch.allclose(got, _bf(xc.grad), atol=2e-2, rtol=2e-2), (got - xc.grad).abs().max()


def _q(x):
    """straight-through bf16 rounding: where the GPU path stores a tensor"""
    return x + (_bf(x) - x).detach()


def _faithful_block(blk, x):
    """Bottleneck.forward with the GPU's storage roundings (conv outputs z and unit outputs y are bf16 buffers), so that
    ReLU gates are decided on the same values on both sides"""
    idn = x if blk.downsample is None else _q(blk.downsample[1](_q(blk.downsample[0](x))))
    o = _q(torch.relu(blk.bn1(_q(blk.conv1(x)))))
    o = _q(torch.relu(blk.bn2(_q(blk.conv2(o)))))
    return _q(torch.relu(blk.bn3(_q(blk.conv3(o))) + idn))


def _small_trunk():
    """the ResNet-50 trunk's structure with one bottleneck per stage (the plan only needs trunk[0..7])"""
    from yolo import resnet
    torch.manual_seed(3)
    mods = [nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, stride=2, padding=1),
            resnet._make_layer(64, 64, 2, 1), resnet._make_layer(256, 128, 1, 2), resnet._make_layer(512, 256, 1, 2), resnet._make_layer(1024, 512, 1, 2)]
    t = nn.Sequential(*mods)
    for m in t.modules():
        if isinstance(m, nn.BatchNorm2d):
            nn.init.uniform_(m.weight, 0.5, 1.5)
            nn.init.normal_(m.bias, 0.0, 0.2)
    return t


@pytest.mark.parametrize("mode,hw", [("train", (128, 128)), ("eval", (128, 128)), ("train", (104, 120))])
def test_trunk_backward_block_by_block(mode, hw):
    """hw (104, 120): a stem map of 52 x 60 that the direct 7x7 weight-gradient kernel's 8 x 16-pixel tiles do not cover (row-unfolded copy +
    generic kernel instead), odd maps further down (13 x 15, 7 x 8).  mode "eval": gradients through the trunk in eval() mode -- every BatchNorm normalises with its running statistics
    (batch_norm(training=False)), nothing is updated, the backward pass has no batch terms (reference: stock autograd through
    src/yolo/models.py:131-176 in any mode)."""
    from yolo import engine
    trunk = _small_trunk()
    if mode == "eval":
        torch.manual_seed(5)
        for m in trunk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    gpu = copy.deepcopy(trunk).cuda()
    gpu = gpu.train() if mode == "train" else gpu.eval()
    plan = engine.ResNetPlan(gpu)
    plan.trace = []
    N = 8
    x = torch.randn(N, 3, *hw)
    params = list(gpu.parameters())
    out = engine.ResNetTrainFunction.apply(plan, mode == "eval", x.cuda(), *params)
    assert out.shape == (N, 2048, 4, 4)            # both sizes end in a 4 x 4 map
    if mode == "eval":
        for (n, b), (_, b0) in zip(gpu.named_buffers(), trunk.named_buffers()):
            assert torch.equal(b.cpu(), b0), n          # running statistics and num_batches_tracked untouched
    gout = torch.randn_like(out)
    saved_blocks = None

    # run backward through autograd so that .grad is filled exactly as in training
    out.backward(gout)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    tr = {(k, what): g for (k, what, g) in plan.trace}
    # blocks in forward order with the Acts that the plan still holds
    cpu = copy.deepcopy(trunk)
    cpu = cpu.train() if mode == "train" else cpu.eval()
    with torch.no_grad():
        for m in cpu.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(_bf(m.weight))
    name_of = {id(p): n for n, p in gpu.named_parameters()}
    gpu_grads = {name_of[id(p)]: p.grad for p in params}
    worst = {}
    for li in range(4, 8):
        for bi, blk in enumerate(cpu[li]):
            u1x = plan._bufs[[k for k in plan._bufs if k[0] == ((li, bi, 1), "z")][0]]      # just to make sure the buffers exist
            # block input = the x Act of unit 1: recover it from the previous block's output / the pooled stem
            if (li, bi) == (4, 0):
                xin = plan._bufs[[k for k in plan._bufs if k[0] == "pool"][0]]
            else:
                pli, pbi = (li, bi - 1) if bi > 0 else (li - 1, len(cpu[li - 1]) - 1)
                xin = plan._bufs[[k for k in plan._bufs if k[0] == ((pli, pbi, 3), "y")][0]]
            xb = xin.interior().float().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            blk.zero_grad()
            yb = _faithful_block(blk, xb)
            yg = plan._bufs[[k for k in plan._bufs if k[0] == ((li, bi, 3), "y")][0]].interior().float().cpu().permute(0, 3, 1, 2)
            assert _rel(yg, yb) < 0.02, ("forward", li, bi, _rel(yg, yb))
            yb.backward(tr[((li, bi), "gout")].cpu())
            r = _rel(tr[((li, bi), "gx")], xb.grad)
            worst[("gx", li, bi)] = r
            for n, p in blk.named_parameters():
                full = f"{li}.{bi}.{n}"
                r = _rel(gpu_grads[full], p.grad)
                worst[(full,)] = r
    # measured 0.2-2.2 % (largest in the 4x4 stage, 128 samples per channel; varies with the launch plans the tuner picks)
    assert max(worst.values()) < 0.04, {k: round(v, 4) for k, v in worst.items() if v >= 0.04}
    # stem: conv1 + bn1 + relu + maxpool, teacher-forced with the GPU's gradient wrt the pooled map
    xs = _bf(x).clone()
    stem = nn.Sequential(cpu[0], cpu[1], cpu[2], cpu[3])
    stem.zero_grad()
    ys = cpu[3](_q(torch.relu(cpu[1](_q(cpu[0](xs))))))
    ys.backward(tr[((4, 0), "gx")].cpu())
    for n, p in [("0.weight", cpu[0].weight), ("1.weight", cpu[1].weight), ("1.bias", cpu[1].bias)]:
        r = _rel(gpu_grads[n], p.grad)
        assert r < 0.03, (n, r)


def test_resnet_yolo_training_step_runs_and_learns():
    """YOLOv1(ResNetBackbone(freeze=False)) -- the reference's default training model -- takes optimizer steps on the engine."""
    from yolo import YOLOv1, ResNetBackbone, YOLOLoss
    from yolo.optim import Adam
    from yolo.dataset import SyntheticYOLODataset
    torch.manual_seed(5)
    model = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=False)).cuda().train()
    ds = SyntheticYOLODataset(4, seed=0)
    x = torch.stack([ds[i][0] for i in range(4)]).cuda()
    t = torch.stack([ds[i][1] for i in range(4)]).cuda()
    crit = YOLOLoss()
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=5e-4, max_grad_norm=10.0)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss, _ = crit(model(x), t)
        loss.backward()
        assert all(p.grad is not None for p in model.backbone.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    # the first three losses repeat run to run (13.1, 10.8, 7.4); from then on the trajectory of this random-init network is chaotic
    # (fp32 atomics in the weight gradients are enough to move step 5 anywhere between 3.8 and 14.8), so the check is on the early steps
    assert all(l == l and l < 1e4 for l in losses) and losses[2] < 0.8 * losses[0] and min(losses) < 0.7 * losses[0], losses
    # two forwards before a backward would share activation buffers: refused loudly, not computed wrongly
    l1, _ = crit(model(x), t)
    l2, _ = crit(model(x), t)
    with pytest.raises(RuntimeError, match="one forward in flight"):
        l1.backward()
    l2.backward()


def test_statistics_from_the_conv_epilogue():
    """yolo_igemm_desc.bn_stats: the conv's epilogue accumulates BatchNorm's per-channel sums of the values it stores, so
    yolo_batchnorm_train_fwd(stats_ready = 1) skips its pass over z.  Checked unit by unit against the mean / variance of the
    stored z itself (the first call of each problem also goes through the tuner, which must not accumulate twice), and the
    separate-pass mode must agree on the first unit's y (same input, statistics equal to fp32 rounding).  Whole-trunk
    outputs of the two modes are NOT compared: a one-ulp difference grows ~10x per bottleneck in this random-init net."""
    from yolo import engine
    trunk = _small_trunk().cuda().train()
    x = torch.randn(8, 3, 128, 128, device="cuda")
    first_y = []
    for flag in (True, False):
        t = copy.deepcopy(trunk)
        plan = engine.ResNetPlan(t)
        engine.BN_STATS_IN_CONV = flag
        try:
            _, saved = plan.forward_train(x)
            for rep in range(2):                       # second pass: every problem is tuned by now
                if rep:
                    _, saved = plan.forward_train(x)
                for (li, bi, u1, u2, u3, ud) in saved["blocks"]:
                    for u in (u1, u2, u3, ud):
                        if u is None:
                            continue
                        z = u.z.interior().float()
                        C = z.shape[-1]
                        mean = z.mean(dim=(0, 1, 2))
                        var = z.var(dim=(0, 1, 2), unbiased=False)
                        st = u.stats
                        assert _rel(st[:C], mean) < 1e-4 + 1e-4 * float(mean.abs().max() == 0), (flag, u.tag, "mean")
                        assert _rel(st[C:2 * C], torch.rsqrt(var + 1e-5)) < 1e-4, (flag, u.tag, "invstd", _rel(st[C:2 * C], torch.rsqrt(var + 1e-5)))
            first_y.append(saved["blocks"][0][2].y.interior().clone())
        finally:
            engine.BN_STATS_IN_CONV = True
    # same input, statistics equal to rounding: the first unit's activation agrees up to single bf16 ulps (the tuner may run
    # the two modes through different launch plans, e.g. split-K, which changes z in its last bit)
    assert _rel(first_y[1], first_y[0]) < 1e-3
