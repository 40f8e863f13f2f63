"""GPU parity of the whole YOLOv1 (24-conv backbone + FC head) forward and training step.

Oracle: (a) the reference model's own output on a fixed image with fixed weights
(tests/golden/backbone_full.npz, produced by running mattiaskvist/yolo-v1's YOLOv1 on the CPU);
(b) stock torch.nn on the host CPU with the same parameters (the reference's arithmetic for these
layers).  bf16 storage / fp32 accumulate through 26 layers: tolerance 3% of the output scale
(measured error is ~0.5%).
"""

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    from yolo import YOLOv1
    m = YOLOv1()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.yolov1_state_dict().items()}, strict=True)
    return m


def _rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def test_forward_matches_reference_fixture(model, golden):
    g = golden("backbone_full.npz")
    m = model.cuda().eval()
    with torch.no_grad():
        y = m(torch.from_numpy(synth.synth_images(1, 0)).cuda())
        y2 = m(torch.from_numpy(synth.synth_images(2, 7)).cuda())
        feat = m.backbone(torch.from_numpy(synth.synth_images(1, 0)).cuda())
    assert y.shape == (1, 7, 7, 30) and feat.shape == (1, 1024, 7, 7)
    for got, ref, what in ((y, g["y"], "y"), (y2, g["y2"], "y2"), (feat, g["feat"], "feat")):
        r = _rel(got, torch.from_numpy(ref))
        assert r < 0.03, (what, r)
        assert (got.cpu() - torch.from_numpy(ref)).abs().max() < 0.15 * np.abs(ref).max(), what
    model.cpu()


def test_train_step_gradients_vs_gate_forced_cpu_autograd(model):
    """loss + backward on 2 images: EVERY parameter gradient vs torch CPU autograd on a network whose LeakyReLU gates and
    max-pool selections are taken from the activations the GPU pass stored.  Free-running fp32 autograd differs from a bf16
    pipeline mainly through gates of pre-activations ~0 that flip (each flip changes a unit's gradient x10), which says
    nothing about the kernels; with the gates forced, the remaining difference is bf16 storage of activations / gradients
    and accumulation order, and the bound is tight: relative L2 error < 2 % per parameter tensor
    (reference: src/yolo/models.py:256-276, src/yolo/loss.py:87-172)."""
    import copy
    import torch.nn as nn
    import torch.nn.functional as F
    from yolo import YOLOLoss
    from test_gpu_layers import _bf
    N = 2
    x = torch.from_numpy(synth.synth_images(N, 3))
    t = torch.from_numpy(synth.synth_targets(N, 21, max_obj=4))
    crit = YOLOLoss()
    m = model.cuda().eval()                      # eval: dropout off
    plan = m.hip_plan()
    plan.debug_keep = True
    try:
        m.zero_grad()
        lg, _ = crit(m(x.cuda()), t.cuda())
        lg.backward()
        torch.cuda.synchronize()
        ws, fc_saved = plan.last
    finally:
        plan.debug_keep = False
        plan.last = None

    def nchw(act):
        return act.interior().float().cpu().permute(0, 3, 1, 2).contiguous()

    def q(v):                                    # straight-through bf16 rounding = a stored activation
        return v + (_bf(v) - v).detach()

    ref = copy.deepcopy(model).cpu().eval()
    mods = list(ref.backbone.features) + list(ref.head)
    with torch.no_grad():
        for mod in mods:
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                mod.weight.copy_(_bf(mod.weight))
    h = _bf(x)
    li = 0                                       # index into plan.layers (conv | pool | flatten | fc), mods carries the LeakyReLUs too
    i = 0
    while i < len(mods):
        mod = mods[i]
        if isinstance(mod, nn.Conv2d):
            z = mod(h)
            gate = torch.where(nchw(ws["acts"][li]) > 0, 1.0, 0.1)           # the GPU's LeakyReLU gates of this layer
            h = q(z * gate)
            i += 2
            li += 1
        elif isinstance(mod, nn.MaxPool2d):
            _, idx = F.max_pool2d(nchw(ws["acts"][li - 1]), 2, 2, return_indices=True)   # the GPU's arg-maxes
            h = h.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            i += 1
            li += 1
        elif isinstance(mod, nn.Flatten):
            h = mod(h)
            i += 1
            li += 1
        elif isinstance(mod, nn.Linear):
            z = mod(h)
            if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU):
                y1 = fc_saved[li][1].float().cpu()
                h = q(z * torch.where(y1 > 0, 1.0, 0.1))
                i += 2
            else:
                h = z
                i += 1
            li += 1
        else:                                    # Dropout in eval mode
            i += 1
    lr, _ = crit(h.view(-1, 7, 7, 30), t)
    lr.backward()
    assert abs(lg.item() - lr.item()) < 0.02 * abs(lr.item()), (lg.item(), lr.item())
    report, bad = [], []
    for (n1, p1), (_, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert p1.grad is not None, n1
        g1, g2 = p1.grad.double().cpu().flatten(), p2.grad.double().flatten()
        rel = ((g1 - g2).norm() / (g2.norm() + 1e-30)).item()
        report.append(f"{n1:34s} rel {rel:.4f} |ref| {g2.norm().item():.3e}")
        if not rel < 0.02:
            bad.append(n1)
    model.cpu()
    print("\n".join(report))
    assert not bad, "\n".join(report)


def test_one_plan_serves_several_input_sizes():
    """sizes A, B, A through ONE backbone plan, forward and backward: the layer geometry belongs to the workspace of a call,
    not to the plan (a standalone YOLOv1Backbone takes any resolution, as the reference's does).  The third call must
    reproduce the first bit for bit in the forward and to fp32-atomic order in the gradients; both sizes agree with stock
    torch; and a forward at size B BETWEEN a training forward at size A and its backward must not disturb that backward."""
    import copy
    from test_gpu_layers import _bf, _close, bf16_faithful
    from yolo import YOLOv1Backbone
    torch.manual_seed(3)
    bb = YOLOv1Backbone()
    ref = bf16_faithful(copy.deepcopy(bb).features)
    bb = bb.cuda().train()
    xa = torch.randn(2, 3, 128, 128)
    xb = torch.randn(1, 3, 192, 160)

    def run(x):
        bb.zero_grad()
        y = bb(x.cuda())
        gy = torch.ones_like(y) / y.numel()
        y.backward(gy)
        return y.detach().clone(), [p.grad.detach().clone() for p in bb.parameters()]

    ya, ga = run(xa)
    yb, gb = run(xb)
    ya2, ga2 = run(xa)
    assert ya.shape == (2, 1024, 2, 2) and yb.shape == (1, 1024, 3, 3)
    assert torch.equal(ya, ya2)
    for a, b in zip(ga, ga2):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-7)
    for x, y in ((xa, ya), (xb, yb)):
        _close(y, _bf(ref(_bf(x))), 6.0, f"backbone forward at {tuple(x.shape)}")
    # interleaved: forward A (training), forward B (no grad), backward A
    bb.zero_grad()
    y = bb(xa.cuda())
    with torch.no_grad():
        bb(xb.cuda())
    y.backward(torch.ones_like(y) / y.numel())
    for a, p in zip(ga, bb.parameters()):
        torch.testing.assert_close(p.grad, a, rtol=1e-4, atol=1e-7)


def test_shape_errors_are_raised_not_read_out_of_bounds(model):
    """the library cannot know buffer extents, so the host side must refuse what the reference refuses (stock nn.Linear /
    tensor indexing raise there): a 224 x 224 batch into the 448 x 448 head, a 4-channel image, YOLOLoss with the wrong grid."""
    from yolo import YOLOLoss
    m = model.cuda().eval()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="cannot be multiplied|does not match"):
            m(torch.zeros(2, 3, 224, 224, device="cuda"))
        with pytest.raises(RuntimeError, match="expected input"):
            m(torch.zeros(2, 4, 448, 448, device="cuda"))
        assert m(torch.zeros(1, 3, 448, 448, device="cuda")).shape == (1, 7, 7, 30)      # the plan is still usable
    pred = torch.zeros(2, 7, 7, 30, device="cuda")
    with pytest.raises(RuntimeError, match="must both be"):
        YOLOLoss(S=14)(pred, pred)
    with pytest.raises(RuntimeError, match="must both be"):
        YOLOLoss()(pred, torch.zeros(2, 7, 7, 25, device="cuda"))
    model.cpu()


def test_loss_decreases_with_adam(model):
    """the drop-in train step (zero_grad / forward / loss / backward / clip / Adam) runs and learns."""
    import copy
    from yolo import YOLOLoss
    m = copy.deepcopy(model).cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=5e-4)
    crit = YOLOLoss()
    x = torch.from_numpy(synth.synth_images(4, 5)).cuda()
    t = torch.from_numpy(synth.synth_targets(4, 22)).cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss, d = crit(m(x), t)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
        opt.step()
        losses.append(d["total"])
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_every_layer_teacher_forced(model):
    """Full-size kernels, one at a time: take the activations / gradients the GPU pass stored and
    recompute every conv layer's forward, weight-, bias- and data-gradient from them with stock torch
    on the CPU.  Tolerance = one bf16 output rounding (k=1) for forward, k=3 for gradients."""
    import torch.nn.functional as F
    from torch.nn.grad import conv2d_input, conv2d_weight
    from test_gpu_layers import _bf, _close
    from yolo import YOLOLoss
    N = 2
    m = model.cuda().eval()
    from yolo import engine
    plan = m.hip_plan()
    plan.debug_keep = True
    engine.STEM_POOL_BWD_FUSED = False        # keep the first pool's gradient buffer so that it can be inspected
    try:
        m.zero_grad()
        x = torch.from_numpy(synth.synth_images(N, 3)).cuda()
        t = torch.from_numpy(synth.synth_targets(N, 21, max_obj=4)).cuda()
        loss, _ = YOLOLoss()(m(x), t)
        loss.backward()
        torch.cuda.synchronize()
        ws, fc_saved = plan.last
        unfused = [m.backbone.features[0].weight.grad.clone(), m.backbone.features[0].bias.grad.clone()]
        # the same pass with the pool backward fused into the stem's weight-gradient kernel: identical bits
        engine.STEM_POOL_BWD_FUSED = True
        plan.debug_keep = False
        m.zero_grad()
        loss2, _ = YOLOLoss()(m(x), t)
        loss2.backward()
        fused = [m.backbone.features[0].weight.grad, m.backbone.features[0].bias.grad]
        # (dZ of the stem is rebuilt identically; upstream gradients differ run to run only by fp32-atomic order in the
        #  FC / conv weight gradients, which do not feed the data-gradient chain)
        assert torch.equal(fused[0], unfused[0]) and torch.equal(fused[1], unfused[1])
    finally:
        engine.STEM_POOL_BWD_FUSED = True
        plan.debug_keep = False
        plan.last = None

    def nchw(act, stuffed=False):
        v = act.interior().float().cpu()
        if stuffed:
            v = v[:, 0::2, 0::2, :]
        return v.permute(0, 3, 1, 2).contiguous()

    layers = plan.layers
    checked = 0
    for li, L in enumerate(layers):
        if L.kind != "conv":
            continue
        a_in = ws["in"] if li == 0 else ws["acts"][li - 1]
        xin = nchw(a_in)[:, : L.Cin]
        w = _bf(L.weight.detach().float().cpu())
        b = L.bias.detach().float().cpu()
        y_ref = F.leaky_relu(F.conv2d(xin, w, b, stride=L.stride, padding=L.pad), 0.1)
        _close(nchw(ws["acts"][li]), _bf(y_ref), 1.0, f"layer {li} forward")
        g = ws["grads"][li]
        dz = nchw(g, stuffed=(L.stride == 2 and not L.first))[:, :, : L.Hout, : L.Wout]
        gw_ref = conv2d_weight(xin, w.shape, dz, stride=L.stride, padding=L.pad)
        _close(L.weight.grad, gw_ref, 3.0, f"layer {li} weight grad")
        _close(L.bias.grad, dz.sum((0, 2, 3)), 3.0, f"layer {li} bias grad")
        if li > 0:
            dx_ref = conv2d_input(xin.shape, w, dz, stride=L.stride, padding=L.pad)
            prev = layers[li - 1]
            if prev.kind == "conv":
                yprev = nchw(ws["acts"][li - 1])
                dx_ref = dx_ref * torch.where(yprev > 0, 1.0, 0.1)
                got = nchw(ws["grads"][li - 1], stuffed=(prev.stride == 2 and not prev.first))[:, :, : prev.Hout, : prev.Wout]
            else:
                got = nchw(ws["misc"][("gpool", li)])
            _close(got, _bf(dx_ref), 3.0, f"layer {li} data grad")
        checked += 1
    assert checked == 24
    # pools: gradient routing recomputed from the stored full-resolution activation
    for li, L in enumerate(layers):
        if L.kind != "pool":
            continue
        yfull = nchw(ws["acts"][li - 1]).requires_grad_(True)
        F.max_pool2d(F.leaky_relu(yfull, 1.0), 2, 2).backward(nchw(ws["misc"][("gpool", li + 1)]))
        ref = yfull.grad * torch.where(yfull.detach() > 0, 1.0, 0.1)
        _close(nchw(ws["grads"][li - 1]), _bf(ref), 1.0, f"pool {li} backward")
    model.cpu()


def test_hip_adam_matches_torch_adam():
    """yolo.optim.Adam(max_grad_norm=10) == clip_grad_norm_(10) + torch.optim.Adam, three steps."""
    from yolo.optim import Adam, clip_grad_norm_
    torch.manual_seed(0)
    shapes = [(1000, 37), (4096,), (3, 3, 3, 5), (1 << 20,)] + [(17 + i,) for i in range(60)]   # > YOLO_MT_MAX tensors: two launches
    pa = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa = Adam(pa, lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=5e-4)
    for it in range(3):
        for p, q in zip(pa, pb):
            g = torch.randn_like(p) * (3.0 if it == 1 else 0.001)   # step 1 clips, steps 0 and 2 do not
            p.grad = g.clone()
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(pb, max_norm=10.0)
        ob.step()
        oa.step()
        torch.cuda.synchronize()
        for p, q in zip(pa, pb):
            torch.testing.assert_close(p, q, rtol=2e-5, atol=2e-6)
            for key in ("exp_avg", "exp_avg_sq"):       # both moments, not only the parameter they move
                torch.testing.assert_close(oa.state[p][key], ob.state[q][key], rtol=2e-5, atol=2e-6)
    # stand-alone clip
    for p, q in zip(pa, pb):
        g = torch.randn_like(p) * 2
        p.grad, q.grad = g.clone(), g.clone()
    n1 = clip_grad_norm_(pa, 10.0)
    n2 = torch.nn.utils.clip_grad_norm_(pb, 10.0)
    torch.testing.assert_close(n1.cpu(), n2.cpu(), rtol=1e-5, atol=1e-5)
    for p, q in zip(pa, pb):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-5, atol=1e-7)
    # state_dict is interchangeable with torch.optim.Adam
    ob.load_state_dict(oa.state_dict())


def test_adam_refreshes_linear_bf16_operands():
    """Adam.attach_plan: the bf16 forward operand of every Linear is rewritten by the optimizer pass itself and the
    engine's cache accepts it (no re-cast); conv operands are re-packed by the next forward.  Two steps vs torch."""
    import copy
    import torch.nn as nn
    from yolo import engine
    from yolo.optim import Adam
    torch.manual_seed(2)
    mods = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(64 * 4 * 4, 128), nn.LeakyReLU(0.1),
                         nn.Dropout(0.5), nn.Linear(128, 30)).cuda().eval()
    ref = copy.deepcopy(mods)
    plan = engine.Plan.from_modules(list(mods), 64, False)
    oa = Adam(mods.parameters(), lr=1e-2, max_grad_norm=10.0)
    oa.attach_plan(plan)
    ob = torch.optim.Adam(ref.parameters(), lr=1e-2)
    x = torch.randn(4, 64, 4, 4, device="cuda")
    fc = [li for li, L in enumerate(plan.layers) if L.kind == "fc"]
    for it in range(2):
        oa.zero_grad(set_to_none=True)
        engine.run_plan(plan, x, False).square().mean().backward()
        for p, q in zip(mods.parameters(), ref.parameters()):
            q.grad = p.grad.clone()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 10.0)
        ob.step()
        oa.step()
        for li in fc:
            L = plan.layers[li]
            key, wf = plan._pf[li]
            assert key == plan._wkey(L.weight), "engine cache must accept the optimizer's shadow"
            assert torch.equal(wf.view(-1), L.weight.detach().to(torch.bfloat16).view(-1))
        for p, q in zip(mods.parameters(), ref.parameters()):
            torch.testing.assert_close(p, q, rtol=2e-5, atol=2e-6)
    # the refreshed operands are what the next forward computes with
    y1 = engine.run_plan(plan, x, False).detach()       # grad mode: the plain operands the optimizer maintains
    plan._pf.clear(); plan._pd.clear()
    y2 = engine.run_plan(plan, x, False).detach()
    with torch.no_grad():
        y3 = engine.run_plan(plan, x, False)            # inference: 128x64 panels packed from the fp32 master
    assert torch.equal(y1, y2) and torch.equal(y1, y3)


def test_adam_background_update_of_the_linear_layers():
    """Adam.attach_plan(plan, overlap=True): the Linear layers are updated by a background pass on a second stream
    (yolo_adam_step_multi_bg); the plan's next forward waits for it, optimizer.synchronize() / state_dict() make the current
    stream wait.  Three steps give the same parameters, optimizer state and outputs as the foreground update."""
    import copy
    import torch.nn as nn
    from yolo import engine
    from yolo.optim import Adam
    torch.manual_seed(3)
    base = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1), nn.LeakyReLU(0.1), nn.Flatten(), nn.Linear(64 * 6 * 6, 4096), nn.LeakyReLU(0.1),
                         nn.Dropout(0.5), nn.Linear(4096, 30)).cuda().eval()
    x = torch.randn(4, 64, 6, 6, device="cuda")
    outs = {}
    for overlap in (False, True):
        mods = copy.deepcopy(base)
        plan = engine.Plan.from_modules(list(mods), 64, False)
        opt = Adam(mods.parameters(), lr=1e-2, weight_decay=5e-4, max_grad_norm=1.0)
        opt.attach_plan(plan, overlap=overlap)
        assert bool(opt.deferred) == overlap
        ys = []
        for it in range(3):
            opt.zero_grad(set_to_none=True)
            y = engine.run_plan(plan, x, False)          # waits for the previous step's background pass in front of the Linear layers
            ys.append(y.detach().clone())
            y.square().mean().backward()
            opt.step()
        sd = opt.state_dict()                            # synchronises
        outs[overlap] = (ys, [p.detach().clone() for p in mods.parameters()],
                         [sd["state"][k]["exp_avg_sq"].clone() for k in sorted(sd["state"])])
    # (the two kernels are compiled separately: the compiler may contract a * b + c differently, hence a tolerance of a few ulp; a
    # forward that missed the update would be off by the whole step, lr = 1e-2)
    assert torch.equal(outs[False][0][0], outs[True][0][0])
    for a, b in zip(outs[False][0], outs[True][0]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5, msg="forward outputs differ: the forward did not wait for (or did not see) the background update")
    # parameters / second moments: the conv layer's weight gradient is summed with fp32 atomics (run-to-run differences of ~1e-9), which
    # Adam's m / (sqrt(v) + eps) magnifies on elements with gradients near eps; a missed update would be off by lr = 1e-2
    for group, atol in ((1, 5e-5), (2, 1e-7)):
        for a, b in zip(outs[False][group], outs[True][group]):
            torch.testing.assert_close(a, b, rtol=1e-3, atol=atol)


def test_detection_head_on_the_engine():
    """DetectionHead (conv 3x3 x4 incl. stride 2, Flatten, FC) forward + backward on the HIP plan vs the
    bf16-faithful stock-torch reference (narrow input so that the CPU side stays cheap)."""
    import copy
    from test_gpu_layers import _bf, _close, bf16_faithful
    from yolo import DetectionHead
    torch.manual_seed(7)
    head = DetectionHead(256, num_classes=20, S=7, B=2).eval()
    x = torch.randn(2, 256, 14, 14)
    gy = torch.randn(2, 7, 7, 30)
    g = copy.deepcopy(head).cuda()
    ref = torch.nn.Sequential(bf16_faithful(head.conv_layers), bf16_faithful(head.fc_layers))
    xc = _bf(x).requires_grad_(True)
    yc = ref(xc).view(-1, 7, 7, 30)
    yc.backward(gy)
    xg = x.clone().cuda().requires_grad_(True)
    yg = g(xg)
    assert yg.shape == (2, 7, 7, 30)
    yg.backward(gy.cuda())
    _close(yg, yc, 8.0, "head y")
    _close(xg.grad, xc.grad, 16.0, "head gx", frac=0.02)
    for (n, p1), (_, p2) in zip(g.named_parameters(), head.named_parameters()):
        _close(p1.grad, p2.grad, 16.0, f"head {n}", frac=0.02)


def test_resnet50_variant_inference():
    """BASELINE config 5 path: YOLOv1(ResNetBackbone) forward on the HIP engine (BN folded, residual add
    fused, 3x3/s2 max-pool) vs the same modules on the CPU (stock torch, eval), then decode + NMS of the
    predictions bit-exact vs the oracle.  ResNet50 numerics vs torchvision are 'parity unpinned' (DESIGN.md);
    this checks the engine against the architecture restated in yolo.resnet."""
    import copy
    from oracle import oracle as O
    from yolo import ResNetBackbone, YOLOv1, ops
    torch.manual_seed(11)
    m = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=True)).eval()
    with torch.no_grad():                      # non-trivial BN statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.6, 1.4)
                mod.weight.uniform_(0.7, 1.3)
                mod.bias.uniform_(-0.2, 0.2)
    x = torch.from_numpy(synth.synth_images(2, 9))
    with torch.no_grad():
        feat_c = m.backbone(x)
        y_c = m(x)
    g = copy.deepcopy(m).cuda()
    with torch.no_grad():
        feat_g = g.backbone(x.cuda())
        y_g = g(x.cuda())
    assert feat_g.shape == (2, 2048, 14, 14) and y_g.shape == (2, 7, 7, 30)
    assert _rel(feat_g, feat_c) < 0.03, _rel(feat_g, feat_c)
    assert _rel(y_g, y_c) < 0.05, _rel(y_g, y_c)
    # post-processing of the GPU predictions at conf 0.3 / nms 0.4 -- whatever the backbone produced
    p01 = torch.sigmoid(y_g)                   # map raw outputs into [0,1] so that boxes survive the threshold
    for variant in (0, 1):
        res = ops.postprocess_host(p01, 0.3, 0.4, variant, 7, 2, 20)
        for n, (rec, keep) in enumerate(res):
            r = O.decode(p01[n].cpu().numpy(), 0.3)
            assert np.array_equal(rec, r) and np.array_equal(keep, O.nms(r, 0.4, variant))
    # an UN-frozen trunk: gradients flow in training mode AND in eval() mode (running statistics; block by block against stock
    # torch in tests/test_gpu_resnet_train.py); the eval()-mode prediction with gradients equals the folded inference path up to
    # bf16 roundings, and backward() fills every trunk gradient
    for p in g.backbone.parameters():
        p.requires_grad = True
    ye = g.eval()(x.cuda())
    assert ye.requires_grad
    assert _rel(ye.detach(), y_g) < 0.05, _rel(ye.detach(), y_g)
    ye.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in g.backbone.parameters())
    assert g.train()(x.cuda()).requires_grad


def test_frozen_resnet_backbone_in_training_mode():
    """The reference's default training run: YOLOv1(ResNetBackbone(freeze=True)) with model.train() -> the frozen trunk's
    BatchNorm layers use BATCH statistics and update their running statistics (trainer.py:49); only the DetectionHead gets
    gradients.  HIP path = conv with raw weights + yolo_batchnorm_train_fwd.  A randomly initialised BatchNorm ResNet in
    batch-statistics mode is chaotic (a 0.3 % bf16 perturbation grows ~1.25x per bottleneck: 54 % after 16 blocks, measured), so
    the trunk is checked TEACHER-FORCED: every bottleneck's CPU result is computed from the GPU's input to that block."""
    import copy
    from yolo import ResNetBackbone, YOLOLoss, YOLOv1
    torch.manual_seed(13)
    m = YOLOv1(backbone=ResNetBackbone(pretrained=False, freeze=True)).train()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.7, 1.3)
                mod.bias.uniform_(-0.2, 0.2)
    for mod in m.modules():                         # dropout off: compare deterministic functions
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    g = copy.deepcopy(m).cuda()
    x = torch.from_numpy(synth.synth_images(4, 21))
    tgt = torch.from_numpy(synth.synth_targets(4, seed=5))
    feat_g = g.backbone(x.cuda())
    assert not feat_g.requires_grad and feat_g.shape == (4, 2048, 14, 14) and torch.isfinite(feat_g).all()
    plan, ext = g.backbone._plan, m.backbone.extractor

    def buf(tag):
        a = next(a for k, a in plan._bufs.items() if k[0] == tag)
        return a.interior().float().permute(0, 3, 1, 2).cpu()

    with torch.no_grad():
        stem_c = ext[2](ext[1](ext[0](x.to(torch.bfloat16).float())))
        assert _rel(buf("stem"), stem_c) < 0.01
        assert _rel(buf("pool"), ext[3](buf("stem"))) < 1e-6                      # max-pool of the same values: exact
        prev = "pool"
        for li in range(4, 8):
            for bi, blk in enumerate(ext[li]):
                assert _rel(buf((li, bi, 3)), blk(buf(prev))) < 0.02, (li, bi)
                prev = (li, bi, 3)
    # running statistics moved as aten's do (momentum 0.1 from mean 0 / var 1), counters incremented
    bc, bg = ext[1], g.backbone.extractor[1]
    torch.testing.assert_close(bg.running_mean.cpu(), bc.running_mean, rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(bg.running_var.cpu(), bc.running_var, rtol=2e-2, atol=2e-3)
    assert int(g.backbone.extractor[7][2].bn3.num_batches_tracked) == 1
    # one training step: gradients reach the head only, and equal the CPU head's gradients for the same features
    crit = YOLOLoss()
    pred_g = g(x.cuda())
    seen = []
    pred_g.register_hook(lambda gr: seen.append(gr.detach().cpu().clone()))     # dL/dpred as it enters the head's backward
    loss_g, _ = crit(pred_g, tgt.cuda())
    loss_g.backward()
    assert all(p.grad is None for p in g.backbone.parameters())
    feats = g.backbone._plan.forward_batch_stats(x.cuda()).cpu()
    # CPU head with the engine's storage roundings (bf16 weights, bf16 activations after every LeakyReLU), so that the
    # LeakyReLU gates are decided on the same values on both sides -- the fp32 head differs by 8-14 % in its first conv's
    # gradient on these chaotic random-init features, depending on nothing but rounding
    def q(t):
        return t + (t.to(torch.bfloat16).float() - t).detach()
    with torch.no_grad():
        for mod in m.head.modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                mod.weight.copy_(mod.weight.to(torch.bfloat16).float())
    h = feats
    for mod in list(m.head.conv_layers) + list(m.head.fc_layers):
        h = mod(h)
        if isinstance(mod, torch.nn.LeakyReLU):
            h = q(h)
    out_c = h.view(-1, 7, 7, 30)
    loss_c, _ = crit(out_c, tgt)
    assert abs(loss_g.item() - loss_c.item()) < 0.02 * abs(loss_c.item())
    # the loss gradient is taken from the GPU pass (teacher forcing): on random-init predictions the loss's choice of the
    # responsible box (arg-max of two IoUs that are both ~0, src/yolo/loss.py:110) flips under a 1 % perturbation of the
    # prediction and changes dL/dpred by tens of per cent -- a property of the loss, checked on its own in test_gpu_loss.py
    out_c.backward(seen[0])
    hg = dict(g.head.named_parameters())
    report = {n: _rel(hg[n].grad, pc.grad) for n, pc in m.head.named_parameters()}
    print("head gradient errors:", {n: round(v, 4) for n, v in report.items()})
    for n, pc in m.head.named_parameters():
        # (4.4-4.7 % with one plain launch per layer, 5.1-5.9 % with the K ranges of the few-pixel head convs summed as slabs: the level is set by
        # LeakyReLU gates flipping under bf16 rounding, not by the arithmetic -- the last Linear, behind no gate, is at 0.3 % either way)
        assert hg[n].grad is not None and report[n] < (0.08 if "fc_layers.4" not in n else 0.01), report


@pytest.mark.parametrize("n", [1, 2, 5])
def test_small_batches_unfuse_the_few_tile_pool_convs(model, n):
    """serving batches: with config.SMALL_SPLIT the deep-K convs in front of a pool that would give the pooled kernel less than a quarter of the chip
    run un-fused (K ranges as slabs + the pool as its own pass, executor.Plan._few_tiles) -- same predictions as the fused launches up to the
    rounding of another fp32 summation order, and the un-fused pool passes are really there."""
    from yolo import engine
    g = model.cuda().eval()
    torch.manual_seed(31)
    x = torch.randn(n, 3, 448, 448, device="cuda")
    out, tags = {}, {}
    for on in (True, False):
        engine.SMALL_SPLIT = on
        try:
            with torch.no_grad():
                g(x)
                engine.TIMERS = []
                out[on] = g(x).float().clone()
                torch.cuda.synchronize()
                tags[on] = [t[0] for t in engine.TIMERS]
        finally:
            engine.TIMERS = None
            engine.SMALL_SPLIT = True
    assert not any(t.startswith("pool") for t in tags[False]), tags[False]            # every pool fused into its conv
    assert ("pool19" in tags[True] and "conv18" in tags[True]) == (n <= 4), tags[True]  # 28x28, 512 -> 1024: 16 tiles of 224 x 256 at batch 1, 72 at 5
    assert ("pool8" in tags[True]) == (n <= 2), tags[True]                             # 56x56, 256 -> 512: 28 tiles at batch 1, 56 at 2, 140 at 5
    assert _rel(out[True], out[False]) < 0.01, _rel(out[True], out[False])


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16, 32, 3, 13, 24])
def test_measured_plans_of_the_other_batch_sizes_agree_with_plain_launches(model, n):
    """yolo/plans/gfx950.json holds measured plans for batches 1, 2, 4, 8, 16 and 32 as well (64 has tests of its own).  The tuner only TIMES a
    candidate; that each chosen plan also computes the layer is checked here for every problem of a batch size at once: forward and backward (a fixed
    dL/dpred, so that YOLOLoss's discontinuity stays out) on the shipped plans against the same pass with no table entries and plain single launches.
    A plan that drops or doubles a K range or a tile shows as an O(1) difference; other fp32 summation orders as 0.2-0.8 % of the predictions and a
    few per cent of the gradients behind many LeakyReLU gates (rounding level on the last Linear)."""
    import copy
    from yolo import engine, plans
    g = copy.deepcopy(model).cuda().train()
    for mod in g.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    torch.manual_seed(41)
    x = torch.from_numpy(synth.synth_images(n, 17)).cuda()
    dpred = torch.randn(n, 7, 7, 30, device="cuda") / n
    shipped = {k: v for k, v in plans._TUNED.items() if k[0] in (1, 2, 4, 8, 16, 32, 64)}
    measured = n in (1, 2, 4, 8, 16, 32)
    # 13, 24 images: no measured plans -- every problem borrows the plan of the same layer at the nearest measured batch size (plans._borrowed_plan);
    # 3 images: the default rules
    assert (sum(1 for k in shipped if k[0] == n) >= 60) == measured
    res = {}
    try:
        for name, table, split in (("shipped", shipped, True), ("plain", {}, False)):
            plans._TUNED.clear()
            plans._TUNED.update(table)
            engine.SMALL_SPLIT = split
            for p in g.parameters():
                p.grad = None
            pred = g(x)
            pred.backward(dpred)
            torch.cuda.synchronize()
            res[name] = (pred.detach().float().clone(), {k: p.grad.detach().float().clone() for k, p in g.named_parameters()})
            if name == "shipped":
                used = [k for k in plans._TUNED if k[0] == n]
                if measured:
                    assert all(k in shipped for k in used), [k for k in used if k not in shipped]      # every problem of the step ran on a measured plan
                elif n >= 8:
                    near = {13: 16, 24: 32}[n]
                    same = sum(1 for k in used if plans._TUNED[k] == shipped.get((near,) + k[1:]))
                    assert same >= 0.8 * len(used) and not plans._BORROWED, (same, len(used))          # ... borrowed, and every borrowed plan has run
    finally:
        plans._TUNED.clear()
        plans._TUNED.update(shipped)
        engine.SMALL_SPLIT = True
    (pa, ga), (pb, gb) = res["shipped"], res["plain"]
    assert _rel(pa, pb) < 0.02, _rel(pa, pb)
    report = {k: round(_rel(ga[k], gb[k]), 4) for k in ga}
    last = [k for k in report if k.startswith("head.4.")]
    assert last and all(report[k] < 0.01 for k in last), report
    # (2 and 3 images: 23-26 % at the first conv layers -- the same level as the two-rank test's cosine of 0.975 there; 4 .. 32 images: < 20 %.  A data-gradient
    # plan that computes something else puts every layer in front of it at ~100 %)
    assert max(report.values()) < (0.4 if n <= 3 else 0.2), report


def test_dropout_probability_is_read_at_every_forward(model):
    """stock nn.Dropout reads ``p`` when it runs; the engine's plan is built once, at the first forward, and must not freeze the value it saw then
    (found when a deep copy of a model that had already run kept dropping half of the Linear layer's outputs after ``mod.p = 0.0``)."""
    import copy
    g = copy.deepcopy(model).cuda().train()
    x = torch.from_numpy(synth.synth_images(2, 3)).cuda()
    with torch.no_grad():
        a, b = g(x).clone(), g(x).clone()
        assert not torch.equal(a, b)                       # p = 0.5: two masks
        drops = [m for m in g.modules() if isinstance(m, torch.nn.Dropout)]
        assert drops
        for m in drops:
            m.p = 0.0
        c, d = g(x).clone(), g(x).clone()
        assert torch.equal(c, d)                           # p = 0: no mask ...
        g.eval()
        assert torch.equal(g(x), c)                        # ... = inference
        g.train()
        for m in drops:
            m.p = 0.5
        assert not torch.equal(g(x), c)


def test_gradient_arena_equals_autograd_path(model):
    """data-parallel plumbing on one GPU: with the gradient arena attached, backward writes the same
    gradients into the flat buffer, assigns p.grad views, and fires the bucket callbacks in arena order
    covering the whole weight region.  (Two passes of the SAME model already differ by ~0.3 % on the deepest
    gradients: the split-K FC forward and the weight-gradient kernel accumulate with fp32 atomics, a different
    summation order can move a bf16 rounding by one ulp and flip LeakyReLU gates downstream -- hence the
    relative-L2 bound instead of elementwise equality; every yolo_igemm configuration itself is bit-reproducible,
    tools/check_determinism.py.)"""
    import copy
    from yolo import YOLOLoss
    m1 = copy.deepcopy(model).cuda().eval()
    m2 = copy.deepcopy(model).cuda().eval()
    x = torch.from_numpy(synth.synth_images(2, 4)).cuda()
    t = torch.from_numpy(synth.synth_targets(2, 23, max_obj=4)).cuda()
    crit = YOLOLoss()
    crit(m1(x), t)[0].backward()
    plan = m2.hip_plan()
    arena = plan.attach_grad_arena(x.device)
    seen = []
    plan.on_grad_ready = lambda lo, hi: seen.append((lo, hi))
    done = []
    plan.on_backward_done = lambda: done.append(True)
    for _ in range(2):                        # second pass: overwrite semantics, no accumulation
        seen.clear()
        crit(m2(x), t)[0].backward()
    assert done and seen[0][0] == 0 and all(a[1] == b[0] for a, b in zip(seen, seen[1:])) and seen[-1][1] == plan._arena_w_end
    assert seen[1][1] - seen[1][0] == 4096 * 50176            # FC1 is ready second (right after the 6 M-parameter FC2)
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert p2.grad.data_ptr() >= arena.data_ptr() and p2.grad.data_ptr() < arena.data_ptr() + arena.numel() * 4, n
        assert _rel(p2.grad, p1.grad) < 0.03, (n, _rel(p2.grad, p1.grad))


def test_adam_takes_the_big_linear_gradient_norm_from_the_weight_gradient_kernel():
    """Plan.backward leaves |dW|_F^2 of the Linear behind nn.Flatten, summed by yolo_wgrad while it stores dW (yolo_wgrad_desc.dw_sumsq,
    engine.FC_NORM_IN_WGRAD); the optimizer uses it instead of reading the 822 MB gradient -- only while .grad is still the memory
    that backward pass wrote, unmodified."""
    from yolo import YOLOLoss, YOLOv1, engine
    from yolo.optim import Adam, grad_norm_sq
    torch.manual_seed(0)
    m = YOLOv1().cuda().eval()
    x = torch.from_numpy(synth.synth_images(2, 3)).cuda()
    t = torch.from_numpy(synth.synth_targets(2, 4)).cuda()
    opt = Adam(m.parameters(), lr=1e-4, max_grad_norm=10.0)
    plan = m.hip_plan()
    opt.attach_plan(plan)
    loss, _ = YOLOLoss()(m(x), t)
    loss.backward()
    params = [p for p in m.parameters() if p.grad is not None]
    big = max(params, key=lambda p: p.numel())
    assert id(big) in plan.grad_norm_sq and plan.grad_norm_sq[id(big)][0] == (big.grad.data_ptr(), tuple(big.grad.shape)), "autograd must take the gradient over without a copy"
    full = grad_norm_sq(params).item()
    hinted = grad_norm_sq(params, plan.grad_norm_sq).item()
    direct = big.grad.double().pow(2).sum().item()
    assert abs(plan.grad_norm_sq[id(big)][2].item() - direct) <= 1e-5 * direct
    assert abs(full - hinted) <= 1e-5 * full
    big.grad.mul_(2.0)                                   # modified in place: the stored norm no longer describes it
    assert abs(grad_norm_sq(params, plan.grad_norm_sq).item() - grad_norm_sq(params).item()) <= 1e-9 * full


def test_flagged_step_updates_nothing_and_model_reads_wait_for_the_background_update():
    """(1) the loss kernel's error word (a target selecting a box slot >= B; the reference raises IndexError inside the loss,
    before any update) reaches the host only after optimizer.step() was enqueued: handed to the optimizer as ``skip_if`` the whole
    update -- foreground and background launches -- is a no-op on the device, and the error surfaces at the first read of the parts;
    (2) with attach_plan(overlap=True) the owning model's state_dict() / load_state_dict() / deepcopy wait for the background pass by
    themselves."""
    import copy
    from yolo import YOLOLoss, YOLOv1
    from yolo.optim import Adam
    torch.manual_seed(5)
    m = YOLOv1().cuda().train()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_plan(m.hip_plan(), overlap=True)
    assert opt._hooked, "the model that owns the plan carries the state_dict hooks"
    x = torch.from_numpy(synth.synth_images(2, 3)).cuda()
    tgt = torch.from_numpy(synth.synth_targets(2, 4)).cuda()
    crit = YOLOLoss()

    def one_step(t):
        opt.zero_grad(set_to_none=True)
        loss, parts = crit(m(x), t)
        loss.backward()
        opt.skip_if = parts.device_flag
        opt.step()
        return parts

    parts = one_step(tgt)
    sd1 = {k: v.detach().clone() for k, v in m.state_dict().items()}        # (2): waits for the background update of the Linear layers
    before = {k: v.clone() for k, v in sd1.items()}
    assert float(parts["total"]) > 0
    assert any(not torch.equal(sd1[k], v) for k, v in copy.deepcopy(m).state_dict().items()) is False
    bad = tgt.clone()
    bad[0, 1, 1, 14] = 1.0                       # channel 14 is a class channel: 4::5 selects "slot 2" of a B = 2 model
    bad[0, 1, 1, 4] = 0.0
    bad[0, 1, 1, 9] = 0.0
    parts = one_step(bad)
    with pytest.raises(RuntimeError, match="box slot"):
        parts["total"]
    torch.cuda.synchronize()
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), f"{k} changed in a flagged step"
    st = opt.state_dict()["state"]
    assert all(float(s["exp_avg"].abs().max()) > 0 for s in st.values())      # the first (valid) step did update
    parts = one_step(tgt)                        # and training goes on
    assert float(parts["total"]) > 0
    changed = sum(not torch.equal(m.state_dict()[k], v) for k, v in before.items())
    assert changed == len(before)
    m.load_state_dict(sd1)                       # (2): load waits as well
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd1[k])


def test_gradient_reaches_the_input_image():
    """The reference's tests/test_backbone.py:187-196 on the device (the one reference-suite test the HIP path failed with
    NotImplementedError): YOLOv1()(x).sum().backward() with x.requires_grad leaves a finite, non-zero x.grad -- and the stem's data
    gradient itself (7x7 / stride 2 / pad 3 as four parity-class correlations, engine.Plan._stem_dgrad) equals stock torch's on two
    images within the 3-ulp bf16 bound of the other gradient checks, teacher-forced: conv -> LeakyReLU -> MaxPool2d with the same
    bf16-rounded operands on both sides, so that LeakyReLU gates and pool arg-maxes agree."""
    import copy
    import torch.nn as nn
    from test_gpu_layers import _bf, _close, bf16_faithful
    from yolo import YOLOv1, engine
    torch.manual_seed(21)
    model = YOLOv1().cuda().eval()
    x = torch.randn(1, 3, 448, 448, device="cuda", requires_grad=True)
    model(x).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    # ... and the parameters got their gradients in the same pass, as before
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    del model
    # the stem alone against stock torch
    mods_c = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3), nn.LeakyReLU(0.1), nn.MaxPool2d(2, 2))
    mods_g = copy.deepcopy(mods_c).cuda()
    xs = torch.randn(2, 3, 64, 96)
    xc = _bf(xs).clone().requires_grad_(True)
    yc = bf16_faithful(mods_c)(xc)
    plan = engine.Plan.from_modules(list(mods_g), 3, True)
    xg = xs.clone().cuda().requires_grad_(True)
    yg = engine.run_plan(plan, xg, False)
    gy = torch.randn(yc.shape, generator=torch.Generator().manual_seed(5))
    yc.backward(gy)
    yg.backward(gy.cuda())
    _close(yg, yc, 1.0, "stem + pool y")
    _close(xg.grad, xc.grad, 3.0, "gradient wrt the image", frac=0.002)
    _close(mods_g[0].weight.grad, mods_c[0].weight.grad, 3.0, "stem gw (un-fused pool backward)")
    # without requires_grad on the input nothing of this runs (the training step's FLOP count skips the product)
    xg2 = xs.clone().cuda()
    engine.run_plan(plan, xg2, False).backward(gy.cuda())
    assert xg2.grad is None
