"""tests/stem_ref.py against stock torch in fp64 at two small sizes (no GPU): the forward descriptor through launch_ref.igemm_ref in every pool mode,
the weight / bias gradient against autograd, the pool + LeakyReLU gradient tile and the arg-max codes against max_pool2d(return_indices=True) --
and an fp32 CPU evaluation of each stays inside its bound."""

import pytest
import torch
import torch.nn.functional as F

import launch_ref as lr
import stem_ref as sr

BF = torch.bfloat16
SIZES = [(1, 16, 32), (2, 48, 64)]          # one tile; 3 x 2 tiles per image


def _problem(seed, N, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    b = torch.randn(64, generator=g) * 0.5
    return x, w, b


def _store(geo, y_nhwc, fill=0.0):
    buf = torch.full((geo.numel,), fill, dtype=BF)
    geo.interior(buf).copy_(y_nhwc.to(BF))
    return buf


@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("mode", ["0", "1", "1full", "3", "0relu"])
def test_forward_reference_equals_stock_torch(N, H, W, mode):
    x, w, b = _problem(N + H, N, H, W)
    slope = 0.0 if mode == "0relu" else 0.1
    pool2 = int(mode[0])
    xbuf, xg = sr.stem_input(x)
    Ho, Wo = H // 2, W // 2
    og = sr.Geo(N, Ho // 2, Wo // 2, 64, 1) if pool2 else sr.Geo(N, Ho, Wo, 64, 1)
    fg = sr.Geo(N, Ho, Wo, 64, 0) if mode == "1full" else None
    d = sr.stem_desc(xg, og, slope, pool2, fg)
    R = sr.stem_fwd_ref(d, xbuf, sr.stem_panel(w), b)
    xd, wd = x.to(BF).double(), w.to(BF).double()
    act = F.leaky_relu(F.conv2d(xd, wd, b.double(), stride=2, padding=3), slope)
    pooled, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    want = (pooled if pool2 else act).permute(0, 2, 3, 1)
    assert torch.allclose(og.interior(R.ref), want, rtol=1e-12, atol=1e-12)
    assert torch.equal(R.addressed, og.mask())
    assert bool((R.bnd[~R.addressed] < 0).all()) and bool((R.bnd[R.addressed] > 0).all())
    # what a correct kernel stores: fp32 accumulation of the same bf16 operands, one rounding
    act32 = F.leaky_relu(F.conv2d(x.to(BF).float(), w.to(BF).float(), b, stride=2, padding=3), slope).to(BF)
    pool32, idx32 = F.max_pool2d(act32.float(), 2, 2, return_indices=True)
    got = _store(og, (pool32 if pool2 else act32).permute(0, 2, 3, 1), 7.0)
    got_aux = got_codes = None
    if fg is not None:
        assert torch.allclose(fg.interior(R.aux_ref), act.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        assert torch.equal(R.aux_addressed, fg.mask()[: R.aux_addressed.numel()])
        got_aux = _store(fg, act32.permute(0, 2, 3, 1), 7.0)
    if pool2 == 3:
        pos32 = ((idx32 // Wo) % 2) * 2 + (idx32 % Wo) % 2
        got_codes = sr.pack_codes(pos32.permute(0, 2, 3, 1), og)
        assert torch.equal(sr.unpack_codes(got_codes, og), pos32.permute(0, 2, 3, 1).to(torch.int32))
        # the reference's own windows give max_pool2d's indices
        pos = ((idx // Wo) % 2) * 2 + (idx % Wo) % 2
        assert torch.equal(R.codes_vals.argmax(1).view(N, Ho // 2, Wo // 2, 64), pos.permute(0, 2, 3, 1))
    worst, fails = R.check(got, got_aux, got_codes, what=mode)
    assert not fails and 0.0 < worst <= 1.0, (worst, fails)
    # and a sabotaged result is rejected: one tap of the window dropped at the right image border
    xs = x.clone()
    xs[:, :, :, -1] = 0.0
    bad = F.leaky_relu(F.conv2d(xs.to(BF).float(), w.to(BF).float(), b, stride=2, padding=3), slope).to(BF)
    bad = (F.max_pool2d(bad.float(), 2, 2) if pool2 else bad).permute(0, 2, 3, 1)
    _, fails = R.check(_store(og, bad), got_aux, None if pool2 != 3 else got_codes, what=mode)
    assert fails


@pytest.mark.parametrize("N,H,W", SIZES)
def test_weight_gradient_reference_equals_autograd(N, H, W):
    x, _, _ = _problem(3 * N + W, N, H, W)
    g = torch.Generator().manual_seed(5)
    Ho, Wo = H // 2, W // 2
    dy = (torch.randn(N, 64, Ho, Wo, generator=g) * 0.25).to(BF)
    xbuf, xg = sr.stem_input(x)
    dg = sr.Geo(N, Ho, Wo, 64, 1)
    dyb = _store(dg, dy.permute(0, 2, 3, 1))
    nt = sr.tiles(N, H, W)
    for G in (1, nt):
        A = sr.wgrad_additions(nt, G)
        assert A == -(-nt // G) * 128 + G
        dw, dwb, db, dbb = sr.stem_wgrad_ref(xbuf, xg, dyb, dg, A)
        xr = x.to(BF).double()
        w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(64, dtype=torch.float64, requires_grad=True)
        F.conv2d(xr, w, b, stride=2, padding=3).backward(dy.double())
        assert torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db, b.grad, rtol=1e-12, atol=1e-12)
        # fp32 autograd (at least P additions per element, more than any A here is sized for only when G is large): inside the G = 1 bound
        if G == 1:
            w32 = torch.zeros(64, 3, 7, 7, requires_grad=True)
            b32 = torch.zeros(64, requires_grad=True)
            F.conv2d(x.to(BF).float(), w32, b32, stride=2, padding=3).backward(dy.float())
            fails = []
            r1 = lr.check_values(dw, dwb, w32.grad, "dw", fails)
            r2 = lr.check_values(db, dbb, b32.grad, "db", fails)
            assert not fails and r1 <= 1.0 and r2 <= 1.0, fails
            # a dropped kx = 6 tap is far outside
            bad = w32.grad.clone()
            bad[..., 6] = 0.0
            lr.check_values(dw, dwb, bad, "dw", fails)
            assert fails


@pytest.mark.parametrize("N,H,W", [(1, 8, 16), (3, 12, 20)])
def test_pool_lrelu_gradient_tile_equals_autograd(N, H, W):
    g = torch.Generator().manual_seed(N)
    vals = torch.tensor([-1.0, -0.25, 0.0, 0.5, 2.0])
    y = vals[torch.randint(0, 5, (N, H, W, 16), generator=g)].to(BF)
    dpool = torch.randn(N, H // 2, W // 2, 16, generator=g).to(BF)
    slope = 0.5                  # a power of two: dpool * slope is exact in bf16, so autograd in fp64 gives the very bits
    dz, pooled, first = sr.pool_lrelu_grad(y, dpool, slope)
    # stock torch: z -> leaky_relu -> max_pool2d, with y = leaky_relu(z) (sign(y) == sign(z))
    yc = y.double().permute(0, 3, 1, 2)
    pc, idx = F.max_pool2d(yc, 2, 2, return_indices=True)
    assert torch.equal(pooled.double(), pc.permute(0, 2, 3, 1))
    pos = ((idx // W) % 2) * 2 + (idx % W) % 2
    assert torch.equal(first.long(), pos.permute(0, 2, 3, 1))
    z = torch.where(yc > 0, yc, yc / slope).requires_grad_(True)
    F.max_pool2d(F.leaky_relu(z, slope), 2, 2).backward(dpool.double().permute(0, 3, 1, 2))
    assert torch.equal(dz.double(), z.grad.permute(0, 2, 3, 1))
    # slope 0.1: the same positions; one fp32 product and one cast where the maximum is not positive, dpool itself elsewhere
    dz1, _, _ = sr.pool_lrelu_grad(y, dpool, 0.1)
    at_first = sr.windows(dz1.float()).gather(-1, first.long().unsqueeze(-1))[..., 0]
    want = torch.where(pooled.float() > 0, dpool.float(), dpool.float() * torch.tensor(0.1, dtype=torch.float32)).to(BF)
    assert torch.equal(at_first, want.float()) and int((dz1 != 0).sum()) == int((want != 0).sum())
    # the set has ties: more than one window in ten holds its maximum twice
    win = sr.windows(y.float())
    assert float(((win == win.amax(-1, keepdim=True)).sum(-1) > 1).float().mean()) > 0.1
    # codes round trip through the packed words
    pg = sr.Geo(N, H // 2, W // 2, 16, 1)
    assert torch.equal(sr.unpack_codes(sr.pack_codes(first, pg), pg), first)
