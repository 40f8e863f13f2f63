"""The fp64 launch reference of tests/launch_ref.py against stock torch on small problems (no GPU): forward convs at stride 1 / 2 with padded channel
strides, the parity classes of a stride-2 data gradient, every epilogue, the fused pool and its arg-max codes, both weight-gradient forms -- and sabotaged
outputs the checkers must reject (three forward ones, four of a weight gradient that relative L2 lets pass)."""

from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import launch_ref as lr

BF = torch.bfloat16


class Buf:
    """zero-haloed NHWC bf16 buffer [N][H+2h][W+2h][Cp] (Cp >= C channels) between guard bands of zeros, as engine.Act lays it out"""

    def __init__(self, N, H, W, C, halo=1, cpad=None, dtype=BF):
        self.N, self.H, self.W, self.C, self.h = N, H, W, C, halo
        self.Cp = cpad or C
        self.Hp, self.Wp = H + 2 * halo, W + 2 * halo
        self.px, self.row, self.img = self.Cp, self.Wp * self.Cp, self.Hp * self.Wp * self.Cp
        self.guard = (self.Wp + 2) * self.Cp + 64
        self.store = torch.zeros(2 * self.guard + N * self.img, dtype=dtype)

    def region(self):
        return self.store[self.guard: self.guard + self.N * self.img]

    def view(self):
        return self.region().view(self.N, self.Hp, self.Wp, self.Cp)

    def interior(self):
        h = self.h
        return self.view()[:, h: h + self.H, h: h + self.W, : self.C]

    def off(self, shift=0):
        h = self.h - shift
        return (h * self.Wp + h) * self.Cp

    def fill(self, x_nchw):
        self.interior().copy_(x_nchw.permute(0, 2, 3, 1).to(self.store.dtype))
        return self


def _bf(t):
    return t.to(BF).double()


def _desc(**kw):
    base = dict(epilogue=0, slope=0.1, out_fp32=0, split_k=1, aux_img_stride=0, aux_row_stride=0, aux_px_stride=0, aux_off=0, pool2=0)
    base.update(kw)
    return SimpleNamespace(**base)


def _conv_desc(xb, ob, k, s, cout, **kw):
    pad = (k - 1) // 2
    Ho, Wo = (xb.H + 2 * pad - k) // s + 1, (xb.W + 2 * pad - k) // s + 1
    return _desc(N=xb.N, Ho=Ho, Wo=Wo, in_img_stride=xb.img, in_row_stride=xb.row, in_px_stride=xb.px, in_off=xb.off(pad), stride=s, KH=k, KW=k,
                 tap_len=xb.C, Cout=cout, out_img_stride=ob.img, out_row_stride=ob.row, out_px_stride=ob.px, out_off=ob.off(), **kw)


def _packed(w):
    """OIHW -> [Cout][KH][KW][Cin] flat bf16, the forward operand"""
    return w.permute(0, 2, 3, 1).contiguous().to(BF).reshape(-1)


def _store(ob, y_nhwc):
    """a kernel's output as the checker reads it: the whole region, y written into the interior"""
    got = ob.region().clone()
    h = ob.h
    got.view(ob.N, ob.Hp, ob.Wp, ob.Cp)[:, h: h + y_nhwc.shape[1], h: h + y_nhwc.shape[2], : y_nhwc.shape[3]] = y_nhwc.to(BF)
    return got


def _problem(seed, N, H, cin, cout, k, s, cpad_in, cpad_out):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, H, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    xb = Buf(N, H, H, cin, 1, cpad_in).fill(x)
    if cpad_in > cin:           # channel padding of the input holds garbage the launch must not read
        xb.view()[..., cin:] = 7.0
    Ho = (H + 2 * ((k - 1) // 2) - k) // s + 1
    ob = Buf(N, Ho, Ho, cout, 1, cpad_out)
    return x, w, xb, ob


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_forward_equals_conv2d_with_padded_channel_strides(k, s):
    x, w, xb, ob = _problem(1 + k + s, 2, 8, 24, 40, k, s, 32, 48)
    d = _conv_desc(xb, ob, k, s, 40)
    R = lr.igemm_ref(d, xb.store, xb.guard, _packed(w))
    want = F.conv2d(_bf(x), _bf(w), stride=s, padding=(k - 1) // 2).permute(0, 2, 3, 1)
    got_ref = lr._out_view(R.ref, d)
    assert torch.allclose(got_ref, want, rtol=1e-12, atol=1e-12)
    # exactly the interior's first Cout channels are addressed: halo and channel padding are not
    assert int(R.addressed.sum()) == want.numel()
    assert bool(lr._out_view(R.addressed, d).all())
    # a float32 result rounded to bf16 (what a correct kernel stores) lies inside the bound
    worst, fails = R.check(_store(ob, F.conv2d(x.to(BF).float(), w.to(BF).float(), stride=s, padding=(k - 1) // 2).permute(0, 2, 3, 1)), what="conv")
    assert not fails and 0.0 < worst <= 1.0


@pytest.mark.parametrize("epi", [1, 2, 3, 4])
def test_epilogues(epi):
    x, w, xb, ob = _problem(10 + epi, 2, 8, 16, 24, 3, 1, 16, 32)
    g = torch.Generator().manual_seed(99)
    bias = torch.randn(24, generator=g)
    a = torch.randn(2, 24, 8, 8, generator=g)
    ab = Buf(2, 8, 8, 24, 1, 40).fill(a)
    d = _conv_desc(xb, ob, 3, 1, 24, epilogue=epi, slope=0.1 if epi != 4 else 0.0,
                   aux_img_stride=ab.img, aux_row_stride=ab.row, aux_px_stride=ab.px, aux_off=ab.off())
    R = lr.igemm_ref(d, xb.store, xb.guard, _packed(w), bias, ab.store, ab.guard)
    z = F.conv2d(_bf(x), _bf(w), padding=1)
    av = _bf(a)
    if epi == 1:
        want = z + bias.double()[None, :, None, None]
    elif epi == 2:
        want = F.leaky_relu(z + bias.double()[None, :, None, None], 0.1)
    elif epi == 3:
        want = z * torch.where(av > 0, 1.0, 0.1)
    else:
        want = F.relu(z + bias.double()[None, :, None, None] + av)
    assert torch.allclose(lr._out_view(R.ref, d), want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    worst, fails = R.check(_store(ob, want.float().permute(0, 2, 3, 1)))
    assert not fails and worst <= 1.0


@pytest.mark.parametrize("pool2", [1, 2, 3])
def test_fused_pool_and_argmax_codes(pool2):
    x, w, xb, ob = _problem(30 + pool2, 2, 8, 16, 24, 3, 1, 16, 24)
    ob = Buf(2, 4, 4, 24, 1, 32)
    full = Buf(2, 8, 8, 24, 1, 24)
    bias = torch.linspace(-0.5, 0.5, 24)
    d = _conv_desc(xb, ob, 3, 1, 24, epilogue=2, pool2=pool2)
    if pool2 == 2:
        d.aux_img_stride, d.aux_row_stride, d.aux_px_stride, d.aux_off = full.img, full.row, full.px, full.off()
    R = lr.igemm_ref(d, xb.store, xb.guard, _packed(w), bias)
    act = F.leaky_relu(F.conv2d(_bf(x), _bf(w), bias.double(), padding=1), 0.1)
    pooled, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    assert torch.allclose(lr._out_view(R.ref, d, pooled=True), pooled.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert int(R.addressed.sum()) == pooled.numel()
    got = _store(ob, pooled.float().permute(0, 2, 3, 1))
    if pool2 == 1:
        worst, fails = R.check(got)
    elif pool2 == 2:
        assert torch.allclose(lr._aux_view(R.aux_ref, d), act.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        worst, fails = R.check(got, got_aux=_store(full, act.float().permute(0, 2, 3, 1)))
    else:
        # codes as F.max_pool2d's indices give them: window position 2 * dy + dx, 2 bits per channel, uint16 per 8 channels at (pooled address) / 8
        H = 8
        iy, ix = idx // H, idx % H
        pos = ((iy % 2) * 2 + (ix % 2)).permute(0, 2, 3, 1)            # [N][4][4][C]
        codes = torch.zeros(ob.N * ob.img // 8, dtype=torch.int32)
        addr = lr._out_view(torch.arange(ob.N * ob.img), d, pooled=True)
        codes.index_put_((addr.reshape(-1) // 8,), (pos.reshape(-1).int() << (2 * (addr.reshape(-1) % 8)).int()), accumulate=True)
        worst, fails = R.check(got, got_codes=codes.to(torch.int16))
        assert not fails
        # a wrong position in a window whose maximum is clear is rejected
        vals = R.codes_vals
        top = vals.topk(2, dim=1).values
        clear = int(torch.nonzero((top[:, 0] - top[:, 1]) > 0.05).flatten()[0])
        w_i, sh = int(R.codes_idx[clear]), int(R.codes_shift[clear])
        bad = codes.clone()
        bad[w_i] ^= 1 << sh
        assert R.check(got, got_codes=bad.to(torch.int16))[1]
    assert not fails and worst <= 1.0


@pytest.mark.parametrize("halo_w", [0, 1])
def test_stride2_data_gradient_by_parity_class(halo_w):
    """the data gradient of a stride-2 3x3 conv as four small convs over the non-zero slots of the zero-stuffed gradient (1x1, 1x2, 2x1 and 2x2 taps),
    each writing its parity class of the input gradient through doubled strides (out_px_stride = 2 * Cout)"""
    N, H, cin, cout = 2, 8, 16, 24
    g = torch.Generator().manual_seed(5 + halo_w)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    dy = torch.randn(N, cout, H // 2, H // 2, generator=g)
    want = F.conv_transpose2d(_bf(dy), _bf(w), stride=2, padding=1, output_padding=1)          # [N][cin][H][H]
    gb = Buf(N, H, H, cout, 1)                      # dy zero-stuffed on the input grid
    gb.interior()[:, ::2, ::2, :] = dy.permute(0, 2, 3, 1).to(BF)
    ob = Buf(N, H, H, cin, 1, cin + 8 * halo_w)
    wd = w.permute(1, 2, 3, 0).flip(1, 2)           # [cin][ky'][kx'][cout], ky' = 2 - ky
    sel = {0: [1], 1: [0, 2]}
    seen = torch.zeros(N * ob.img, dtype=torch.int32)
    total = torch.full((N * ob.img,), float("nan"), dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            wc = wd[:, sel[py]][:, :, sel[px]].contiguous().to(BF).reshape(-1)
            d = _desc(N=N, Ho=H // 2, Wo=H // 2, in_img_stride=gb.img, in_row_stride=2 * gb.row, in_px_stride=2 * gb.px, in_off=gb.off(), stride=1,
                      KH=1 + py, KW=1 + px, tap_len=cout, Cout=cin, out_img_stride=ob.img, out_row_stride=2 * ob.row, out_px_stride=2 * ob.px,
                      out_off=ob.off() + py * ob.row + px * ob.px)
            R = lr.igemm_ref(d, gb.store, gb.guard, wc)
            seen += R.addressed.int()
            total[R.addressed] = R.ref[R.addressed]
    assert int(seen.max()) == 1 and int(seen.sum()) == want.numel()         # the four classes tile the interior
    got = total.view(N, ob.Hp, ob.Wp, ob.Cp)[:, 1: 1 + H, 1: 1 + H, :cin]
    assert torch.allclose(got, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def _wgrad_problem(seed, N, H, cin, cout, s, cpad_in, cpad_dy):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, H, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    gy = torch.randn(N, cout, H // s, H // s, generator=g)
    xd = _bf(x).requires_grad_(True)
    wd = _bf(w).requires_grad_(True)
    F.conv2d(xd, wd, stride=s, padding=1).backward(_bf(gy))
    xb = Buf(N, H, H, cin, 1, cpad_in).fill(x)
    gb = Buf(N, H, H, cout, 1, cpad_dy)                 # dy in the input's geometry (zero-stuffed for stride 2)
    gb.interior()[:, ::s, ::s, :] = gy.permute(0, 2, 3, 1).to(BF)
    return wd.grad.permute(0, 2, 3, 1).reshape(cout, -1), _bf(gy).sum((0, 2, 3)), xb, gb


@pytest.mark.parametrize("geo,s", [(False, 1), (True, 1), (True, 2)])
def test_weight_gradient_equals_autograd(geo, s):
    N, H, cin, cout = 2, 8, 16, 24
    want_dw, want_db, xb, gb = _wgrad_problem(40 + s + geo, N, H, cin, cout, s, 24, 32)
    d = SimpleNamespace(P=N * xb.Hp * xb.Wp, dy_px_stride=gb.px, x_px_stride=xb.px, Cout=cout, Cin=cin, KH=3, KW=3, pad=1, x_row_stride=xb.row,
                        geo_W=0)
    if geo:
        d.P, d.geo_W, d.geo_H = N * (H // s) ** 2, H // s, H // s
        d.geo_img_slots, d.geo_row_slots, d.geo_px_slots, d.geo_slot0 = xb.Hp * xb.Wp, s * xb.Wp, s, xb.Wp + 1
    lo, hi = lr.wgrad_extent(d, "x")
    assert -lo <= xb.guard and hi <= xb.guard + N * xb.img            # (the flat form reads into the guard bands)
    dw, db = lr.wgrad_ref(d, xb.store, xb.guard, gb.store, gb.guard)
    assert torch.allclose(dw, want_dw, rtol=1e-12, atol=1e-10)
    assert torch.allclose(db, want_db, rtol=1e-12, atol=1e-10)
    # a float32 result is inside the per-tensor bound, one pixel range of eight left out is not
    assert lr.rel_l2(dw.float(), want_dw) < 1e-6
    if geo:
        d.P = N * (H // s) ** 2 * 7 // 8
        assert lr.rel_l2(lr.wgrad_ref(d, xb.store, xb.guard, gb.store, gb.guard)[0], want_dw) > 1e-3


def test_checker_rejects_sabotaged_outputs():
    """three ways a plan can be subtly wrong: one tap's weights dropped, one of 16 K ranges left out, one 16-pixel tile never written"""
    x, w, xb, ob = _problem(77, 2, 8, 64, 32, 3, 1, 64, 32)
    d = _conv_desc(xb, ob, 3, 1, 32)
    wp = _packed(w)
    R = lr.igemm_ref(d, xb.store, xb.guard, wp)

    def launch(wflat):
        wm = wflat.view(32, 3, 3, 64).permute(0, 3, 1, 2).float()
        return _store(ob, F.conv2d(x.to(BF).float(), wm, padding=1).permute(0, 2, 3, 1))

    good = launch(wp)
    assert not R.check(good)[1]
    no_tap = wp.clone().view(32, 9, 64)
    no_tap[:, 4] = 0
    assert R.check(launch(no_tap.reshape(-1)), what="tap")[1]
    no_range = wp.clone().view(32, 16, 36)              # K = 576 in 16 ranges of 36
    no_range[:, 11] = 0
    assert R.check(launch(no_range.reshape(-1)), what="K range")[1]
    old = torch.randn(ob.N * ob.img).to(BF)
    stale = good.clone()
    lr._out_view(stale, d)[0, 2:4] = lr._out_view(old, d)[0, 2:4]      # flattened output pixels 16 .. 31 keep what the buffer held before
    fails = R.check(stale, what="tile")[1]
    assert fails and "outside their bound" in fails[0]
    for smooth in (False, True):
        _wgrad_sabotage(smooth)


def _wgrad_sabotage(smooth):
    """Four ways a weight gradient can be subtly wrong in an otherwise correct result -- one pixel dropped, one tap shifted by a pixel, two input
    channels swapped, one db element missing one pixel -- over P = 1536 interior pixels (3x3, 16 <- 16 channels).  The element check of
    launch_ref.wgrad_bound flags each of them, on zero-mean noise and on smooth operands.

    Relative L2 at 1e-3 (all tests/test_gpu_plan_table.py asked of a weight gradient) sees a wrong fraction f of zero-mean terms as sqrt(f) and does
    flag these on noise.  On smooth operands -- activations and gradients with a common sign and 3 % variation, as behind a LeakyReLU; x zero on the
    outer ring of the image so that a shifted tap still meets every pixel -- an element is P times a mean, a lost pixel changes it by 1 / P = 6.5e-4,
    a shifted tap or swapped channel by the variation only, and relative L2 passes all four.  That gap is what the element check closes."""
    N, H, cin, cout = 6, 16, 16, 16
    g = torch.Generator().manual_seed(90 + smooth)
    xb, gb = Buf(N, H, H, cin), Buf(N, H, H, cout)
    if smooth:
        xv = 1.0 + 0.03 * torch.randn(N, H, H, cin, generator=g)
        xv[:, 0], xv[:, -1], xv[:, :, 0], xv[:, :, -1] = 0, 0, 0, 0
        gv = 0.1 * (1.0 + 0.03 * torch.randn(N, H, H, cout, generator=g))
    else:
        xv, gv = torch.randn(N, H, H, cin, generator=g), 0.1 * torch.randn(N, H, H, cout, generator=g)
    xb.interior().copy_(xv.to(BF))
    gb.interior().copy_(gv.to(BF))
    d = SimpleNamespace(P=N * H * H, dy_px_stride=gb.px, x_px_stride=xb.px, Cout=cout, Cin=cin, KH=3, KW=3, pad=1, x_row_stride=xb.row, split=1, accumulate=0,
                        geo_W=H, geo_H=H, geo_img_slots=xb.Hp * xb.Wp, geo_row_slots=xb.Wp, geo_px_slots=1, geo_slot0=xb.Wp + 1)
    b = lr.wgrad_bound(d, xb.store, xb.guard, gb.store, gb.guard)
    assert b.n == d.P

    def flagged(dw, db):
        fails = []
        lr.check_values(b.dw, b.dw_bnd, dw.float(), "dw", fails)
        lr.check_values(b.db, b.db_bnd, db.float(), "db", fails)
        return bool(fails), max(lr.rel_l2(dw.float(), b.dw), lr.rel_l2(db.float(), b.db))

    hit, l2 = flagged(b.dw, b.db)
    assert not hit and l2 < 1e-7                                # the fp32 rounding of the reference passes
    dw3 = b.dw.view(cout, 9, cin)
    px = gb.interior()[2, 5, 7].clone()
    gb.interior()[2, 5, 7] = 0
    no_pixel = lr.wgrad_ref(d, xb.store, xb.guard, gb.store, gb.guard)[0].reshape(-1)
    gb.interior()[2, 5, 7] = px
    shifted = dw3.clone()
    shifted[:, 0] = dw3[:, 1]                                   # tap (0, 0) computed one pixel to the right: the values of tap (0, 1)
    swapped = dw3.clone()
    swapped[:, :, 3], swapped[:, :, 5] = dw3[:, :, 5], dw3[:, :, 3]
    db_short = b.db.clone()
    db_short[3] -= px[3].double()
    for name, dw, db in (("pixel", no_pixel, b.db), ("tap", shifted.reshape(-1), b.db), ("channels", swapped.reshape(-1), b.db), ("db", b.dw, db_short)):
        hit, l2 = flagged(dw, db)
        assert hit, (name, smooth)
        assert (l2 < 1e-3) == smooth, (name, smooth, l2)


def test_blocked_weight_panels_are_the_linear_weight():
    """w_blocked = 1: the [ceil(O/128)][K/64][128][64] panels of yolo_pack_fc_weight_blocked (rows >= O zero) describe the same Linear layer"""
    g = torch.Generator().manual_seed(8)
    O, K, N = 200, 192, 3
    w = torch.randn(O, K, generator=g)
    x = torch.randn(N, K, generator=g)
    panels = torch.zeros(2, K // 64, 128, 64)
    wp = torch.zeros(256, K)
    wp[:O] = w
    panels[:] = wp.view(2, 128, K // 64, 64).permute(0, 2, 1, 3)
    d = _desc(N=N, Ho=1, Wo=1, in_img_stride=K, in_row_stride=0, in_px_stride=K, in_off=0, stride=1, KH=1, KW=1, tap_len=K, Cout=O,
              out_img_stride=O, out_row_stride=0, out_px_stride=O, out_off=0, out_fp32=1, w_blocked=1)
    assert lr.igemm_extent(d, "w") == (0, panels.numel())
    R = lr.igemm_ref(d, x.to(BF).reshape(-1), 0, panels.to(BF).reshape(-1))
    assert torch.allclose(R.ref, F.linear(_bf(x), _bf(w)).reshape(-1), rtol=1e-12, atol=1e-12)
    d.w_blocked = 0
    assert lr.igemm_extent(d, "w") == (0, O * K)
    assert torch.equal(lr.igemm_ref(d, x.to(BF).reshape(-1), 0, w.to(BF).reshape(-1)).ref, R.ref)


def _bn_problem(seed, N, H, W, C, ratio):
    """bf16 conv outputs whose channels have |mean| / std = ratio"""
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(C, generator=g) + 0.5
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    z = _bf(sign * ratio * std + std * torch.randn(N, H, W, C, generator=g))
    return z, (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double() * 0.5, g


def _bn_kernel_fwd(z, gamma, beta, eps, L, residual=None, relu=False, lanes_dropped=0):
    """bn.hip's forward arithmetic on the CPU: fp32 lane partials of L pixels, fp64 across lanes, fp32 scale / shift, fma, bf16 store
    (lanes_dropped: the last lanes' partials lost, as a wrong grid stride would)"""
    P, C = z.shape
    zf = z.float()
    nl = -(-P // L)
    pad = torch.zeros(nl * L - P, C)
    lanes = torch.cat([zf, pad]).view(nl, L, C)
    s1 = torch.zeros(nl, C, dtype=torch.float32)
    s2 = torch.zeros(nl, C, dtype=torch.float32)
    for i in range(L):
        s1 += lanes[:, i]
        s2 += lanes[:, i] * lanes[:, i]
    s1, s2 = s1[: nl - lanes_dropped].double().sum(0), s2[: nl - lanes_dropped].double().sum(0)
    mean = s1 / P
    var = (s2 / P - mean * mean).clamp_min(0)
    sc = gamma * (var + eps).rsqrt()
    scale, shift = sc.float(), (beta - mean * sc).float()
    y = (zf.double() * scale.double() + shift.double()).float()      # fma: one rounding of the exact product + sum
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = y.clamp_min(0)
    return y.to(BF).double(), torch.stack([mean, (var + eps).rsqrt(), scale.double(), shift.double()]).float()


@pytest.mark.parametrize("ratio,relu,res", [(1.0, True, False), (10.0, False, True), (30.0, True, False)])
def test_batchnorm_forward_reference_equals_torch(ratio, relu, res):
    N, H, W, C = 2, 9, 11, 64
    z, gamma, beta, g = _bn_problem(int(ratio) + relu, N, H, W, C, ratio)
    r = _bf(torch.randn(N, H, W, C, generator=g)) if res else None
    P = N * H * W
    zz, rr = z.reshape(P, C), (r.reshape(P, C) if res else None)
    L = lr.bn_lane_pixels(P, C)
    assert L == 7                     # 198 pixels over 32 lanes
    mean, var, dm, dv = lr.bn_stats_ref(zz, L)
    R = lr.bn_fwd_ref(zz, mean, var, dm, dv, gamma, beta, 1e-5, rr, relu)
    rm, rv = torch.randn(C, generator=g).double(), torch.rand(C, generator=g).double() + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    want = F.batch_norm(z.permute(0, 3, 1, 2), rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
    if res:
        want = want + r.permute(0, 3, 1, 2)
    if relu:
        want = want.clamp_min(0)
    assert torch.allclose(R.y, want.permute(0, 2, 3, 1).reshape(P, C), rtol=1e-10, atol=1e-10)
    new_m, bm, new_v, bv = lr.bn_running_ref(rm, rv, mean, var, dm, dv, 0.1, P)
    assert torch.allclose(new_m, rm_t, rtol=1e-12, atol=1e-12) and torch.allclose(new_v, rv_t, rtol=1e-12, atol=1e-12)
    # the kernel's own arithmetic lies inside every bound; statistics one pixel lane short and a channel group left stale do not
    y, save = _bn_kernel_fwd(zz, gamma, beta, 1e-5, L, rr, relu)
    fails = []
    assert lr.check_values(R.y, R.bnd, y, "y", fails) <= 1.0 and lr.check_values(R.save, R.save_bnd, save, "save", fails) <= 1.0, fails
    short, _ = _bn_kernel_fwd(zz, gamma, beta, 1e-5, L, rr, relu, lanes_dropped=1)
    assert lr.check_values(R.y, R.bnd, short, "y", fails) > 1.0
    stale = y.clone()
    stale[:, 16:24] = zz[:, 16:24]
    assert lr.check_values(R.y, R.bnd, stale, "y", fails) > 1.0


@pytest.mark.parametrize("mask_from,frozen", [("y", False), ("z", False), (None, False), ("y", True)])
def test_batchnorm_backward_reference_equals_autograd(mask_from, frozen):
    N, H, W, C = 2, 7, 9, 32
    z, gamma, beta, g = _bn_problem(3 + frozen, N, H, W, C, 2.0)
    P = N * H * W
    dy = _bf(torch.randn(N, H, W, C, generator=g))
    rm, rv = torch.randn(C, generator=g).double(), torch.rand(C, generator=g).double() + 0.5
    zc = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    gc, bc = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(zc, rm.clone(), rv.clone(), gc, bc, not frozen, 0.1, 1e-5)
    if mask_from is not None:
        y = y.clamp_min(0)
    y.backward(dy.permute(0, 3, 1, 2))
    zz = z.reshape(P, C)
    if frozen:
        mean, inv = rm, (rv + 1e-5).rsqrt()
    else:
        mean, inv = zz.mean(0), (zz.var(0, unbiased=False) + 1e-5).rsqrt()
    save = torch.stack([mean, inv, gamma * inv, beta - mean * gamma * inv])
    yv = y.detach().permute(0, 2, 3, 1).reshape(P, C)
    mask = {"y": yv > 0, "z": zz * save[2] + save[3] > 0, None: None}[mask_from]
    L = lr.bn_lane_pixels(P, C)
    R = lr.bn_bwd_ref(dy.reshape(P, C), zz, gamma, save, L, mask, frozen)
    assert torch.allclose(R.dz, zc.grad.permute(0, 2, 3, 1).reshape(P, C), rtol=1e-9, atol=1e-9)
    assert torch.allclose(R.dgamma, gc.grad, rtol=1e-9, atol=1e-9) and torch.allclose(R.dbeta, bc.grad, rtol=1e-9, atol=1e-9)
    # an fp32 evaluation in the kernel's order lies inside the bounds
    gf, zf, sv = R.g.float(), zz.float(), save.float()
    xh = (zf - sv[0]) * sv[1]
    s1, s2 = gf.double().sum(0), (gf * xh).double().sum(0)
    c0 = gamma.float() * sv[1]
    c1, c2 = ((s1 / P).float(), (s2 / P).float()) if not frozen else (torch.zeros(C), torch.zeros(C))
    dz = (c0 * (gf - c1 - xh * c2)).to(BF)
    fails = []
    assert lr.check_values(R.dz, R.bnd, dz, "dz", fails) <= 1.0, fails
    assert lr.check_values(R.dbeta, R.dbeta_bnd, s1.float(), "dbeta", fails) <= 1.0, fails
    assert lr.check_values(R.dgamma, R.dgamma_bnd, s2.float(), "dgamma", fails) <= 1.0, fails
    if not frozen:      # the batch terms taken from half the pixels are rejected
        c1h = (gf[: P // 2].double().sum(0) / (P // 2)).float()
        assert lr.check_values(R.dz, R.bnd, (c0 * (gf - c1h - xh * c2)).to(BF), "dz", fails) > 1.0


@pytest.mark.parametrize("H,W", [(8, 10), (7, 9)])
def test_pool_references_equal_torch(H, W):
    g = torch.Generator().manual_seed(H)
    N, C = 2, 16
    x = _bf(torch.relu(torch.randn(N, H, W, C, generator=g)))
    x[:, 2:6, 3:7] = 0.0                     # ties: windows of equal values
    xc = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(xc, 3, 2, 1)
    assert torch.equal(lr.maxpool3s2_ref(x), y.detach().permute(0, 2, 3, 1))
    assert torch.equal(lr.maxpool2_ref(x), F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    dy = _bf(torch.randn(y.shape, generator=g))
    y.backward(dy)
    dx, bnd = lr.maxpool3s2_bwd_ref(x, dy.permute(0, 2, 3, 1))
    want = xc.grad.permute(0, 2, 3, 1)
    assert torch.allclose(dx, want, rtol=1e-12, atol=1e-12)
    fails = []
    assert lr.check_values(dx, bnd, want.float().to(BF), "dx", fails) <= 1.0, fails
    # the gradient of a tied window routed to its LAST maximum is rejected
    Ho, Wo = y.shape[2], y.shape[3]
    last = torch.zeros_like(want)
    for oy in range(Ho):
        for ox in range(Wo):
            win = x[:, max(2 * oy - 1, 0): 2 * oy + 2, max(2 * ox - 1, 0): 2 * ox + 2]           # [N][h][w][C]
            flat = win.reshape(N, -1, C)
            rev = flat.flip(1).argmax(1)                                                       # last maximum
            k = flat.shape[1] - 1 - rev
            wy, wx = k // win.shape[2] + max(2 * oy - 1, 0), k % win.shape[2] + max(2 * ox - 1, 0)
            for n in range(N):
                for c in range(C):
                    last[n, wy[n, c], wx[n, c], c] += dy[n, c, oy, ox]
    assert not torch.equal(last, want)
    assert lr.check_values(dx, bnd, last, "dx", fails) > 1.0
