"""Every ABI entry of csrc/layout.hip, called directly, bit for bit against the index expressions of tests/elementwise_ref.py.

All of them are data movement with at most one rounding or a fixed chain of fp32 operations that cannot contract, so equality is demanded.  Every
output lies between guard bands of a NaN pattern that must survive.  Haloed outputs are run twice: from zeros (the halo, which include/yolo_hip.h
says producers never write, must still be zero) and from a 7.0 fill (it must not have been written with anything else either); outputs a launch
writes completely start from the 7.0 fill.  Rejected shapes are those the C entries test on the host before launching."""


import pytest
import torch

import elementwise_ref as er
import launch_ref as lr

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
E_ARG, E_UNSUPPORTED = -1, -2


def _L():
    from yolo._hip import lib
    return lib()


def _st():
    from yolo._hip import stream
    return stream()


def _ok(rc):
    assert rc == 0, _L().yolo_hip_last_error().decode(errors="replace")


def _rejected(rc, code):
    assert rc == code and _L().yolo_hip_last_error(), f"expected {code}, got {rc}"


def _out(init):
    return er.Guarded(init.cuda())


def _fill(shape, dtype, value=7.0):
    return torch.full(shape, value, dtype=dtype)


def _same(G, ref, what, fails):
    torch.cuda.synchronize()
    er.check_exact(ref, G.t.cpu(), "output", fails, what)
    if not G.guards_ok():
        fails.append(f"{what}: guard band overwritten")


def _report(fails):
    assert not fails, "\n".join(fails[:10])


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- activations ----------------------------------------------------------------------------------------------------------------------------------

def _nchw_case(N, C, H, W, Cpad, lo, hi, fails, src_offset=0):
    x = _randn(N, C, H, W, seed=C * 1000 + W)
    xd = torch.empty(x.numel() + 4, device="cuda")
    xd[src_offset: src_offset + x.numel()] = x.reshape(-1).cuda()
    for fill in (0.0, 7.0):
        init = _fill((N, H + lo + hi, W + lo + hi, Cpad), BF, fill)
        G = _out(init)
        _ok(_L().yolo_nchw_f32_to_nhwc_bf16(xd.data_ptr() + 4 * src_offset, N, C, H, W, G.ptr, Cpad, lo, hi, _st()))
        _same(G, er.nchw_to_nhwc_ref(x, Cpad, lo, hi, init), f"nchw->nhwc N={N} C={C} H={H} W={W} Cpad={Cpad} halo=({lo},{hi}) src+{src_offset} fill={fill}", fails)


def test_nchw_f32_to_nhwc_bf16_image_paths():
    """C <= 4, Cpad = 4: the four-pixel kernel (C = 3, W % 4 == 0, aligned pointers) with both store paths ((w + halo_lo) even / odd), unequal halos;
    the per-pixel kernel for W % 4 != 0, for a source pointer offset by 4 B, and for C = 1, 2, 4"""
    fails = []
    for lo in (0, 1, 2, 3):
        for hi in (lo, 3 - lo):
            for W in (8, 32):
                _nchw_case(2, 3, 3, W, 4, lo, hi, fails)
    for W in (1, 7, 33):
        _nchw_case(2, 3, 3, W, 4, 3, 3, fails)
        _nchw_case(2, 3, 3, W, 4, 0, 1, fails)
    _nchw_case(2, 3, 3, 8, 4, 3, 3, fails, src_offset=1)
    _nchw_case(2, 3, 3, 8, 4, 2, 1, fails, src_offset=1)
    for C in (1, 2, 4):
        for W in (8, 5):
            _nchw_case(2, C, 3, W, 4, 1, 2, fails)
    _nchw_case(1, 3, 224, 224, 4, 3, 3, fails)             # the shipped stem's geometry
    _report(fails)


CW = [(5, 8, 1), (5, 5, 112), (31, 32, 31), (32, 32, 32), (33, 40, 33), (33, 33, 1), (64, 64, 112), (64, 72, 31), (1024, 1024, 33)]


def test_nchw_f32_to_nhwc_bf16_tile_path():
    """general C through the 32 x 32 LDS tile: C and W at the tile edges +-1, Cpad > C (padding channels zero), halos, N * H at the grid limit"""
    fails = []
    for C, Cpad, W in CW:
        for lo, hi in ((1, 1), (0, 0), (3, 1)):
            _nchw_case(2, C, 3, W, Cpad, lo, hi, fails)
    _nchw_case(1, 5, 65535, 1, 8, 0, 0, fails)
    _report(fails)
    x, y = torch.zeros(65536 * 5, device="cuda"), torch.zeros(65536 * 8, dtype=BF, device="cuda")
    _rejected(_L().yolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), 1, 5, 65536, 1, y.data_ptr(), 8, 0, 0, _st()), E_UNSUPPORTED)
    _rejected(_L().yolo_nchw_f32_to_nhwc_bf16(x.data_ptr(), 1, 5, 4, 4, y.data_ptr(), 4, 0, 0, _st()), E_ARG)       # Cpad < C
    _rejected(_L().yolo_nchw_f32_to_nhwc_bf16(None, 1, 5, 4, 4, y.data_ptr(), 8, 0, 0, _st()), E_ARG)


@pytest.mark.parametrize("to", ["f32", "bf16"])
def test_nhwc_bf16_to_nchw(to):
    """yolo_nhwc_bf16_to_nchw_f32 / yolo_nhwc_bf16_to_nchw_bf16: halo 0, 1, 3, the same C / W edges, the halo (filled with 9.0) never read into the result"""
    fn = _L().yolo_nhwc_bf16_to_nchw_f32 if to == "f32" else _L().yolo_nhwc_bf16_to_nchw_bf16
    dt = torch.float32 if to == "f32" else BF
    fails = []
    cases = [(2, C, 3, W, h) for C, _, W in CW for h in (0, 1, 3)] + [(1, 5, 65535, 1, 0), (1, 3, 2, 2, 1)]
    for N, C, H, W, h in cases:
        x = _fill((N, H + 2 * h, W + 2 * h, C), BF, 9.0)
        x[:, h:h + H, h:h + W] = _randn(N, H, W, C, seed=C + W).to(BF)
        G = _out(_fill((N, C, H, W), dt))
        _ok(fn(x.cuda().data_ptr(), N, C, H, W, h, G.ptr, _st()))
        _same(G, er.nhwc_to_nchw_ref(x, h, dt), f"nhwc->nchw {to} N={N} C={C} H={H} W={W} halo={h}", fails)
    _report(fails)
    x, y = torch.zeros(65536 * 5, dtype=BF, device="cuda"), torch.zeros(65536 * 5, dtype=dt, device="cuda")
    _rejected(fn(x.data_ptr(), 1, 5, 65536, 1, 0, y.data_ptr(), _st()), E_UNSUPPORTED)
    _rejected(fn(x.data_ptr(), 1, 5, 4, 4, -1, y.data_ptr(), _st()), E_ARG)


# ---- conv weights -----------------------------------------------------------------------------------------------------------------------------------

CONV = [(64, 3, 7, 7, 4, 8), (64, 64, 1, 1, 64, 1), (128, 64, 3, 3, 64, 3), (64, 192, 3, 3, 192, 3), (5, 3, 3, 3, 8, 4), (30, 7, 1, 3, 7, 3)]


def test_pack_conv_weight():
    """yolo_pack_conv_weight: forward panel with zero padding (Cinp > Cin, KWp > KW; the 7x7x3 -> 64 stem, 1x1, 3x3), flipped data-gradient panel,
    either or both outputs; equal to yolo_pack_conv_weights_multi where that entry accepts the shape"""
    from yolo._hip import ConvPackItem
    fails = []
    for Co, Ci, KH, KW, Cip, KWp in CONV:
        w = _randn(Co, Ci, KH, KW, seed=Co + Ci)
        wd_ = w.cuda()
        rf, rd = er.pack_conv_fwd_ref(w, Cip, KWp), er.pack_conv_dgrad_ref(w)
        for use_f, use_d in ((1, 1), (1, 0), (0, 1)):
            F, D = _out(_fill(rf.shape, BF)), _out(_fill(rd.shape, BF))
            _ok(_L().yolo_pack_conv_weight(wd_.data_ptr(), Co, Ci, KH, KW, Cip, KWp, F.ptr if use_f else None, D.ptr if use_d else None, _st()))
            what = f"pack_conv_weight {Co}x{Ci}x{KH}x{KW} Cinp={Cip} KWp={KWp} outputs=({use_f},{use_d})"
            _same(F, rf if use_f else _fill(rf.shape, BF), what + " forward", fails)
            _same(D, rd if use_d else _fill(rd.shape, BF), what + " dgrad", fails)
        if Co % 64 == 0 and Ci % 64 == 0 and Cip == Ci and KWp == KW:
            F, D = _out(_fill(rf.shape, BF)), _out(_fill(rd.shape, BF))
            it = (ConvPackItem * 1)(ConvPackItem(wd_.data_ptr(), F.ptr, D.ptr, Co, Ci, KH, KW))
            _ok(_L().yolo_pack_conv_weights_multi(it, 1, _st()))
            _same(F, rf, f"pack_conv_weights_multi {Co}x{Ci}x{KH}x{KW} forward", fails)
            _same(D, rd, f"pack_conv_weights_multi {Co}x{Ci}x{KH}x{KW} dgrad", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_pack_conv_weight(x.data_ptr(), 2, 4, 1, 1, 3, 1, x.data_ptr(), None, _st()), E_ARG)      # Cinp < Cin
    _rejected(_L().yolo_pack_conv_weight(x.data_ptr(), 2, 4, 1, 1, 4, 1, None, None, _st()), E_ARG)


def test_unpack_conv_wgrad():
    """yolo_unpack_conv_wgrad: overwrite and accumulate onto a non-zero gradient, padded panels; equal to yolo_unpack_conv_wgrads_multi where accepted"""
    from yolo._hip import ConvUnpackItem
    fails = []
    for Co, Ci, KH, KW, Cip, KWp in CONV:
        dwp, dw0 = _randn(Co, KH, KWp, Cip, seed=Co), _randn(Co, Ci, KH, KW, seed=Ci)
        src = dwp.cuda()
        for acc in (0, 1):
            G = _out(dw0)
            _ok(_L().yolo_unpack_conv_wgrad(src.data_ptr(), Co, Ci, KH, KW, Cip, KWp, G.ptr, acc, _st()))
            _same(G, er.unpack_conv_wgrad_ref(dwp, Ci, KW, dw0, acc), f"unpack_conv_wgrad {Co}x{Ci}x{KH}x{KW} Cinp={Cip} KWp={KWp} accumulate={acc}", fails)
        if Co % 4 == 0 and Ci % 64 == 0 and Cip == Ci and KWp == KW:
            G = _out(dw0)
            it = (ConvUnpackItem * 1)(ConvUnpackItem(src.data_ptr(), G.ptr, Co, Ci, KH, KW))
            _ok(_L().yolo_unpack_conv_wgrads_multi(it, 1, _st()))
            _same(G, er.unpack_conv_wgrad_ref(dwp, Ci, KW, dw0, 0), f"unpack_conv_wgrads_multi {Co}x{Ci}x{KH}x{KW}", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_unpack_conv_wgrad(x.data_ptr(), 2, 4, 1, 3, 4, 2, x.data_ptr(), 0, _st()), E_ARG)       # KWp < KW


# ---- Linear weights ---------------------------------------------------------------------------------------------------------------------------------

def test_pack_fc_weight():
    """yolo_pack_fc_weight: HW = 1 (plain cast) and HW = 49 with C = 1024 (the 50176-wide head at O = 70), C not a multiple of 64, HW = 256 (the LDS
    limit), with and without the transposed copy; HW = 257 rejected"""
    fails = []
    for O, C, HW in ((70, 1024, 1), (70, 1024, 49), (7, 100, 49), (3, 65, 2), (65, 8, 256), (1, 1, 1)):
        w = _randn(O, C * HW, seed=O + C + HW)
        wd_ = w.cuda()
        rf, rt = er.pack_fc_ref(w, C, HW)
        for use_t in (1, 0):
            F, T = _out(_fill(rf.shape, BF)), _out(_fill(rt.shape, BF))
            _ok(_L().yolo_pack_fc_weight(wd_.data_ptr(), O, C, HW, F.ptr, T.ptr if use_t else None, _st()))
            _same(F, rf, f"pack_fc_weight O={O} C={C} HW={HW}", fails)
            _same(T, rt if use_t else _fill(rt.shape, BF), f"pack_fc_weight O={O} C={C} HW={HW} transposed={use_t}", fails)
    _report(fails)
    x = torch.zeros(64 * 257, device="cuda")
    _rejected(_L().yolo_pack_fc_weight(x.data_ptr(), 1, 64, 257, x.data_ptr(), None, _st()), E_UNSUPPORTED)
    _rejected(_L().yolo_pack_fc_weight(x.data_ptr(), 1, 64, 4, None, None, _st()), E_ARG)


def test_pack_fc_weight_blocked():
    """yolo_pack_fc_weight_blocked / _hwc: O below, at and above a 128-row panel and the head's 1470; rows >= O zero; read back through
    launch_ref.weight_matrix(blocked=True) the panels are the source (resp. its (c, hw) -> (hw, c) permutation)"""
    fails = []
    for O, C, HW in [(O, 64, 1) for O in (30, 128, 129, 1470)] + [(O, 1024, 4) for O in (30, 128, 129, 1470)] + [(30, 1024, 49), (129, 8, 8), (5, 24, 8)]:
        K = C * HW
        w = _randn(O, K, seed=O + K)
        wd_ = w.cuda()
        for hwc in (0, 1):
            ref = er.pack_fc_blocked_hwc_ref(w, C, HW) if hwc else er.pack_fc_blocked_ref(w)
            G = _out(_fill(ref.shape, BF))
            if hwc:
                _ok(_L().yolo_pack_fc_weight_blocked_hwc(wd_.data_ptr(), O, C, HW, G.ptr, _st()))
            else:
                _ok(_L().yolo_pack_fc_weight_blocked(wd_.data_ptr(), O, K, G.ptr, _st()))
            what = f"pack_fc_weight_blocked{'_hwc' if hwc else ''} O={O} C={C} HW={HW}"
            _same(G, ref, what, fails)
            src = w.view(O, C, HW).permute(0, 2, 1).reshape(O, K) if hwc else w
            back = lr.weight_matrix(G.t.cpu(), O, K, blocked=True)
            if not torch.equal(back, src.to(BF)):
                fails.append(f"{what}: weight_matrix(blocked) of the panels is not the source")
            rows = G.t.cpu().view((O + 127) // 128, K // 64, 128, 64).permute(0, 2, 1, 3).reshape(-1, K)[O:]
            if bool((rows.view(torch.int16) != 0).any()):
                fails.append(f"{what}: rows >= O are not zero")
    _report(fails)
    x = torch.zeros(4096, device="cuda")
    _rejected(_L().yolo_pack_fc_weight_blocked(x.data_ptr(), 2, 96, x.data_ptr(), _st()), E_ARG)                 # K % 64 != 0
    _rejected(_L().yolo_pack_fc_weight_blocked_hwc(x.data_ptr(), 2, 30, 32, x.data_ptr(), _st()), E_ARG)         # C % 8 != 0
    _rejected(_L().yolo_pack_fc_weight_blocked_hwc(x.data_ptr(), 2, 8, 4, x.data_ptr(), _st()), E_ARG)           # C * HW % 64 != 0


EDGES = (1, 63, 64, 65, 130)


def test_transposes():
    """yolo_transpose_f32_to_bf16 and yolo_transpose_bf16 at the 64 x 64 tile edges +-1, ld > R and ldx > Cc: the columns between R and ld keep their fill"""
    fails = []
    for R in EDGES:
        for Cc in EDGES:
            for pad in (0, 3):
                x = _randn(R, Cc, seed=R * 131 + Cc)
                init = _fill((Cc, R + pad), BF)
                G = _out(init)
                _ok(_L().yolo_transpose_f32_to_bf16(x.cuda().data_ptr(), R, Cc, G.ptr, R + pad, _st()))
                _same(G, er.transpose_f32_to_bf16_ref(x, R + pad, init), f"transpose_f32_to_bf16 R={R} Cc={Cc} ld={R + pad}", fails)
                xb = _randn(R, Cc + 2 * pad, seed=R + Cc).to(BF)
                G = _out(init)
                _ok(_L().yolo_transpose_bf16(xb.cuda().data_ptr(), R, Cc, Cc + 2 * pad, G.ptr, R + pad, _st()))
                _same(G, er.transpose_bf16_ref(xb, Cc, init), f"transpose_bf16 R={R} Cc={Cc} ldx={Cc + 2 * pad} ldy={R + pad}", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_transpose_f32_to_bf16(x.data_ptr(), 4, 4, x.data_ptr(), 3, _st()), E_ARG)
    _rejected(_L().yolo_transpose_bf16(x.data_ptr(), 4, 4, 3, x.data_ptr(), 4, _st()), E_ARG)
    _rejected(_L().yolo_transpose_bf16(x.data_ptr(), 4, 4, 4, x.data_ptr(), 3, _st()), E_ARG)


def test_im2col_rows():
    """yolo_im2col_rows as the executors call it for the 7x7 / stride-2 stem (NHWC4 input with halo 3: pixel stride 4, stride 2, KH 7, seg 32, output
    halo 1), and N = 3 with an odd 5 x 7 output; the output's halo is not written"""
    fails = []
    for N, Ho, Wo in ((2, 8, 16), (3, 5, 7), (1, 1, 1)):
        Hp, Wp = 2 * Ho + 6, 2 * Wo + 6
        x = _randn(N * Hp * Wp * 4, seed=Ho).to(BF)
        for fill in (0.0, 7.0):
            init = _fill((N, Ho + 2, Wo + 2, 7 * 32), BF, fill)
            G = _out(init)
            _ok(_L().yolo_im2col_rows(x.cuda().data_ptr(), Hp * Wp * 4, Wp * 4, 4, 2, 7, 32, N, Ho, Wo, 1, G.ptr, _st()))
            _same(G, er.im2col_rows_ref(x, Hp * Wp * 4, Wp * 4, 4, 2, 7, 32, N, Ho, Wo, 1, init), f"im2col_rows N={N} Ho={Ho} Wo={Wo} fill={fill}", fails)
    _report(fails)
    x = torch.zeros(4096, dtype=BF, device="cuda")
    _rejected(_L().yolo_im2col_rows(x.data_ptr(), 64, 16, 4, 2, 7, 12, 1, 1, 1, 0, x.data_ptr(), _st()), E_ARG)      # seg % 8 != 0


# ---- casts and row epilogues -----------------------------------------------------------------------------------------------------------------------

SPECIAL = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38,     # largest finite fp32 -> inf in bf16
           1.00390625, 1.01171875, -1.00390625, 1.0039062, 1.0039063,              # ties between bf16 neighbours (to even: down, up) and their two sides
           1e-40, -1e-40, 1.401298464324817e-45, 9.183549615799121e-41, 4.591774807899561e-41, 1.1754942106924411e-38]    # subnormals, half the smallest bf16 subnormal
NS = (0, 1, 7, 8, 9, 2047, 2048, 2049, (1 << 20) + 5)


def test_casts():
    """yolo_cast_f32_to_bf16 (round to nearest even as torch's .to(bfloat16); +-0, +-inf, NaN stays NaN, overflow to inf, ties, subnormals) and
    yolo_cast_bf16_to_f32 (exact), bodies of 8 with tails of 1-7"""
    fails = []
    for n in NS:
        x = _randn(n, seed=n) * 100
        k = min(n, len(SPECIAL))
        x[:k] = torch.tensor(SPECIAL[:k])
        if n > 64:
            x[-len(SPECIAL):] = torch.tensor(SPECIAL)          # the scalar tail sees them too
        G = _out(_fill((n,), BF))
        _ok(_L().yolo_cast_f32_to_bf16(er.Guarded(x.cuda()).ptr if n == 0 else x.cuda().data_ptr(), n, G.ptr, _st()))
        _same(G, x.to(BF), f"cast_f32_to_bf16 n={n}", fails)
        xb = x.to(BF)
        if n:
            xb.view(torch.int16)[0] = 0x7FA5                                   # a NaN payload travels as it is
        G = _out(_fill((n,), torch.float32))
        _ok(_L().yolo_cast_bf16_to_f32(er.Guarded(xb.cuda()).ptr if n == 0 else xb.cuda().data_ptr(), n, G.ptr, _st()))
        _same(G, xb.float(), f"cast_bf16_to_f32 n={n}", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_cast_f32_to_bf16(x.data_ptr(), -1, x.data_ptr(), _st()), E_ARG)
    _rejected(_L().yolo_cast_bf16_to_f32(None, 4, x.data_ptr(), _st()), E_ARG)


def test_bias_lrelu_rows():
    """yolo_bias_lrelu_rows and _slabs (1, 2, 7 slabs added in index order in fp32, then bias, then the gate): bias NULL or not, only the bf16 output,
    only the fp32 one, both; zeros and negative zeros among the sums"""
    fails = []
    for R, Cc in ((1, 1), (3, 30), (64, 1470), (5, 257)):
        for slabs in (1, 2, 7):
            x = _randn(slabs, R, Cc, seed=R + Cc + slabs)
            x[:, 0, 0] = 0.0
            if slabs > 1:
                x[1, -1, -1] = -x[0, -1, -1]
            bias = _randn(Cc, seed=Cc)
            bias[0] = -0.0 if slabs == 2 else 0.0
            xd, bd = x.cuda(), bias.cuda()
            for use_bias in (1, 0):
                rb, rf = er.bias_lrelu_rows_ref(x, bias if use_bias else None, 0.1)
                for ub, uf in ((1, 1), (1, 0), (0, 1)):
                    B, F = _out(_fill((R, Cc), BF)), _out(_fill((R, Cc), torch.float32))
                    args = (bd.data_ptr() if use_bias else None, R, Cc, 0.1, B.ptr if ub else None, F.ptr if uf else None, _st())
                    if slabs == 1:
                        _ok(_L().yolo_bias_lrelu_rows(xd.data_ptr(), *args))
                    else:
                        _ok(_L().yolo_bias_lrelu_rows_slabs(xd.data_ptr(), slabs, *args))
                    what = f"bias_lrelu_rows R={R} Cc={Cc} slabs={slabs} bias={use_bias} outputs=({ub},{uf})"
                    _same(B, rb if ub else _fill((R, Cc), BF), what + " bf16", fails)
                    _same(F, rf if uf else _fill((R, Cc), torch.float32), what + " fp32", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_bias_lrelu_rows(x.data_ptr(), None, 2, 2, 0.1, None, None, _st()), E_ARG)
    _rejected(_L().yolo_bias_lrelu_rows_slabs(x.data_ptr(), 0, None, 2, 2, 0.1, None, x.data_ptr(), _st()), E_ARG)


def test_scale_rows_to_bf16():
    """yolo_scale_rows_to_bf16: mask / act NULL or not, ld > Cc (padding columns zero), act exactly 0 and -0 take the slope branch"""
    fails = []
    for R, Cc, ld in ((1, 1, 8), (64, 30, 32), (3, 4096, 4096), (5, 257, 264)):
        x = _randn(R, Cc, seed=R + Cc)
        mask = (torch.rand(R, Cc, generator=torch.Generator().manual_seed(Cc)) < 0.5).to(torch.uint8)
        mask[0, 0] = 2                                                                         # any non-zero byte keeps
        act = _randn(R, Cc, seed=ld).to(BF)
        act.view(-1)[0::7] = 0.0
        act.view(-1)[3::7] = -0.0
        xd, md, ad = x.cuda(), mask.cuda(), act.cuda()
        for um in (1, 0):
            for ua in (1, 0):
                G = _out(_fill((R, ld), BF))
                _ok(_L().yolo_scale_rows_to_bf16(xd.data_ptr(), md.data_ptr() if um else None, 2.0, ad.data_ptr() if ua else None, 0.1, R, Cc, ld, G.ptr, _st()))
                _same(G, er.scale_rows_ref(x, mask if um else None, 2.0, act if ua else None, 0.1, ld), f"scale_rows R={R} Cc={Cc} ld={ld} mask={um} act={ua}", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_scale_rows_to_bf16(x.data_ptr(), None, 1.0, None, 0.1, 2, 4, 3, x.data_ptr(), _st()), E_ARG)      # ld < Cc


def test_dropout_bf16():
    fails = []
    for n in (0, 1, 255, 256, 257, (1 << 16) + 3):
        x = (_randn(n, seed=n) * 10).to(BF)
        mask = (torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5).to(torch.uint8) * 3
        G = _out(_fill((n,), BF))
        xg, mg = er.Guarded(x.cuda()), er.Guarded(mask.cuda())
        _ok(_L().yolo_dropout_bf16(xg.ptr, mg.ptr, 2.0, n, G.ptr, _st()))
        _same(G, er.dropout_ref(x, mask, 2.0), f"dropout n={n}", fails)
    _report(fails)
    _rejected(_L().yolo_dropout_bf16(xg.ptr, None, 2.0, 4, G.ptr, _st()), E_ARG)


def test_fc_dgrad_to_nhwc():
    """yolo_fc_dgrad_to_nhwc: N and C at the 64-wide tile edges, 7 x 7 and 3 x 5 maps, halo 0 and 1 (not written), y_act NULL or not (0 and -0 gate
    to the slope)"""
    fails = []
    cases = [(N, 64, 3, 5, 1) for N in (1, 63, 64, 65)] + [(2, C, 7, 7, h) for C in (30, 64, 1024) for h in (0, 1)] + [(65, 30, 3, 5, 0)]
    for N, C, H, W, h in cases:
        dxT = _randn(C * H * W, N, seed=N + C)
        ya = _randn(N, H + 2 * h, W + 2 * h, C, seed=C).to(BF)
        ya.view(-1)[0::5] = 0.0
        ya.view(-1)[2::5] = -0.0
        dd, yd = dxT.cuda(), ya.cuda()
        for use_y in (1, 0):
            for fill in (0.0, 7.0):
                init = _fill((N, H + 2 * h, W + 2 * h, C), BF, fill)
                G = _out(init)
                _ok(_L().yolo_fc_dgrad_to_nhwc(dd.data_ptr(), N, C, H, W, h, yd.data_ptr() if use_y else None, 0.1, G.ptr, _st()))
                _same(G, er.fc_dgrad_to_nhwc_ref(dxT, N, C, H, W, h, ya if use_y else None, 0.1, init),
                      f"fc_dgrad_to_nhwc N={N} C={C} {H}x{W} halo={h} y_act={use_y} fill={fill}", fails)
    _report(fails)
    x = torch.zeros(64, device="cuda")
    _rejected(_L().yolo_fc_dgrad_to_nhwc(x.data_ptr(), 1, 1, 256, 256, 0, None, 0.1, x.data_ptr(), _st()), E_UNSUPPORTED)     # H * W > 65535
    _rejected(_L().yolo_fc_dgrad_to_nhwc(None, 1, 1, 2, 2, 0, None, 0.1, x.data_ptr(), _st()), E_ARG)
