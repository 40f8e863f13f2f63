"""tests/elementwise_ref.py against stock torch and naive loops (no GPU): the Adam reference against an fp64 torch.optim.Adam, an fp32 emulation of
adam1 inside the propagated bound for every element, the clip coefficient against clip_grad_norm_, the sum-of-squares bound, every layout reference
against a Python loop at a tiny shape -- and the list of ABI entries the two GPU test files must call."""

import os
import re

import numpy as np
import pytest
import torch

import elementwise_ref as er
import launch_ref as lr

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4)


def _state(n, seed, lo=1e-12, hi=1e3):
    """p, g, m, v fp32 with |g| log-uniform in [lo, hi], m and v a previous state of the same scale"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    mag = torch.exp(r() * (np.log(hi) - np.log(lo)) + np.log(lo))
    sign = torch.where(r() < 0.5, -1.0, 1.0)
    g = (mag * sign).float()
    m = (mag * (r() * 2 - 1)).float()
    v = (mag * (0.1 + 0.9 * r())).float() ** 2
    p = torch.randn(n, generator=gen, dtype=torch.float64).float()
    return p, g, m, v


def test_adam_ref_is_torch_adam_in_fp64():
    """five steps of torch.optim.Adam in fp64 with the same (fp32-valued) hyper-parameters: the same formula, so agreement to 1e-12 relative"""
    f = er._f32
    p, g0, m, v = _state(4096, 1, 1e-6, 1e1)
    m, v = torch.zeros_like(m), torch.zeros_like(v)
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=f(HYPER["lr"]), betas=(f(HYPER["beta1"]), f(HYPER["beta2"])), eps=f(HYPER["eps"]), weight_decay=f(HYPER["wd"]))
    P, M, V = p.double(), m.double(), v.double()
    for step in range(1, 6):
        g = (g0.double() * (1.0 + 0.25 * step)).float()
        q.grad = g.double()
        opt.step()
        (P, M, V), _ = er.adam_ref(P, g, M, V, step=step, norm_sq=None, max_norm=10.0, exact_constants=True, **HYPER)
        st = opt.state[q]
        for got, ref, name in ((P, q.detach(), "p"), (M, st["exp_avg"], "m"), (V, st["exp_avg_sq"], "v")):
            rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
            assert rel < 1e-12, f"step {step}: {name} differs from torch.optim.Adam (fp64) by {rel:.3g} relative"


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.5)])
@pytest.mark.parametrize("norm_sq", [None, (10.0 / 0.37) ** 2])
def test_fp32_adam1_lies_inside_the_bound(step, betas, norm_sq):
    """adam1 evaluated in fp32 with one rounding per operation, 2^20 elements, |g| from 1e-12 to 1e3: every element of p, m, v within the bound"""
    p, g, m, v = _state(1 << 20, 7 + step)
    h = dict(HYPER, beta1=betas[0], beta2=betas[1])
    got = er.adam1_fp32(p, g, m, v, step=step, norm_sq=norm_sq, max_norm=10.0, **h)
    refs, bnds = er.adam_ref(p, g, m, v, step=step, norm_sq=norm_sq, max_norm=10.0, **h)
    fails = []
    for name, gt, rf, bd in zip("pmv", got, refs, bnds):
        worst = lr.check_values(rf, bd, gt, name, fails, f"step {step} betas {betas}")
        assert worst > 0.05, f"{name}: worst |err| / bound {worst:.3g}: the bound is far from what fp32 does"
        rel = float((bd / rf.abs().clamp_min(1e-300)).median())
        assert rel < 1e-6, f"{name}: median relative bound {rel:.3g}"
    assert not fails, "\n".join(fails)


def test_adam_ref_rejects_a_wrong_moment():
    """the 1 - b2 -> 1 - b1 slip in the second moment lies far outside the bound"""
    p, g, m, v = _state(4096, 3, 1e-6, 1e3)
    refs, bnds = er.adam_ref(p, g, m, v, step=2, norm_sq=None, max_norm=10.0, **HYPER)
    bad_v = v * np.float32(0.999) + (np.float32(1.0) - np.float32(0.9)) * g * g
    fails = []
    lr.check_values(refs[2], bnds[2], bad_v, "v", fails)
    assert fails


def test_clip_ref_is_clip_grad_norm():
    """grads scaled by torch.nn.utils.clip_grad_norm_ == g * clip_ref(total_norm^2) bit for bit (total_norm fp32: its square is exact in double)"""
    torch.manual_seed(5)
    for scale in (0.01, 1.0, 30.0):
        ps = [torch.zeros(n, requires_grad=True) for n in (1000, 37, 5)]
        for q in ps:
            q.grad = torch.randn_like(q) * scale
        g0 = [q.grad.clone() for q in ps]
        total = torch.nn.utils.clip_grad_norm_(ps, 10.0, foreach=False)
        nsq = float(total.double()) ** 2
        c = er.clip_ref(nsq, 10.0)
        assert (c < 1.0) == (float(total) + 1e-6 > 10.0) or abs(float(total) - 10.0) < 1e-5
        for q, g in zip(ps, g0):
            assert torch.equal(q.grad, g * torch.tensor(c, dtype=torch.float32)), f"scale {scale}"
    assert er.clip_ref(None, 10.0) == 1.0
    # total + 1e-6f == max_norm exactly: c == 1, the `c < 1` branch is not taken; one fp32 step further it is
    below = float(np.nextafter(np.float32(10.0), np.float32(0.0)))
    assert er.clip_ref(below ** 2, 10.0) == 1.0 and er.clip_raw(below ** 2, 10.0) == 1.0
    assert er.clip_ref(100.0, 10.0) < 1.0


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 65537])
def test_sumsq_bound_holds_for_the_kernel_arithmetic(n):
    """fp32 squares and pair sums, fp64 after -- added sequentially and pairwise: both inside sumsq_ref's bound, onto a non-zero accumulator"""
    torch.manual_seed(n)
    g = torch.randn(n) * 3
    acc0 = 123.456
    ref, bnd = er.sumsq_ref(g, acc0)
    body = g[: n // 4 * 4].view(-1, 4)
    sq = body * body
    terms = torch.cat([(sq[:, 0] + sq[:, 1]).double(), (sq[:, 2] + sq[:, 3]).double(), (g[n // 4 * 4:] * g[n // 4 * 4:]).double()])
    seq = acc0
    for t in terms.tolist():
        seq += t
    pair = float(terms.sum()) + acc0
    for got, name in ((seq, "sequential"), (pair, "pairwise")):
        assert abs(got - ref) <= bnd, f"{name}: |{got} - {ref}| > {bnd}"
    assert bnd < 2.1 * er.U * ref + n * 2.0 ** -52 * ref


# ---- layout references against loops --------------------------------------------------------------------------------------------------------------

def _bf(x):
    return torch.tensor(float(x), dtype=torch.float32).to(BF)


def _eq(ref, got, what):
    fails = []
    er.check_exact(ref, got, "ref", fails, what)
    assert not fails, fails[0]


def test_activation_layout_refs():
    torch.manual_seed(0)
    N, C, H, W, Cp, lo, hi = 2, 3, 2, 3, 4, 1, 2
    x = torch.randn(N, C, H, W)
    init = torch.full((N, H + lo + hi, W + lo + hi, Cp), 7.0, dtype=BF)
    want = init.clone()
    for n in range(N):
        for h in range(H):
            for w in range(W):
                for c in range(Cp):
                    want[n, h + lo, w + lo, c] = _bf(x[n, c, h, w]) if c < C else 0.0
    _eq(want, er.nchw_to_nhwc_ref(x, Cp, lo, hi, init), "nchw_to_nhwc")
    halo = 1
    y = torch.randn(N, H + 2, W + 2, C).to(BF)
    for dt in (torch.float32, BF):
        want = torch.zeros(N, C, H, W, dtype=dt)
        for n in range(N):
            for c in range(C):
                for h in range(H):
                    for w in range(W):
                        want[n, c, h, w] = y[n, h + halo, w + halo, c]
        _eq(want, er.nhwc_to_nchw_ref(y, halo, dt), "nhwc_to_nchw")


def test_conv_weight_refs():
    torch.manual_seed(1)
    Co, Ci, KH, KW, Cip, KWp = 3, 2, 2, 3, 4, 4
    w = torch.randn(Co, Ci, KH, KW)
    wf, wd = torch.zeros(Co, KH, KWp, Cip, dtype=BF), torch.zeros(Ci, KH, KW, Co, dtype=BF)
    for co in range(Co):
        for ci in range(Ci):
            for ky in range(KH):
                for kx in range(KW):
                    wf[co, ky, kx, ci] = _bf(w[co, ci, ky, kx])
                    wd[ci, KH - 1 - ky, KW - 1 - kx, co] = _bf(w[co, ci, ky, kx])
    _eq(wf, er.pack_conv_fwd_ref(w, Cip, KWp), "pack fwd")
    _eq(wd, er.pack_conv_dgrad_ref(w), "pack dgrad")
    dwp, dw0 = torch.randn(Co, KH, KWp, Cip), torch.randn(Co, Ci, KH, KW)
    for acc in (0, 1):
        want = dw0.clone()
        for co in range(Co):
            for ci in range(Ci):
                for ky in range(KH):
                    for kx in range(KW):
                        want[co, ci, ky, kx] = (dw0[co, ci, ky, kx] if acc else 0.0) + dwp[co, ky, kx, ci]
        _eq(want, er.unpack_conv_wgrad_ref(dwp, Ci, KW, dw0, acc), f"unpack accumulate={acc}")


def test_fc_weight_refs():
    torch.manual_seed(2)
    O, C, HW = 3, 8, 8
    w = torch.randn(O, C * HW)
    wf = torch.zeros(O, HW * C, dtype=BF)
    for o in range(O):
        for c in range(C):
            for hw in range(HW):
                wf[o, hw * C + c] = _bf(w[o, c * HW + hw])
    got_f, got_t = er.pack_fc_ref(w, C, HW)
    _eq(wf, got_f, "pack_fc")
    _eq(wf.t().contiguous(), got_t, "pack_fc transposed")
    K = C * HW
    for src, got in ((w, er.pack_fc_blocked_ref(w)), (wf.float(), er.pack_fc_blocked_hwc_ref(w, C, HW))):
        want = torch.zeros(1, K // 64, 128, 64, dtype=BF)
        for o in range(O):
            for k in range(K):
                want[0, k // 64, o, k % 64] = _bf(src[o, k])
        _eq(want, got, "blocked")
        assert torch.equal(lr.weight_matrix(got.reshape(-1), O, K, blocked=True), src.to(BF))


def test_transpose_and_im2col_refs():
    torch.manual_seed(3)
    R, Cc, ld, ldx = 3, 5, 4, 7
    x = torch.randn(R, Cc)
    init = torch.full((Cc, ld), 7.0, dtype=BF)
    want = init.clone()
    for r in range(R):
        for c in range(Cc):
            want[c, r] = _bf(x[r, c])
    _eq(want, er.transpose_f32_to_bf16_ref(x, ld, init), "transpose f32")
    xb = torch.randn(R, ldx).to(BF)
    want = init.clone()
    for r in range(R):
        for c in range(Cc):
            want[c, r] = xb[r, c]
    _eq(want, er.transpose_bf16_ref(xb, Cc, init), "transpose bf16")
    N, Ho, Wo, KH, seg, stride, ho, px = 2, 2, 3, 3, 8, 2, 1, 4
    Hin, Win = (Ho - 1) * stride + KH, (Wo - 1) * stride + seg // px
    row, img = Win * px, Hin * Win * px
    xs = torch.randn(N * img).to(BF)
    init = torch.zeros(N, Ho + 2, Wo + 2, KH * seg, dtype=BF)
    want = init.clone()
    for n in range(N):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(KH):
                    for j in range(seg):
                        want[n, oy + ho, ox + ho, ky * seg + j] = xs[n * img + (oy * stride + ky) * row + ox * stride * px + j]
    _eq(want, er.im2col_rows_ref(xs, img, row, px, stride, KH, seg, N, Ho, Wo, ho, init), "im2col_rows")


def test_row_epilogue_refs():
    torch.manual_seed(4)
    S, R, Cc, ld, slope = 3, 2, 5, 8, 0.1
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    x, bias = torch.randn(S, R, Cc), torch.randn(Cc)
    want = torch.zeros(R, Cc)
    for r in range(R):
        for c in range(Cc):
            v = x[0, r, c]
            for s in range(1, S):
                v = v + x[s, r, c]
            v = v + bias[c]
            want[r, c] = v if v > 0 else v * f32(slope)
    yb, yf = er.bias_lrelu_rows_ref(x, bias, slope)
    _eq(want, yf, "bias_lrelu fp32")
    _eq(want.to(BF), yb, "bias_lrelu bf16")
    x2, mask, act = torch.randn(R, Cc), (torch.rand(R, Cc) < 0.5).to(torch.uint8), torch.randn(R, Cc).to(BF)
    act[0, 0], act[0, 1] = 0.0, -0.0
    want = torch.zeros(R, ld, dtype=BF)
    for r in range(R):
        for c in range(Cc):
            v = x2[r, c] * (f32(2.0) if mask[r, c] else f32(0.0))
            v = v * (f32(1.0) if float(act[r, c]) > 0 else f32(slope))
            want[r, c] = v.to(BF)
    _eq(want, er.scale_rows_ref(x2, mask, 2.0, act, slope, ld), "scale_rows")
    xb = torch.randn(R * Cc).to(BF)
    want = torch.zeros(R * Cc, dtype=BF)
    for i in range(R * Cc):
        if mask.reshape(-1)[i]:
            want[i] = (xb[i].float() * f32(2.0)).to(BF)
    _eq(want, er.dropout_ref(xb, mask.reshape(-1), 2.0), "dropout")
    N, C, H, W, halo = 2, 3, 2, 2, 1
    dxT = torch.randn(C * H * W, N)
    ya = torch.randn(N, H + 2, W + 2, C).to(BF)
    for yact in (None, ya):
        init = torch.zeros(N, H + 2, W + 2, C, dtype=BF)
        want = init.clone()
        for n in range(N):
            for c in range(C):
                for h in range(H):
                    for w in range(W):
                        v = dxT[(c * H + h) * W + w, n]
                        if yact is not None and not float(yact[n, h + halo, w + halo, c]) > 0:
                            v = v * f32(slope)
                        want[n, h + halo, w + halo, c] = v.to(BF)
        _eq(want, er.fc_dgrad_to_nhwc_ref(dxT, N, C, H, W, halo, yact, slope, init), "fc_dgrad_to_nhwc")


def test_check_exact_tells_bits_apart():
    a = torch.tensor([0.0, 1.0, float("nan"), float("inf")])
    fails = []
    assert er.check_exact(a, a.clone(), "x", fails) == 0 and not fails
    assert er.check_exact(a, torch.tensor([-0.0, 1.0, float("nan"), float("inf")]), "x", fails) == 1
    assert er.check_exact(a.to(BF), torch.tensor([0.0, 1.0078125, float("nan"), float("inf")]).to(BF), "x", fails) == 1


def test_every_optim_and_layout_entry_is_called_by_the_new_gpu_tests():
    """every YOLO_API entry optim.hip and layout.hip define is named by tests/test_gpu_optim.py or tests/test_gpu_layout.py"""
    src = ""
    for name in ("optim.hip", "layout.hip"):
        with open(os.path.join(ROOT, "yolo-v1_amd", "csrc", name)) as f:
            src += f.read()
    entries = set(re.findall(r"YOLO_API int (yolo_\w+)", src))
    assert len(entries) >= 26, sorted(entries)
    tests = ""
    for name in ("test_gpu_optim.py", "test_gpu_layout.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            tests += f.read()
    called = set(re.findall(r"\.(yolo_\w+)\b", tests))               # attribute access on the loaded library
    missing = sorted(entries - called)
    assert not missing, f"no new GPU test calls {missing}"
