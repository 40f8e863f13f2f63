"""fp64 references of ONE yolo_igemm and ONE yolo_wgrad launch, as include/yolo_hip.h defines them, with element-wise error bounds.

Operands are flat tensors plus element offsets: ``buf[base + i]`` is element i of the pointer the launch receives (base > 0 lets a launch read in
front of its pointer, as the weight gradient's tap offsets and guard bands do).  The CPU tests pass ordinary tensors; the GPU test passes raw views
of the device pointers a launch received.  Descriptors are read by attribute name (a ``yolo._hip.IgemmDesc`` / ``WgradDesc`` or any namespace).

igemm_ref(...) evaluates every output element the descriptor addresses in fp64 from the bf16 operands as stored, and the bound

    |got - ref| <= 2^-8 |ref| + 1.01 Ktot 2^-24 (|patch row| |weight row| + |bias| + |aux|) + 2^-126

(one bf16 rounding plus the worst case of an fp32 sum of Ktot products, by Cauchy-Schwarz); a pooled element takes the largest bound of its window.

wgrad_ref(...) is the fp64 weight and bias gradient of one yolo_wgrad launch, wgrad_bound(...) its element bound gamma(P + ranges - 1 + a) sum |dy| |x|
(fp32 additions of exact products; 0 for operands whose partial sums are all representable).

Below them: BatchNorm forward / backward in training mode (bn.hip) and the pools (pool.hip) on logical NHWC fp64 views, each with a per-element
bound derived from the kernel's arithmetic (check_values compares any region against such a reference).
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EPI_NONE, EPI_BIAS, EPI_BIAS_LRELU, EPI_MUL_DLRELU, EPI_BIAS_ADD_LRELU = 0, 1, 2, 3, 4
CHUNK_BYTES = 256 << 20       # fp64 im2col rows per matmul (the patches of one image at least)
TINY = 2.0 ** -126
U = 2.0 ** -24                # unit roundoff of fp32


def _g(d, name, default=0):
    return int(getattr(d, name, default) or 0)


def igemm_extent(d, what: str):
    """(lo, hi): the launch touches elements [lo, hi) relative to its `what` pointer ("in", "w", "aux", "out", "codes"); lo <= 0"""
    N, Ho, Wo, s, KH, KW, T = _g(d, "N"), _g(d, "Ho"), _g(d, "Wo"), _g(d, "stride"), _g(d, "KH"), _g(d, "KW"), _g(d, "tap_len")
    if what == "in":
        lo = min(0, _g(d, "in_off"))
        hi = ((N - 1) * _g(d, "in_img_stride") + _g(d, "in_off") + ((Ho - 1) * s + KH - 1) * _g(d, "in_row_stride")
              + ((Wo - 1) * s + KW - 1) * _g(d, "in_px_stride") + T)
        return lo, hi
    if what == "w":
        if _g(d, "w_blocked"):
            return 0, (_g(d, "Cout") + 127) // 128 * 128 * KH * KW * T
        return 0, _g(d, "Cout") * KH * KW * T
    if what == "out":
        return 0, N * _g(d, "out_img_stride")
    if what == "codes":
        return 0, (N * _g(d, "out_img_stride") + 7) // 8
    if what == "aux":
        hy, hx = (Ho, Wo)
        return min(0, _g(d, "aux_off")), ((N - 1) * _g(d, "aux_img_stride") + (hy - 1) * _g(d, "aux_row_stride") + (hx - 1) * _g(d, "aux_px_stride")
                                          + _g(d, "aux_off") + _g(d, "Cout"))
    raise ValueError(what)


def _out_view(buf, d, base=0, pooled=False):
    """[N][Ho'][Wo'][Cout] strided view of the output addressing (pooled map if `pooled`)"""
    N, Ho, Wo = _g(d, "N"), _g(d, "Ho"), _g(d, "Wo")
    if pooled:
        Ho, Wo = Ho // 2, Wo // 2
    return buf.as_strided((N, Ho, Wo, _g(d, "Cout")), (_g(d, "out_img_stride"), _g(d, "out_row_stride"), _g(d, "out_px_stride"), 1),
                          buf.storage_offset() + base + _g(d, "out_off"))


def _aux_view(buf, d, base=0):
    return buf.as_strided((_g(d, "N"), _g(d, "Ho"), _g(d, "Wo"), _g(d, "Cout")),
                          (_g(d, "aux_img_stride"), _g(d, "aux_row_stride"), _g(d, "aux_px_stride"), 1), buf.storage_offset() + base + _g(d, "aux_off"))


class IgemmRef:
    """reference of one launch over the output region [0, N * out_img_stride) of its out pointer (halo and padding included):

    addressed      bool [R]   elements the descriptor writes (every image)
    ref, bnd       fp64 [R]   value and bound where checked (NaN / -1 elsewhere: not addressed, or an image outside `images`)
    aux_*          the same over the aux region for pool2 = 2 (un-pooled activation written through aux)
    codes_*        pool2 = 3: per checked pooled element (flat index into the codes buffer, bit shift) the four window values and bounds
    """

    def check(self, got_out, got_aux=None, got_codes=None, what=""):
        """-> (worst |got - ref| / bound, list of failure messages)"""
        fails, worst = [], 0.0
        worst = max(worst, _check_region(self.ref, self.bnd, got_out, "out", fails, what))
        if self.aux_ref is not None:
            worst = max(worst, _check_region(self.aux_ref, self.aux_bnd, got_aux, "aux", fails, what))
        if self.codes_idx is not None:
            _check_codes(self, got_codes, fails, what)
        return worst, fails


def _check_region(ref, bnd, got, tag, fails, what):
    m = bnd >= 0
    if not bool(m.any()):
        return 0.0
    g = got[: ref.numel()].double()[m]
    r, b = ref[m], bnd[m]
    bad_nan = ~torch.isfinite(g)
    err = (g - r).abs()
    ratio = torch.where(bad_nan, torch.full_like(err, math.inf), err / b)
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = int(torch.nonzero(m).flatten()[i])
        nbad = int((ratio > 1.0).sum())
        fails.append(f"{what}: {nbad} of {int(m.sum())} {tag} elements outside their bound (element {idx}: got {float(g[i]):.6g}, "
                     f"ref {float(r[i]):.6g}, bound {float(b[i]):.3g}, ratio {worst:.3g})")
    return worst


def _check_codes(R, got_codes, fails, what):
    words = got_codes.to(torch.int32)[R.codes_idx] & 0xFFFF
    pos = ((words >> R.codes_shift) & 3).long()
    vals, bnds = R.codes_vals, R.codes_bnds                  # [P, 4]
    first = vals.argmax(1)                                    # torch.argmax returns the FIRST maximum
    top2 = vals.topk(2, dim=1)
    b_top = bnds.gather(1, top2.indices)
    certain = (top2.values[:, 0] - top2.values[:, 1]) > 2.0 * b_top.sum(1)
    wrong_certain = certain & (pos != first)
    mx = vals.max(1).values
    vpos = vals.gather(1, pos[:, None])[:, 0]
    bpos = bnds.gather(1, pos[:, None])[:, 0]
    wrong_loose = ~certain & ((mx - vpos) > (bpos + bnds.gather(1, first[:, None])[:, 0]))
    nbad = int(wrong_certain.sum()) + int(wrong_loose.sum())
    if nbad:
        i = int(torch.nonzero(wrong_certain | wrong_loose).flatten()[0])
        fails.append(f"{what}: {nbad} of {vals.shape[0]} arg-max codes wrong (first: code word {int(R.codes_idx[i])} bit {int(R.codes_shift[i])}: "
                     f"position {int(pos[i])}, reference window {[round(float(v), 6) for v in vals[i]]})")


def igemm_ref(d, inp, in_base, w, bias=None, aux=None, aux_base=0, images=None, device=None) -> IgemmRef:
    """fp64 reference of yolo_igemm(d, inp, w, bias, aux, out) (epilogues 0-4, pool2 0-3; px_begin / px_end and split_k are launch details the
    plan layer resolves: the reference describes the whole problem).  inp / w / aux: flat bf16 tensors, bias fp32 [Cout] or None.  images: the
    image indices whose values are computed (None: all); every image's elements count as addressed."""
    N, Ho, Wo, s = _g(d, "N"), _g(d, "Ho"), _g(d, "Wo"), _g(d, "stride")
    KH, KW, T, Co = _g(d, "KH"), _g(d, "KW"), _g(d, "tap_len"), _g(d, "Cout")
    epi, pool2, slope = _g(d, "epilogue"), _g(d, "pool2"), float(getattr(d, "slope", 0.0))
    K = KH * KW * T
    dev = device if device is not None else inp.device
    R = IgemmRef()
    R.aux_ref = R.aux_bnd = R.codes_idx = None
    nreg = N * _g(d, "out_img_stride")
    R.addressed = torch.zeros(nreg, dtype=torch.bool, device=dev)
    _out_view(R.addressed, d, pooled=bool(pool2)).fill_(True)
    R.ref = torch.full((nreg,), math.nan, dtype=torch.float64, device=dev)
    R.bnd = torch.full((nreg,), -1.0, dtype=torch.float64, device=dev)
    if pool2 == 2:
        _, ahi = igemm_extent(d, "aux")
        R.aux_addressed = torch.zeros(ahi, dtype=torch.bool, device=dev)
        R.aux_ref = torch.full_like(R.aux_addressed, math.nan, dtype=torch.float64)
        R.aux_bnd = torch.full_like(R.aux_addressed, -1.0, dtype=torch.float64)
        _aux_view(R.aux_addressed, d).fill_(True)
    wm = weight_matrix(w, Co, K, bool(_g(d, "w_blocked"))).to(dev, torch.float64)
    wn = wm.norm(dim=1)
    b = bias.to(dev, torch.float64)[:Co] if (bias is not None and epi in (EPI_BIAS, EPI_BIAS_LRELU, EPI_BIAS_ADD_LRELU)) else None
    imgs = list(range(N)) if images is None else sorted(set(int(i) for i in images if i < N))
    per_img = Ho * Wo * K * 8
    step = max(1, CHUNK_BYTES // max(1, per_img))
    codes_idx, codes_shift, codes_vals, codes_bnds = [], [], [], []
    ref_v, bnd_v = _out_view(R.ref, d, pooled=bool(pool2)), _out_view(R.bnd, d, pooled=bool(pool2))
    addr = torch.arange(nreg, device=dev) if pool2 == 3 else None
    runs = []
    for i in imgs:
        if runs and runs[-1][1] == i and runs[-1][1] - runs[-1][0] < step:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    for n0, n1 in runs:
        nb = n1 - n0
        A = inp.as_strided((nb, Ho, Wo, KH, KW, T),
                           (_g(d, "in_img_stride"), s * _g(d, "in_row_stride"), s * _g(d, "in_px_stride"), _g(d, "in_row_stride"), _g(d, "in_px_stride"), 1),
                           inp.storage_offset() + in_base + n0 * _g(d, "in_img_stride") + _g(d, "in_off"))
        A = A.to(dev, torch.float64).reshape(nb * Ho * Wo, K)
        acc = A @ wm.T                                                   # [P][Cout]
        gb = A.norm(dim=1)[:, None] * wn[None, :]
        del A
        if b is not None:
            acc = acc + b
            gb = gb + b.abs()
        if epi in (EPI_MUL_DLRELU, EPI_BIAS_ADD_LRELU):
            av = _aux_view(aux, d, aux_base)[n0:n1].to(dev, torch.float64).reshape(nb * Ho * Wo, Co)
            if epi == EPI_MUL_DLRELU:
                acc = acc * torch.where(av > 0, 1.0, slope)
            else:
                acc = acc + av
                gb = gb + av.abs()
        if epi in (EPI_BIAS_LRELU, EPI_BIAS_ADD_LRELU):
            acc = torch.where(acc > 0, acc, acc * slope)
        bound = 2.0 ** -8 * acc.abs() + 1.01 * K * 2.0 ** -24 * gb + TINY
        acc = acc.view(nb, Ho, Wo, Co)
        bound = bound.view(nb, Ho, Wo, Co)
        if not pool2:
            ref_v[n0:n1] = acc
            bnd_v[n0:n1] = bound
            continue
        hq, wq = Ho // 2, Wo // 2
        win = acc[:, :2 * hq, :2 * wq].reshape(nb, hq, 2, wq, 2, Co).permute(0, 1, 3, 5, 2, 4).reshape(nb, hq, wq, Co, 4)
        wb = bound[:, :2 * hq, :2 * wq].reshape(nb, hq, 2, wq, 2, Co).permute(0, 1, 3, 5, 2, 4).reshape(nb, hq, wq, Co, 4)
        ref_v[n0:n1] = win.max(-1).values
        bnd_v[n0:n1] = wb.max(-1).values
        if pool2 == 2:
            _aux_view(R.aux_ref, d)[n0:n1] = acc
            _aux_view(R.aux_bnd, d)[n0:n1] = bound
        elif pool2 == 3:
            pa = _out_view(addr, d, pooled=True)[n0:n1].reshape(-1)
            codes_idx.append(pa // 8)
            codes_shift.append(2 * (pa % 8))
            codes_vals.append(win.reshape(-1, 4))
            codes_bnds.append(wb.reshape(-1, 4))
    if pool2 == 3:
        R.codes_idx, R.codes_shift = torch.cat(codes_idx), torch.cat(codes_shift)
        R.codes_vals, R.codes_bnds = torch.cat(codes_vals), torch.cat(codes_bnds)
    return R


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------------

def _wgrad_pixels(d):
    """(dims, dy strides, x strides, slot0) of the pixel index: flat (one axis over P slots) or the geometry form"""
    if _g(d, "geo_W"):
        H, W = _g(d, "geo_H"), _g(d, "geo_W")
        N = _g(d, "P") // (H * W)
        slots = (_g(d, "geo_img_slots"), _g(d, "geo_row_slots"), _g(d, "geo_px_slots"))
        return (N, H, W), slots, _g(d, "geo_slot0")
    return (_g(d, "P"),), (1,), 0


def wgrad_extent(d, what: str):
    """(lo, hi) of the elements a yolo_wgrad launch reads / writes relative to its `what` pointer ("x", "dy", "dw", "db")"""
    dims, slots, slot0 = _wgrad_pixels(d)
    last = slot0 + sum((n - 1) * st for n, st in zip(dims, slots))
    if what == "dy":
        return slot0 * _g(d, "dy_px_stride"), last * _g(d, "dy_px_stride") + _g(d, "Cout")
    if what == "x":
        pad, xr, xp = _g(d, "pad"), _g(d, "x_row_stride"), _g(d, "x_px_stride")
        return (min(0, slot0 * xp - pad * xr - pad * xp),
                last * xp + (_g(d, "KH") - 1 - pad) * xr + (_g(d, "KW") - 1 - pad) * xp + _g(d, "Cin"))
    if what == "dw":
        return 0, _g(d, "Cout") * _g(d, "KH") * _g(d, "KW") * _g(d, "Cin")
    if what == "db":
        return 0, _g(d, "Cout")
    raise ValueError(what)


def wgrad_ref(d, x, x_base, dy, dy_base=0, device=None, absolute=False):
    """fp64 (dw [Cout][KH*KW*Cin], db [Cout]) of one yolo_wgrad launch, WITHOUT the previous contents of dw / db (the caller adds them where the
    launch accumulates).  dw[co][tap][ci] = sum_p dy[slot(p) * dy_px_stride + co] * x[slot(p) * x_px_stride + tapoff(tap) + ci].
    absolute: -> (dw, db, S_dw, S_db) with S the same sums over |dy| and |x| (one more matmul per chunk): the scale of wgrad_bound"""
    dev = device if device is not None else x.device
    dims, slots, slot0 = _wgrad_pixels(d)
    Co, Ci, KH, KW, pad = _g(d, "Cout"), _g(d, "Cin"), _g(d, "KH"), _g(d, "KW"), _g(d, "pad")
    dyp, xp, xr = _g(d, "dy_px_stride"), _g(d, "x_px_stride"), _g(d, "x_row_stride")
    K = KH * KW * Ci
    dw = torch.zeros(Co, K, dtype=torch.float64, device=dev)
    db = torch.zeros(Co, dtype=torch.float64, device=dev)
    adw, adb = (torch.zeros_like(dw), torch.zeros_like(db)) if absolute else (None, None)
    outer, inner = dims[0], dims[1:]
    n_inner = math.prod(inner) if inner else 1
    step = max(1, CHUNK_BYTES // max(1, n_inner * (K + Co) * 8))
    for a in range(0, outer, step):
        b = min(outer, a + step)
        sz = (b - a,) + tuple(inner)
        base_slot = slot0 + a * slots[0]
        G = dy.as_strided(sz + (Co,), tuple(st * dyp for st in slots) + (1,), dy.storage_offset() + dy_base + base_slot * dyp)
        X = x.as_strided(sz + (KH, KW, Ci), tuple(st * xp for st in slots) + (xr, xp, 1),
                         x.storage_offset() + x_base + base_slot * xp - pad * xr - pad * xp)
        G = G.to(dev, torch.float64).reshape(-1, Co)
        X = X.to(dev, torch.float64).reshape(-1, K)
        dw += G.T @ X
        db += G.sum(0)
        if absolute:
            G.abs_()
            X.abs_()
            adw += G.T @ X
            adb += G.sum(0)
    return (dw, db, adw, adb) if absolute else (dw, db)


def gamma(n) -> float:
    """Higham's gamma_n = n u / (1 - n u) for fp32: the relative error bound of any n chained roundings, second-order terms included (n u < 1)"""
    nu = n * U
    assert nu < 1.0, n
    return nu / (1.0 - nu)


def wgrad_bound(d, x, x_base, dy, dy_base=0, dw0=None, db0=None, ranges=None, exact=False, device=None, refs=None):
    """Value and element bound of one yolo_wgrad launch: -> namespace (dw, dw_bnd [Cout * KH*KW*Cin], db, db_bnd [Cout], n).

    The operands are bf16, so every product dy * x is exact in fp32 (8 + 8 significand bits) and the only roundings are fp32 additions.  An output
    element is the sum of P products, added in some tree inside the MFMA accumulation of a pixel range, plus the additions that join the R pixel
    ranges of a tile (atomics or the slab sum), plus one onto the previous contents where the launch accumulates.  No term passes more than
        n = P + R - 1 + a
    additions whatever the tree or the order, each relative to a partial sum of magnitude <= S = sum_p |dy| |x| (+ |dw0|), so
        |dw - ref| <= gamma(n) (S + |dw0|),     gamma(n) = n u / (1 - n u),  u = 2^-24
    and the same for db with x = 1 (the bf16 -> fp32 conversion is exact).  R = `ranges` (the schedule's exact value), else d.split, else 512 (the
    workgroup slots: the library never splits a tile finer).  dw0 / db0: previous contents (flat fp tensors) where the launch adds onto them, None
    where it stores.  refs: wgrad_ref(..., absolute=True) of the same problem, computed once for several modes.  exact: the operands make every
    partial sum representable (see tests/wgrad_cases.py), so the bound is 0: bit equality.

    Measured on an MI355X: the sum of TWO products comes back up to 1.5 u |sum| off, so the MFMA does not round its internal additions to nearest,
    and the model of one u per addition has the least room at the smallest P: worst |err| / bound 0.76 - 0.99 at P = 2, 0.46 at P = 3, 0.34 at
    P = 4, 0.15 at P = 8, about 0.01 from a hundred pixels on."""
    dev = device if device is not None else x.device
    dw, db, S, Sb = refs if refs is not None else wgrad_ref(d, x, x_base, dy, dy_base, device=dev, absolute=True)
    dw, S = dw.reshape(-1), S.reshape(-1)
    R = int(ranges) if ranges else (_g(d, "split") if _g(d, "split") > 0 else 512)
    out = SimpleNamespace()
    n = out.n = _g(d, "P") + R - 1
    if dw0 is not None:
        dw0 = dw0.to(dev, torch.float64).reshape(-1)
        dw, S = dw + dw0, S + dw0.abs()
    if db0 is not None:
        db0 = db0.to(dev, torch.float64).reshape(-1)
        db, Sb = db + db0, Sb + db0.abs()
    out.dw, out.db = dw, db
    if exact:
        out.dw_bnd, out.db_bnd = torch.zeros_like(S), torch.zeros_like(Sb)
    else:
        out.dw_bnd = gamma(n + (dw0 is not None)) * S
        out.db_bnd = gamma(n + (db0 is not None)) * Sb
    return out


def rel_l2(got, ref) -> float:
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def weight_matrix(w, Co, K, blocked=False):
    """[Cout][K] view of a forward weight operand: row-major, or (blocked, yolo_igemm_desc.w_blocked = 1) the Linear panels
    [ceil(Cout/128)][K/64][128][64] of yolo_pack_fc_weight_blocked"""
    if not blocked:
        return w.as_strided((Co, K), (K, 1), w.storage_offset())
    nb = (Co + 127) // 128
    panels = w.as_strided((nb, 128, K // 64, 64), (128 * K, 64, 128 * 64, 1), w.storage_offset())
    return panels.reshape(nb * 128, K)[:Co]


# ---- element-wise check of any launch ------------------------------------------------------------------------------------------------------------

def check_values(ref, bnd, got, tag, fails, what=""):
    """ref / bnd fp64 over a region, got the region as stored: bnd < 0 not checked, bnd == 0 equal to ref (ref is then the value as stored),
    else |got - ref| <= bnd.  Appends a message to `fails` on a violation; -> worst |err| / bound (0 for exact elements)"""
    m = (bnd >= 0).reshape(-1)
    if not bool(m.any()):
        return 0.0
    g = got.reshape(-1)[: m.numel()].double()[m]
    r, b = ref.reshape(-1)[m], bnd.reshape(-1)[m]
    err = (g - r).abs()
    ratio = torch.where(b > 0, err / b.clamp_min(TINY), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, math.inf))
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        fails.append(f"{what}: {int((ratio > 1.0).sum())} of {int(m.sum())} {tag} elements outside their bound (element {int(torch.nonzero(m).flatten()[i])}: "
                     f"got {float(g[i]):.6g}, ref {float(r[i]):.6g}, bound {float(b[i]):.3g})")
    return worst


# ---- BatchNorm in training mode (bn.hip) ---------------------------------------------------------------------------------------------------------

def bn_lane_pixels(P, C):
    """pixels each lane of bn.hip's statistics / backward-reduction launch adds in fp32: groups of 8 channels, 256 // min(C/8, 256) pixel lanes per
    workgroup, ~32 pixels per lane, at most 2048 workgroups along the pixels (the launch's own grid formula)"""
    gpb = min(C // 8, 256)
    ppb = 256 // gpb
    gy = min(2048, max(1, -(-P // (ppb * 32))))
    return -(-P // (gy * ppb))


def bn_stats_ref(z, L):
    """z fp64 [P][C] -> (mean, biased variance, bound of the kernel's mean, bound of its variance) when each lane adds L values and L squares in fp32
    and the lanes' sums meet in fp64: var = E[z^2] - mean^2 then carries (L + 2) u E[z^2], so |mean| / std of a channel sets its error"""
    P = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    sq = (z * z).sum(0) / P
    dm = 1.01 * (L + 1) * U * z.abs().sum(0) / P
    dv = 1.01 * (L + 2) * U * sq + 2.0 * mean.abs() * dm + dm * dm + 2.0 ** -50 * sq
    return mean, var, dm, dv


def bn_fwd_ref(z, mean, var, dm, dv, gamma, beta, eps, residual=None, relu=False):
    """bn_finalize + bn_apply from fp64 statistics (mean, var) whose kernel values lie within (dm, dv):
    y = [relu](fma(z, scale, shift) [+ residual]) in fp32, scale = fp32(gamma invstd), shift = fp32(beta - mean scale), one bf16 rounding.
    The statistics' errors enter as (z - mean) dscale + dmean scale (shift is formed from the kernel's own mean and scale); the fp32 roundings of
    scale, shift, the fma and the residual add come on top.  -> namespace: y, bnd [P][C]; save, save_bnd [4][C] (mean, invstd, scale, shift)"""
    g, b = gamma.double(), beta.double()
    v = var.clamp_min(0.0)
    inv = (v + eps).rsqrt()
    dinv = torch.maximum(((v - dv).clamp_min(0.0) + eps).rsqrt() - inv, inv - (v + dv + eps).rsqrt())
    scale = g * inv
    dscale = g.abs() * dinv
    shift = b - mean * scale
    t = z * scale + shift
    err = (z - mean).abs() * dscale + dm * (scale.abs() + dscale) + U * (z.abs() * scale.abs() + shift.abs() + t.abs())
    if residual is not None:
        t = t + residual
        err = err + U * t.abs()
    if relu:
        t = t.clamp_min(0.0)
    R = SimpleNamespace(y=t, bnd=(1 + 2.0 ** -8) * 1.01 * err + 2.0 ** -8 * t.abs() + TINY)
    R.save = torch.stack([mean, inv, scale, shift])
    R.save_bnd = 1.01 * torch.stack([dm + U * mean.abs(), dinv + U * inv, dscale + U * scale.abs(),
                                     dm * (scale.abs() + dscale) + mean.abs() * dscale + U * shift.abs()]) + TINY
    return R


def bn_running_ref(rm, rv, mean, var, dm, dv, momentum, P):
    """running_mean / running_var after one update (unbiased variance, as aten) and their bounds"""
    unb = P / (P - 1) if P > 1 else 1.0
    new_m = (1.0 - momentum) * rm.double() + momentum * mean
    new_v = (1.0 - momentum) * rv.double() + momentum * var * unb
    return new_m, momentum * dm + 2.02 * U * new_m.abs() + TINY, new_v, momentum * dv * unb + 2.02 * U * new_v.abs() + TINY


def bn_bwd_ref(dy, z, gamma, save, L, mask=None, frozen=False):
    """bn_bwd_reduce / finalize / apply of one launch from its operands: dy, z fp64 [P][C]; mask bool [P][C] or None; save the forward's fp32 [4][C]
    (mean, invstd, scale, shift).  dy' = dy mask; dbeta = sum dy', dgamma = sum dy' xhat (lanes of L pixels in fp32, fp64 after);
    dz = gamma invstd (dy' - dbeta / P - xhat dgamma / P) in fp32 (frozen: gamma invstd dy'), one bf16 rounding"""
    P = z.shape[0]
    mean, inv = save[0].double(), save[1].double()
    g = dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))
    xh = (z - mean) * inv
    gx = g * xh
    s1, s2 = g.sum(0), gx.sum(0)
    e1 = 1.01 * (L + 1) * U * g.abs().sum(0)
    e2 = 1.01 * (L + 4) * U * gx.abs().sum(0)
    c0 = gamma.double() * inv
    if frozen:
        c1 = c2 = d1 = d2 = torch.zeros_like(s1)
    else:
        c1, c2 = s1 / P, s2 / P
        d1, d2 = e1 / P + U * c1.abs(), e2 / P + U * c2.abs()
    inner = g - c1 - xh * c2
    mag = g.abs() + c1.abs() + (xh * c2).abs()
    dinner = d1 + xh.abs() * d2 + 2.02 * U * xh.abs() * c2.abs() + 3.03 * U * mag
    dz = c0 * inner
    err = c0.abs() * (dinner + 2.02 * U * mag)
    R = SimpleNamespace(g=g, dz=dz, bnd=(1 + 2.0 ** -8) * 1.01 * err + 2.0 ** -8 * dz.abs() + TINY)
    R.dbeta, R.dbeta_bnd = s1, e1 + U * s1.abs() + TINY
    R.dgamma, R.dgamma_bnd = s2, e2 + U * s2.abs() + TINY
    return R


# ---- pools (pool.hip), NHWC fp64 views ----------------------------------------------------------------------------------------------------------

def maxpool2_ref(x):
    """MaxPool2d(2, 2) of x [N][H][W][C] (exact)"""
    N, H, W, C = x.shape
    return x[:, : H // 2 * 2, : W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C).amax((2, 4))


def maxpool3s2_ref(x):
    """MaxPool2d(3, stride 2, pad 1) of x [N][H][W][C] (exact; -inf padding, as the operator)"""
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def maxpool3s2_bwd_ref(x, dy):
    """aten's MaxPool2d(3, 2, 1) backward: each window's dy goes to its FIRST maximum in row-major order; a pixel sums <= 4 windows in fp32, one bf16
    rounding.  x [N][H][W][C], dy [N][Ho][Wo][C] fp64 -> (dx, bound) [N][H][W][C]"""
    N, H, W, C = x.shape
    _, idx = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    idx = idx.reshape(N, C, -1)
    g = dy.permute(0, 3, 1, 2).reshape(N, C, -1)
    dx = torch.zeros(N, C, H * W, dtype=torch.float64, device=x.device).scatter_add_(2, idx, g)
    ab = torch.zeros_like(dx).scatter_add_(2, idx, g.abs())
    dx, ab = (t.view(N, C, H, W).permute(0, 2, 3, 1) for t in (dx, ab))
    return dx, 2.0 ** -8 * dx.abs() + 3.03 * U * ab + TINY
