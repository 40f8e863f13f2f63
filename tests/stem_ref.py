"""fp64 references of the 7x7 / stride-2 / pad-3 stem launches (csrc/stem.hip, stem_wgrad_kernel<MODE> of csrc/wgrad_stem.hip) with element-wise error
bounds, in launch_ref.py's conventions: operands are flat bf16 / fp32 tensors as stored, results are an IgemmRef or (ref, bnd) pairs for check_values.

Forward.  The stem is the yolo_igemm problem the generic path runs: KH 7, KW 8, tap_len 4, stride 2, in_px_stride 4, Cout 64, bias + LeakyReLU, over the
NHWC4 halo-3 input (in_off 0: pixel (-3, -3) is the first element of an image) and the [64][7][8][4] weight panel.  stem_desc() writes that
descriptor as a namespace and launch_ref.igemm_ref evaluates it unchanged: the bound 2^-8 |ref| + 1.01 K 2^-24 (|patch| |w| + |bias|) + 2^-126 with
K = 224, the window rule of pooled elements and the certain / loose rule of arg-max codes are igemm_ref's.  For the fp32-input entry the reference
input is built on the host (stem_input: torch's round-to-nearest-even cast into a zeroed buffer); no device conversion takes part.

Weight gradient.  dw[co][c][ky][kx] = sum_p dy[p][co] x[2 oy + ky - 3][2 ox + kx - 3][c], db[co] = sum_p dy[p][co], in fp64 from the operands as stored.
Products of two bf16 values are exact in fp32, so only additions round:

    |dw - ref| <= 1.01 u A sum_p |dy| |x|        |db - ref| <= 1.01 u A sum_p |dy|        u = 2^-24

with A the number of fp32 additions on the longest path to one output (wgrad_additions).

Pool + LeakyReLU gradient tile (modes 1 and 2 rebuild it per tile): the first maximum of each 2x2 window, in the order (0,0), (0,1), (1,0), (1,1),
receives bf16(fp32(dpool) * (max > 0 ? 1 : slope)), the other three positions 0.  One fp32 product and one round-to-nearest-even cast: the host
reproduces it exactly (pool_lrelu_grad), so that reference has no bound.
"""

from __future__ import annotations

from types import SimpleNamespace

import torch

import launch_ref as lr

BF = torch.bfloat16
TILE_H, TILE_W = 8, 16          # output pixels of one workgroup tile (16 x 32 input pixels)
PART = 64 * 7 * 8 * 4 + 64      # floats of one weight-gradient workgroup's partial: [64][7][8][4] + 64 bias sums
COUT = 64


class Geo:
    """addressing of an NHWC buffer [N][H + 2 halo][W + 2 halo][C]: element strides, the offset of pixel (0, 0) and views of a flat region"""

    def __init__(self, N, H, W, C, halo):
        self.N, self.H, self.W, self.C, self.halo = N, H, W, C, halo
        self.Hp, self.Wp = H + 2 * halo, W + 2 * halo
        self.px, self.row, self.img = C, self.Wp * C, self.Hp * self.Wp * C
        self.off = (halo * self.Wp + halo) * C
        self.numel = N * self.img

    def view(self, flat):
        return flat[: self.numel].view(self.N, self.Hp, self.Wp, self.C)

    def interior(self, flat):
        h = self.halo
        return self.view(flat)[:, h: h + self.H, h: h + self.W, :]

    def mask(self, device=None):
        """bool [numel]: the elements of the interior"""
        m = torch.zeros(self.numel, dtype=torch.bool, device=device)
        self.interior(m).fill_(True)
        return m


def tiles(N, H, W):
    """workgroup tiles of an N x H x W input (output H/2 x W/2)"""
    return N * (H // 2 // TILE_H) * (W // 2 // TILE_W)


def stem_input(x):
    """x fp32 [N][3][H][W] -> (flat bf16 NHWC4 buffer with halo 3, its Geo): torch's round-to-nearest-even cast, channel 3 and the halo zero"""
    N, _, H, W = x.shape
    g = Geo(N, H, W, 4, 3)
    buf = torch.zeros(g.numel, dtype=BF, device=x.device)
    g.interior(buf)[..., :3] = x.permute(0, 2, 3, 1).to(BF)
    return buf, g


def stem_panel(w):
    """w [64][3][7][7] -> the flat bf16 forward operand [64][7][8][4] (kx 7 and channel 3 zero)"""
    p = torch.zeros(w.shape[0], 7, 8, 4, dtype=BF, device=w.device)
    p[:, :, :7, :3] = w.permute(0, 2, 3, 1).to(BF)
    return p.reshape(-1)


def stem_desc(xg: Geo, og: Geo, slope, pool2=0, fg: Geo | None = None):
    """the yolo_igemm descriptor of a stem forward.  og addresses `out` (the pooled map when pool2); pool2 as the stem entries take it: 0, 1, 3, and
    1 with fg (the geometry of out_full) given, which is yolo_igemm's pool2 = 2 with the un-pooled activation written through aux"""
    Ho, Wo = xg.H // 2, xg.W // 2
    d = SimpleNamespace(N=xg.N, Ho=Ho, Wo=Wo, stride=2, KH=7, KW=8, tap_len=4, Cout=COUT, in_img_stride=xg.img, in_row_stride=xg.row, in_px_stride=xg.px,
                        in_off=0, out_img_stride=og.img, out_row_stride=og.row, out_px_stride=og.px, out_off=og.off, epilogue=lr.EPI_BIAS_LRELU,
                        slope=float(slope), pool2=int(pool2), out_fp32=0, split_k=1, w_blocked=0, aux_img_stride=0, aux_row_stride=0, aux_px_stride=0,
                        aux_off=0)
    if fg is not None:
        assert pool2 == 1
        d.pool2 = 2
        d.aux_img_stride, d.aux_row_stride, d.aux_px_stride, d.aux_off = fg.img, fg.row, fg.px, fg.off
    return d


def stem_fwd_ref(d, xbuf, panel, bias, images=None, device=None) -> lr.IgemmRef:
    """igemm_ref of a stem_desc: xbuf / panel flat bf16 (stem_input, stem_panel), bias fp32 [64]"""
    return lr.igemm_ref(d, xbuf, 0, panel, bias, images=images, device=device)


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------------

def wgrad_additions(ntiles, G):
    """fp32 additions on the longest path to one dw / db element, from stem_wgrad_kernel and stem_wgrad_reduce_kernel (csrc/wgrad_stem.hip).
    Workgroup g of G walks the tiles g, g + G, ...: at most ceil(ntiles / G).  Per tile an accumulator element receives the 128 pixel products in
    four v_mfma_f32_16x16x32_bf16 (32 products each, added inside the instruction and to the running accumulator: at most 128 additions however
    the instruction orders them); the bias sum takes 32 pixels per lane and tile (pairs first, then the running sum) plus two cross-lane
    additions at the end.  The reduce kernel then adds the G partials of an element, 16 interleaved slices of ceil(G / 16) and the 16 slice
    sums: fewer than G + 16 <= G + 128.  So A = ceil(ntiles / G) * 128 + G covers both outputs."""
    return -(-ntiles // G) * 128 + G


def wgrad_grid(ntiles, scratch_elems, grid=768):
    """workgroups of a weight-gradient launch (wgrad_stem7_impl): min(tiles, grid, scratch_elems / PART)"""
    return min(ntiles, grid, scratch_elems // PART)


def stem_wgrad_ref(xbuf, xg: Geo, dy, dg: Geo, A, device=None):
    """fp64 (dw [64][3][7][7], dw bound, db [64], db bound) of one weight-gradient launch: xbuf the NHWC4 halo-3 input as stored, dy the flat
    bf16 gradient buffer addressed by dg (un-pooled map, 64 channels), A = wgrad_additions(tiles, G)"""
    dev = device if device is not None else xbuf.device
    N, Ho, Wo = xg.N, xg.H // 2, xg.W // 2
    assert (dg.N, dg.H, dg.W, dg.C) == (N, Ho, Wo, COUT)
    dw = torch.zeros(COUT, 224, dtype=torch.float64, device=dev)
    aw = torch.zeros_like(dw)
    db = torch.zeros(COUT, dtype=torch.float64, device=dev)
    ab = torch.zeros_like(db)
    step = max(1, lr.CHUNK_BYTES // (Ho * Wo * 224 * 8))
    for n0 in range(0, N, step):
        nb = min(step, N - n0)
        X = xbuf.as_strided((nb, Ho, Wo, 7, 8, 4), (xg.img, 2 * xg.row, 2 * xg.px, xg.row, xg.px, 1), xbuf.storage_offset() + n0 * xg.img)
        X = X.to(dev, torch.float64).reshape(nb * Ho * Wo, 224)
        Gd = dg.interior(dy)[n0: n0 + nb].to(dev, torch.float64).reshape(nb * Ho * Wo, COUT)
        dw += Gd.T @ X
        aw += Gd.abs().T @ X.abs()
        db += Gd.sum(0)
        ab += Gd.abs().sum(0)
    oihw = lambda t: t.view(COUT, 7, 8, 4)[:, :, :7, :3].permute(0, 3, 1, 2).contiguous()   # noqa: E731
    return oihw(dw), 1.01 * lr.U * A * oihw(aw), db, 1.01 * lr.U * A * ab


# ---- MaxPool2d(2, 2) + LeakyReLU backward, exact ----------------------------------------------------------------------------------------------

def windows(y):
    """[N][H][W][C] -> [N][H/2][W/2][C][4], window order (0,0), (0,1), (1,0), (1,1)"""
    N, H, W, C = y.shape
    return y.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def first_max(y):
    """y [N][H][W][C] (any float type) -> (maximum [N][H/2][W/2][C], window position 0..3 of its FIRST occurrence)"""
    win = windows(y)
    mx = win.amax(-1)
    first = (win == mx.unsqueeze(-1)).to(torch.int32).argmax(-1)         # argmax returns the first of equal values
    return mx, first


def pool_lrelu_grad(y_full, dpool, slope):
    """y_full bf16 [N][H][W][C], dpool bf16 [N][H/2][W/2][C] -> (dz bf16 [N][H][W][C], pooled bf16, first [N][H/2][W/2][C] int32):
    what yolo_maxpool2_bwd_lrelu writes, bit for bit (fp32 product, round-to-nearest-even cast)"""
    N, H, W, C = y_full.shape
    mx, first = first_max(y_full.float())
    s = torch.tensor(slope, dtype=torch.float32, device=y_full.device)
    gv = (dpool.float() * torch.where(mx > 0, torch.ones_like(s), s)).to(BF)
    tile = torch.zeros(N, H // 2, W // 2, C, 4, dtype=BF, device=y_full.device)
    tile.scatter_(-1, first.long().unsqueeze(-1), gv.unsqueeze(-1))
    dz = tile.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    return dz, mx.to(BF), first


def pack_codes(first, pg: Geo):
    """first [N][H][W][C] window positions of the pooled map pg addresses -> int16 [pg.numel / 8]: the uint16 word at (element address) / 8
    holds 2 bits per channel of its 8-channel chunk; words of halo pixels are zero"""
    N, H, W, C = first.shape
    f8 = first.to(torch.int32).reshape(N, H, W, C // 8, 8)
    word = sum(f8[..., k] << (2 * k) for k in range(8))
    words = torch.zeros(pg.N, pg.Hp, pg.Wp, C // 8, dtype=torch.int32, device=first.device)
    h = pg.halo
    words[:, h: h + H, h: h + W] = word
    return words.to(torch.int16).reshape(-1)             # values < 2^16: the cast keeps the bit pattern


def unpack_codes(codes, pg: Geo):
    """int16 code words over the region of pg -> [N][H][W][C] window positions of the interior"""
    c = codes[: pg.numel // 8].to(torch.int32) & 0xFFFF
    c = c.view(pg.N, pg.Hp, pg.Wp, pg.C // 8)
    pos = torch.stack([(c >> (2 * k)) & 3 for k in range(8)], dim=-1).reshape(pg.N, pg.Hp, pg.Wp, pg.C)
    h = pg.halo
    return pos[:, h: h + pg.H, h: h + pg.W]
