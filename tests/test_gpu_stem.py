"""The 7x7 / stride-2 stem family, launch by launch through the C ABI, against the fp64 references of tests/stem_ref.py:

  yolo_conv_stem7_fwd, yolo_conv_stem7_fwd_f32            csrc/stem.hip          (persistent, two-buffer pipeline, stores one iteration late)
  yolo_wgrad_stem7, yolo_wgrad_stem7_pooled, _codes       csrc/wgrad_stem.hip    (stem_wgrad_kernel<0 / 1 / 2> + stem_wgrad_reduce_kernel)
  yolo_maxpool3s2_fwd                                     csrc/pool.hip

Every addressed output element lies within its derived bound (arg-max codes by igemm_ref's rule), the entries that promise equal bits give equal
bits, every element a launch does not address keeps the bit pattern it was pre-filled with (halo rings, guard bands, code words of halo pixels,
scratch behind the partials), and the persistent loops are walked for one, two and three trips with both exits.

Geometries are input N x H x W; a tile is 8 x 16 output pixels = 16 x 32 input pixels.
"""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import launch_ref as lr
import stem_ref as sr

pytestmark = pytest.mark.gpu

FWD_GRID = 1024      # csrc/stem.hip:332 and :365, yolo_conv_stem7_fwd / _fwd_f32: `const long G = std::min<long>(nt, 1024);`
WGRAD_GRID = 768     # csrc/wgrad_stem.hip:297, wgrad_stem7_impl: `long G = std::min<long>(nt, 768);`
PART = sr.PART       # csrc/wgrad_stem.hip: ST_PART = 64 * ST_COLS + 64 floats per workgroup partial

CASES = {
    "A": (1, 16, 32),        # one tile: all four image borders inside it
    "B": (2, 48, 32),        # 3 x 1 tiles per image
    "C": (2, 16, 96),        # 1 x 3 tiles per image
    "D": (3, 96, 128),       # 72 tiles
    "E": (17, 128, 256),     # 1088 tiles: forward workgroups 0..63 take two tiles, the rest one (both loop exits)
    "F": (34, 128, 256),     # 2176 tiles: workgroups 0..127 take three tiles (back to buffer A), the rest two
}
BF = torch.bfloat16
PAT16, PAT32 = 0x5AA5, 0x5AA55AA5
GUARD = 4096
DEV = "cuda"


def _api():
    from yolo import _hip
    return _hip


class PB:
    """n elements of 2 or 4 bytes on the device between two guard bands, everything pre-filled with a fixed bit pattern"""

    def __init__(self, n, size=2):
        self.n, self.size = n, size
        self.store = torch.full((n + 2 * GUARD,), PAT16 if size == 2 else PAT32, dtype=torch.int16 if size == 2 else torch.int32, device=DEV)
        self.pat = PAT16 if size == 2 else PAT32

    @property
    def region(self):
        return self.store[GUARD: GUARD + self.n]

    def bf(self):
        return self.region.view(BF)

    def f32(self):
        return self.region.view(torch.float32)

    def ptr(self, elems=0):
        return ctypes.c_void_p(self.region.data_ptr() + elems * self.size)

    def check(self, addressed, what, fails, written=True):
        """the guard bands and every element outside `addressed` (bool [n]) kept the pattern; every addressed element lost it (`written`: not
        asked of arg-max code words, one in 2^16 of which is the pattern by right)"""
        keep = self.store == self.pat
        if not bool(keep[:GUARD].all()) or not bool(keep[GUARD + self.n:].all()):
            fails.append(f"{what}: guard band written")
        k = keep[GUARD: GUARD + self.n]
        if bool((~k & ~addressed).any()):
            fails.append(f"{what}: {int((~k & ~addressed).sum())} elements outside the addressed set written")
        if written and bool((k & addressed).any()):
            fails.append(f"{what}: {int((k & addressed).sum())} addressed elements not written")


def _p(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Problem:
    """random images, weights and bias of one case: the fp32 batch, the host-built NHWC4 halo-3 bf16 buffer, the weight panel"""

    def __init__(self, case, seed=1):
        self.N, self.H, self.W = CASES[case]
        g = _gen(seed + ord(case))
        x = torch.randn(self.N, 3, self.H, self.W, generator=g)              # distinct images: a stale patch or tile of another image must show
        w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
        b = torch.randn(64, generator=g) * 0.5
        self.set(x, w, b)

    def set(self, x, w, b):
        xbuf, self.xg = sr.stem_input(x)                                      # torch's cast on the host, no device conversion kernel
        self.x, self.xbuf, self.panel, self.bias = x.to(DEV), xbuf.to(DEV), sr.stem_panel(w).to(DEV), b.to(DEV)
        self.Ho, self.Wo = self.H // 2, self.W // 2
        self.ntiles = sr.tiles(self.N, self.H, self.W)
        return self


def _forward(P, entry, slope, pool2, og, fg=None, chunk=None):
    """one forward (or one per `chunk` images into the same buffers) -> (out PB, out_full / codes PB or None)"""
    H_ = _api()
    L, st = H_.lib(), H_.stream()
    out = PB(og.numel)
    second = PB(og.numel // 8) if pool2 == 3 else PB(fg.numel) if fg is not None else None
    fimg, frow, foff = (fg.img, fg.row, fg.off) if fg is not None else (0, 0, 0)
    step = chunk or P.N
    for n0 in range(0, P.N, step):
        nb = min(step, P.N - n0)
        sp = None if second is None else second.ptr(n0 * (og.img // 8 if pool2 == 3 else fg.img))
        if entry == "f32":
            rc = L.yolo_conv_stem7_fwd_f32(_p(P.x, n0 * 3 * P.H * P.W), _p(P.panel), _p(P.bias), nb, P.H, P.W, slope, pool2, out.ptr(n0 * og.img), og.img,
                                           og.row, og.off, sp, fimg, frow, foff, st)
        else:
            rc = L.yolo_conv_stem7_fwd(_p(P.xbuf, n0 * P.xg.img), _p(P.panel), _p(P.bias), nb, P.Ho, P.Wo, P.xg.img, P.xg.row, slope, pool2,
                                       out.ptr(n0 * og.img), og.img, og.row, og.off, sp, fimg, frow, foff, st)
        H_.check(rc, f"stem forward {entry}")
    return out, second


def _geos(P, pool2, oh, fh=None):
    og = sr.Geo(P.N, P.Ho // 2, P.Wo // 2, 64, oh) if pool2 else sr.Geo(P.N, P.Ho, P.Wo, 64, oh)
    fg = sr.Geo(P.N, P.Ho, P.Wo, 64, fh) if fh is not None else None
    return og, fg


def _code_words(addressed):
    words = torch.zeros(addressed.numel() // 8, dtype=torch.bool, device=addressed.device)
    words[torch.nonzero(addressed).flatten() // 8] = True
    return words


# (name, slope, pool2, out halo, out_full halo or None)
CONFIGS = [("pool0", 0.1, 0, 1, None), ("pool0", 0.1, 0, 0, None), ("pool1", 0.1, 1, 1, None), ("pool1", 0.1, 1, 0, None),
           ("pool1+full", 0.1, 1, 1, 0), ("pool1+full", 0.1, 1, 0, 1), ("pool3", 0.1, 3, 1, None), ("pool3", 0.1, 3, 0, None),
           ("relu", 0.0, 0, 1, None), ("relu", 0.0, 0, 0, None)]


@pytest.mark.parametrize("case", list(CASES))
def test_forward_entries_against_fp64(case):
    """both forward entries in every mode: within igemm_ref's bound, equal bits between the entries, untouched memory, fused pool == pool after,
    and (more than one tile per workgroup) equal bits to launches of at most 1024 tiles, whose workgroups take one tile each"""
    H_ = _api()
    P = Problem(case)
    large = P.ntiles > FWD_GRID
    fails, worst, kept = [], {}, {}
    for name, slope, pool2, oh, fh in CONFIGS:
        tag = f"{case} {name} halo {oh}/{fh}"
        og, fg = _geos(P, pool2, oh, fh)
        R = sr.stem_fwd_ref(sr.stem_desc(P.xg, og, slope, pool2, fg), P.xbuf, P.panel, P.bias, device=DEV)
        out, second = _forward(P, "bf16", slope, pool2, og, fg)
        out32, second32 = _forward(P, "f32", slope, pool2, og, fg)
        if not torch.equal(out.store, out32.store) or (second is not None and not torch.equal(second.store, second32.store)):
            fails.append(f"{tag}: the fp32-input entry differs from the bf16-input entry")
        r, f = R.check(out.bf(), second.bf() if fg is not None else None, second.region if pool2 == 3 else None, what=tag)
        worst[name] = max(worst.get(name, 0.0), r)
        fails += f
        out.check(R.addressed, f"{tag} out", fails)
        if fg is not None:
            second.check(fg.mask(DEV), f"{tag} out_full", fails)
        if pool2 == 3:
            second.check(_code_words(R.addressed), f"{tag} codes", fails, written=False)      # (their values: R.check above)
        if large:
            per = FWD_GRID // (P.ntiles // P.N)               # 16 images = 1024 tiles
            for entry in ("bf16", "f32"):
                o2, s2 = _forward(P, entry, slope, pool2, og, fg, chunk=per)
                if not torch.equal(o2.store, out.store) or (second is not None and not torch.equal(s2.store, second.store)):
                    fails.append(f"{tag}: {entry} entry, one launch differs from launches of {per} images (one tile per workgroup)")
        kept[(name, oh)] = (og, out, fg, second)
    # the modes against each other, bit for bit: fused pool == yolo_maxpool2_fwd of the stored activation, every pooled map the same, out_full == pool2 = 0
    og0, out0, _, _ = kept[("pool0", 1)]
    pg = sr.Geo(P.N, P.Ho // 2, P.Wo // 2, 64, 1)
    after = PB(pg.numel)
    pd = H_.PoolDesc(P.N, P.Ho, P.Wo, 64, 1, 1)
    H_.check(H_.lib().yolo_maxpool2_fwd(ctypes.byref(pd), out0.ptr(), after.ptr(), H_.stream()), "maxpool2_fwd")
    after.check(pg.mask(DEV), f"{case} yolo_maxpool2_fwd", fails)
    want = pg.interior(after.region)
    for (name, oh), (og, out, fg, second) in kept.items():
        if name.startswith("pool") and name != "pool0" and not torch.equal(og.interior(out.region), want):
            fails.append(f"{case} {name} halo {oh}: fused pool differs from pool2 = 0 followed by yolo_maxpool2_fwd")
        if fg is not None and not torch.equal(fg.interior(second.region), og0.interior(out0.region)):
            fails.append(f"{case} {name} halo {oh}: out_full differs from the pool2 = 0 output")
    print(f"\nstem forward {case} ({P.ntiles} tiles): worst |err| / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()), flush=True)
    assert not fails, "\n".join(fails)


def test_forward_exact_integers_and_tied_windows():
    """operands whose every pre-activation, activation and pooled value is exact in bf16 (x, w in {-1, 0, 1}, integer bias, slope 0.5): the device
    equals the fp64 reference bit for bit in every mode and the codes equal max_pool2d's indices, on windows of which many are tied"""
    P = Problem("D")
    g = _gen(77)
    x = torch.randint(-1, 2, (P.N, 3, P.H, P.W), generator=g).float()
    w = torch.randint(0, 2, (64, 3, 7, 7), generator=g).float() * 2 - 1
    w = w * (torch.rand(64, 3, 7, 7, generator=g) < 0.15)
    b = torch.randint(-2, 3, (64,), generator=g).float()
    P.set(x, w, b)
    act = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3), 0.5) + 0.0       # (+ 0.0: no negative zero)
    assert torch.equal(act.to(BF).double(), act), "the recipe must stay exact in bf16"
    pooled, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    first = (((idx // P.Wo) % 2) * 2 + (idx % P.Wo) % 2).permute(0, 2, 3, 1).to(torch.int32).to(DEV)
    win = sr.windows(act.permute(0, 2, 3, 1))
    tied = float(((win == win.amax(-1, keepdim=True)).sum(-1) > 1).double().mean())
    assert tied >= 0.1, f"only {tied:.3f} of the windows are tied"
    act_b = act.permute(0, 2, 3, 1).to(BF).to(DEV).view(torch.int16)
    pooled_b = pooled.permute(0, 2, 3, 1).to(BF).to(DEV).view(torch.int16)
    fails = []
    for name, _, pool2, oh, fh in CONFIGS[:8]:
        og, fg = _geos(P, pool2, oh, fh)
        for entry in ("bf16", "f32"):
            out, second = _forward(P, entry, 0.5, pool2, og, fg)
            tag = f"{name} halo {oh}/{fh} {entry}"
            if not torch.equal(og.interior(out.region), pooled_b if pool2 else act_b):
                fails.append(f"{tag}: output differs from the exact reference")
            if fg is not None and not torch.equal(fg.interior(second.region), act_b):
                fails.append(f"{tag}: out_full differs from the exact reference")
            if pool2 == 3 and not torch.equal(sr.unpack_codes(second.region, og), first):
                n = int((sr.unpack_codes(second.region, og) != first).sum())
                fails.append(f"{tag}: {n} arg-max codes differ from max_pool2d's indices (first maximum)")
    print(f"\nstem forward exact integers: max |y| {float(act.abs().max()):g}, tied windows {tied:.3f}", flush=True)
    assert not fails, "\n".join(fails)


def test_f32_entry_rounds_to_nearest_even_at_ties():
    """fp32 inputs whose low 16 bits are exactly 0x8000 (a tie between two bf16 values; even and odd upper halves, both signs) and their two fp32
    neighbours, at every pixel of the images (corners, first and last column of every tile): the fp32-input entry equals the bf16-input entry on
    the buffer the host rounded to nearest even"""
    P = Problem("A")
    P.N, P.H, P.W = 2, 32, 64                      # 2 x 2 tiles per image
    g = _gen(31)
    shape = (P.N, 3, P.H, P.W)
    sign = torch.randint(0, 2, shape, generator=g)
    expo = torch.randint(122, 130, shape, generator=g)                     # |x| in [2^-5, 2^3)
    man = torch.randint(0, 128, shape, generator=g)
    upper = (sign << 15) | (expo << 7) | man
    low = torch.tensor([0x8000, 0x8000, 0x7FFF, 0x8001])[torch.randint(0, 4, shape, generator=g)]
    bits = (upper << 16) | low
    x = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    P.set(x, w, torch.randn(64, generator=g) * 0.5)
    # the reference itself: ties go to the even upper half, the neighbours down / up
    got = (sr.Geo(P.N, P.H, P.W, 4, 3).interior(P.xbuf.cpu())[..., :3].permute(0, 3, 1, 2).contiguous().view(torch.int16).to(torch.int64)) & 0xFFFF
    want = torch.where(low == 0x7FFF, upper, torch.where(low == 0x8001, upper + 1, upper + (upper & 1)))
    assert torch.equal(got, want)
    tie = low == 0x8000
    odd = (upper & 1) == 1
    assert int((tie & odd).sum()) > 100 and int((tie & ~odd).sum()) > 100 and int((tie & (sign == 1)).sum()) > 100
    fails = []
    for pool2, oh in ((0, 1), (3, 0)):
        og, _ = _geos(P, pool2, oh)
        a, a2 = _forward(P, "bf16", 0.1, pool2, og)
        b, b2 = _forward(P, "f32", 0.1, pool2, og)
        if not torch.equal(a.store, b.store) or (a2 is not None and not torch.equal(a2.store, b2.store)):
            n = int((a.store != b.store).sum())
            fails.append(f"pool2 {pool2}: {n} output elements differ between the fp32-input entry and the host-rounded buffer")
    assert not fails, "\n".join(fails)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------------------

def _zeros(geo):
    return torch.zeros(geo.numel, dtype=BF, device=DEV)


def _wgrad(P, mode, a, ag, scratch_elems, dpool=None, pg=None, codes=None, slope=0.1, x_row=None, a_off=None, Ho=None):
    """one weight-gradient launch: mode 0 (a = gradient, geometry ag), 1 (a = un-pooled activation ag, dpool pg), 2 (a = pooled activation, codes,
    dpool, all pg) -> (rc, dw, db, scratch PB); dw / db pre-filled with NaN, the scratch with the pattern"""
    H_ = _api()
    L, st = H_.lib(), H_.stream()
    dw = torch.full((64, 3, 7, 7), float("nan"), device=DEV)
    db = torch.full((64,), float("nan"), device=DEV)
    scratch = PB(scratch_elems, 4)
    xr = P.xg.row if x_row is None else x_row
    Ho = P.Ho if Ho is None else Ho
    if mode == 0:
        rc = L.yolo_wgrad_stem7(_p(P.xbuf), _p(a), P.N, Ho, P.Wo, P.xg.img, xr, ag.img, ag.row, ag.off if a_off is None else a_off, _p(dw), _p(db),
                                scratch.ptr(), scratch_elems, st)
    elif mode == 1:
        rc = L.yolo_wgrad_stem7_pooled(_p(P.xbuf), _p(a), P.N, Ho, P.Wo, P.xg.img, xr, ag.img, ag.row, ag.off if a_off is None else a_off, _p(dpool),
                                       pg.img, pg.row, pg.off, slope, _p(dw), _p(db), scratch.ptr(), scratch_elems, st)
    else:
        rc = L.yolo_wgrad_stem7_codes(_p(P.xbuf), _p(a), _p(codes), P.N, Ho, P.Wo, P.xg.img, xr, _p(dpool), pg.img, pg.row,
                                      pg.off if a_off is None else a_off, slope, _p(dw), _p(db), scratch.ptr(), scratch_elems, st)
    return rc, dw, db, scratch


def _scratch_addressed(scratch, G):
    m = torch.zeros(scratch.n, dtype=torch.bool, device=DEV)
    m[: G * PART] = True
    return m


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_weight_gradient_entries_against_fp64(case):
    """the three entries with 1, 5 and the default number of workgroups: within the dw / db bounds of the fp64 reference, bit-reproducible, the
    scratch behind the partials untouched; the pooled and codes entries equal the gradient entry on the tile the host (and
    yolo_maxpool2_bwd_lrelu) builds, bit for bit; codes and pooled map as the host packs them and as the forward with pool2 = 3 leaves them"""
    H_ = _api()
    P = Problem(case, seed=3)
    N, Ho, Wo, nt = P.N, P.Ho, P.Wo, P.ntiles
    g = _gen(40 + ord(case))
    fails, worst = [], {}
    yg, pg, dg = sr.Geo(N, Ho, Wo, 64, 1), sr.Geo(N, Ho // 2, Wo // 2, 64, 0 if case in "BD" else 1), sr.Geo(N, Ho, Wo, 64, 0 if case in "CD" else 1)
    # operands: a random gradient; an activation full of ties, zeros and negatives with a random pooled gradient
    dy = _zeros(dg)
    dg.interior(dy).copy_((torch.randn(N, Ho, Wo, 64, generator=g) * 0.25).to(BF))
    vals = torch.tensor([-1.0, -0.25, 0.0, 0.5, 2.0])
    yi = vals[torch.randint(0, 5, (N, Ho, Wo, 64), generator=g)].to(BF)
    dpi = torch.randn(N, Ho // 2, Wo // 2, 64, generator=g).to(BF)
    dz_h, pooled_h, first_h = sr.pool_lrelu_grad(yi, dpi, 0.1)                  # on the host: fp32 product, torch's cast
    yfull, dpool, ypool = _zeros(yg), _zeros(pg), _zeros(pg)
    yg.interior(yfull).copy_(yi)
    pg.interior(dpool).copy_(dpi)
    pg.interior(ypool).copy_(pooled_h)
    codes_h = sr.pack_codes(first_h, pg).to(DEV)
    # the gradient tile as yolo_maxpool2_bwd_lrelu writes it == the host's, bit for bit; it then feeds the gradient entry
    dz = PB(yg.numel)
    pd = H_.PoolDesc(N, Ho, Wo, 64, yg.halo, pg.halo)
    H_.check(H_.lib().yolo_maxpool2_bwd_lrelu(ctypes.byref(pd), _p(yfull), _p(dpool), 0.1, dz.ptr(), H_.stream()), "maxpool2_bwd_lrelu")
    dz.check(yg.mask(DEV), f"{case} yolo_maxpool2_bwd_lrelu", fails)
    if not torch.equal(yg.interior(dz.region), dz_h.to(DEV).view(torch.int16)):
        fails.append(f"{case}: the host's gradient tile differs from yolo_maxpool2_bwd_lrelu's")
    # what the forward leaves on the same input: pool2 = 3 (pooled map + codes) and pool2 = 1 with out_full
    f_pool3, f_codes = _forward(P, "bf16", 0.1, 3, pg)
    f_pool1, f_full = _forward(P, "bf16", 0.1, 1, pg, yg)
    # fp64 references once (A = 1), scaled per launch
    ref_dy = sr.stem_wgrad_ref(P.xbuf, P.xg, dy, dg, 1, device=DEV)
    ref_dz = sr.stem_wgrad_ref(P.xbuf, P.xg, dz.bf(), yg, 1, device=DEV)

    def bounded(ref, A, dw, db, tag, key):
        rw = lr.check_values(ref[0], A * ref[1], dw, "dw", fails, tag)
        rb = lr.check_values(ref[2], A * ref[3], db, "db", fails, tag)
        w0, b0 = worst.get(key, (0.0, 0.0))
        worst[key] = (max(w0, rw), max(b0, rb))

    for want_G in (1, 5, None):
        elems = WGRAD_GRID * PART if want_G is None else want_G * PART + PART - 1
        G = sr.wgrad_grid(nt, elems, WGRAD_GRID)
        assert G == (min(nt, WGRAD_GRID) if want_G is None else min(nt, want_G))
        A = sr.wgrad_additions(nt, G)
        tag = f"{case} G {G}"

        def run(mode, *a, **kw):
            rc, dw, db, scratch = _wgrad(P, mode, *a, **kw)
            H_.check(rc, f"{tag} mode {mode}")
            scratch.check(_scratch_addressed(scratch, G), f"{tag} mode {mode} scratch", fails)
            return dw, db

        dw, db = run(0, dy, dg, elems)
        bounded(ref_dy, A, dw, db, f"{tag} yolo_wgrad_stem7", ("grad", G))
        dw2, db2 = run(0, dy, dg, elems)
        if not (torch.equal(dw, dw2) and torch.equal(db, db2)):
            fails.append(f"{tag}: two gradient launches differ")
        dw0, db0 = run(0, dz.bf(), yg, elems)
        bounded(ref_dz, A, dw0, db0, f"{tag} yolo_wgrad_stem7 on the pool gradient tile", ("grad", G))
        for name, mode, args in (("pooled", 1, (yfull, yg, elems, dpool, pg)), ("codes", 2, (ypool, pg, elems, dpool, pg, codes_h))):
            dw1, db1 = run(mode, *args)
            bounded(ref_dz, A, dw1, db1, f"{tag} yolo_wgrad_stem7_{name}", (name, G))
            if not (torch.equal(dw1, dw0) and torch.equal(db1, db0)):
                fails.append(f"{tag}: yolo_wgrad_stem7_{name} differs from yolo_wgrad_stem7 on the gradient tile "
                             f"(dw {float((dw1 - dw0).abs().max()):.3g}, db {float((db1 - db0).abs().max()):.3g})")
            dwr, dbr = run(mode, *args)
            if not (torch.equal(dw1, dwr) and torch.equal(db1, dbr)):
                fails.append(f"{tag}: two yolo_wgrad_stem7_{name} launches differ")
        # the device's own forward chain: (pool2 = 3 -> codes entry) == (pool2 = 1 with out_full -> pooled entry)
        dwc, dbc = run(2, f_pool3.bf(), pg, elems, dpool, pg, f_codes.region)
        dwp, dbp = run(1, f_full.bf(), yg, elems, dpool, pg)
        if not (torch.equal(dwc, dwp) and torch.equal(dbc, dbp)):
            fails.append(f"{tag}: forward pool2 = 3 + codes entry differs from forward pool2 = 1 with out_full + pooled entry")
    print(f"\nstem weight gradient {case} ({nt} tiles): worst |err| / bound (dw, db)  " +
          "  ".join(f"{k[0]} G={k[1]} {v[0]:.3f} {v[1]:.3f}" for k, v in worst.items()), flush=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_weight_gradient_exact_integers(case):
    """x and the gradient in {-1, 0, 1} (pool modes: pooled gradient in -2 .. 2, slope 0.5, so the tile holds multiples of 1/2): every product and
    every partial sum is a multiple of 1/2 below 2^23, exact in fp32 in any order.  dw and db then equal the fp64 reference bit for bit for every
    number of workgroups and every entry: a tile skipped, taken twice or paired with another tile's patch cannot hide in a rounding bound"""
    P = Problem(case, seed=7)
    N, Ho, Wo = P.N, P.Ho, P.Wo
    g = _gen(90 + ord(case))
    P.set(torch.randint(-1, 2, (N, 3, P.H, P.W), generator=g).float(), torch.zeros(64, 3, 7, 7), torch.zeros(64))
    yg, pg, dg = sr.Geo(N, Ho, Wo, 64, 1), sr.Geo(N, Ho // 2, Wo // 2, 64, 1), sr.Geo(N, Ho, Wo, 64, 0)
    dy = _zeros(dg)
    dg.interior(dy).copy_(torch.randint(-1, 2, (N, Ho, Wo, 64), generator=g).to(BF))
    vals = torch.tensor([-1.0, -0.25, 0.0, 0.5, 2.0])
    yi = vals[torch.randint(0, 5, (N, Ho, Wo, 64), generator=g)].to(BF)
    dpi = torch.randint(-2, 3, (N, Ho // 2, Wo // 2, 64), generator=g).to(BF)
    dz_h, pooled_h, first_h = sr.pool_lrelu_grad(yi, dpi, 0.5)
    yfull, dpool, ypool, dz = _zeros(yg), _zeros(pg), _zeros(pg), _zeros(dg)
    yg.interior(yfull).copy_(yi)
    pg.interior(dpool).copy_(dpi)
    pg.interior(ypool).copy_(pooled_h)
    dg.interior(dz).copy_(dz_h)
    codes_h = sr.pack_codes(first_h, pg).to(DEV)
    ref_dy = sr.stem_wgrad_ref(P.xbuf, P.xg, dy, dg, 1, device=DEV)
    ref_dz = sr.stem_wgrad_ref(P.xbuf, P.xg, dz, dg, 1, device=DEV)
    assert float(ref_dy[0].abs().max()) < 2 ** 23 and float(ref_dz[0].abs().max()) < 2 ** 23 and float(ref_dz[0].abs().max()) > 0
    fails = []
    for want_G in (1, 5, None):
        elems = WGRAD_GRID * PART if want_G is None else want_G * PART
        for name, ref, mode, args in (("yolo_wgrad_stem7", ref_dy, 0, (dy, dg, elems)), ("yolo_wgrad_stem7 (tile)", ref_dz, 0, (dz, dg, elems)),
                                      ("yolo_wgrad_stem7_pooled", ref_dz, 1, (yfull, yg, elems, dpool, pg)),
                                      ("yolo_wgrad_stem7_codes", ref_dz, 2, (ypool, pg, elems, dpool, pg, codes_h))):
            rc, dw, db, _ = _wgrad(P, mode, *args, slope=0.5)
            _api().check(rc, name)
            if not (torch.equal(dw.double(), ref[0]) and torch.equal(db.double(), ref[2])):
                fails.append(f"{case} {name}, scratch for {want_G or WGRAD_GRID} workgroups: {int((dw.double() != ref[0]).sum())} dw and "
                             f"{int((db.double() != ref[2]).sum())} db elements differ from the exact sums")
    assert not fails, "\n".join(fails)


def test_weight_gradient_refusals_write_nothing():
    """a 30 x 48 output, a scratch smaller than one partial and misaligned strides are refused by every entry: non-zero, and nothing is written"""
    P = Problem("D", seed=5)
    P.N, P.H, P.W = 1, 64, 96
    g = _gen(6)
    P.set(torch.randn(1, 3, 64, 96, generator=g), torch.randn(64, 3, 7, 7, generator=g) * 0.1, torch.zeros(64))
    yg, pg = sr.Geo(1, 32, 48, 64, 1), sr.Geo(1, 16, 24, 64, 1)
    a, dpool, codes = _zeros(yg), _zeros(pg), torch.zeros(pg.numel // 8, dtype=torch.int16, device=DEV)
    a.copy_(torch.randn(yg.numel, generator=g).to(BF))
    dpool.copy_(torch.randn(pg.numel, generator=g).to(BF))
    ok = 4 * PART
    modes = {0: (a, yg), 1: (a, yg, dpool, pg), 2: (dpool, pg, dpool, pg, codes)}
    fails = []
    for mode, args in modes.items():
        first, rest = args[:2], args[2:]
        for what, kw, elems in (("30 x 48 output", dict(Ho=30), ok), ("scratch below one partial", {}, PART - 1),
                                ("misaligned input row stride", dict(x_row=P.xg.row + 4), ok), ("misaligned offset", dict(a_off=first[1].off + 4), ok)):
            rc, dw, db, scratch = _wgrad(P, mode, *first, elems, *rest, **kw)
            if rc == 0:
                fails.append(f"mode {mode}: {what} accepted")
            if not (bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())):
                fails.append(f"mode {mode}: {what}: dw / db written")
            scratch.check(torch.zeros(scratch.n, dtype=torch.bool, device=DEV), f"mode {mode} {what} scratch", fails)
        rc, dw, db, _ = _wgrad(P, mode, *first, ok, *rest)
        if rc != 0 or not bool(torch.isfinite(dw).all()):
            fails.append(f"mode {mode}: the well-formed call failed")
    assert not fails, "\n".join(fails)


# ---- MaxPool2d(3, 2, 1) forward -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(16, 20), (15, 19), (7, 8)])
@pytest.mark.parametrize("C", [64, 24])
@pytest.mark.parametrize("out_halo", [0, 1])
def test_maxpool3s2_forward_is_exact(H, W, C, out_halo):
    """yolo_maxpool3s2_fwd on non-negative inputs with ties == MaxPool2d(3, 2, 1) bit for bit; nothing outside the output interior is written"""
    H_ = _api()
    g = _gen(H * W + C)
    N = 3
    x = torch.relu(torch.randn(N, H, W, C, generator=g)).to(BF)
    x[:, 3:7, 4:8] = 0.5                          # windows of equal values
    x[:, :2, :, : C // 2] = 0.0                   # and windows that hold nothing but zeros
    xg, og = sr.Geo(N, H, W, C, 1), sr.Geo(N, (H + 1) // 2, (W + 1) // 2, C, out_halo)
    xb = _zeros(xg)
    xg.interior(xb).copy_(x)
    out = PB(og.numel)
    pd = H_.PoolDesc(N, H, W, C, 1, out_halo)
    H_.check(H_.lib().yolo_maxpool3s2_fwd(ctypes.byref(pd), _p(xb), out.ptr(), H_.stream()), "maxpool3s2_fwd")
    fails = []
    out.check(og.mask(DEV), "yolo_maxpool3s2_fwd", fails)
    want = lr.maxpool3s2_ref(x.double()).to(BF).to(DEV).view(torch.int16)
    if not torch.equal(og.interior(out.region), want):
        fails.append(f"{int((og.interior(out.region) != want).sum())} of {want.numel()} elements differ from MaxPool2d(3, 2, 1)")
    assert not fails, "\n".join(fails)
