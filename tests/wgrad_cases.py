"""The case matrix of tests/test_gpu_wgrad.py: every form of yolo_wgrad (include/yolo_hip.h) as (shape, mode) pairs, the operands of a shape on any
device, a Python mirror of the library's two-segment schedule, and the table of the forms the header documents as refused.  A plain module: it
imports without a GPU, and tests/test_wgrad_cases_cpu.py checks on the CPU what the GPU test relies on.

Shapes.  A Linear-form shape is two row-major matrices dy [P][dy_px_stride], x [P][x_px_stride] (1x1, pad 0, x_row_stride 0, no halo).  A conv
shape lays both buffers out as engine.Act does: [N][H + 2][W + 2][px_stride] with a zero halo of one pixel, between guard bands of zeros of
(Wp + 2) * px_stride + 512 elements (rounded up to 128) -- more than any |tapoff| -- and is reduced over every slot ("flat"), over the interior pixels
("interior", geo_px_slots = 1) or, as Plan._wgrad_desc builds a stride-2 conv, over every second pixel of a zero-stuffed dy ("stride2":
geo_row_slots = 2 * Wp, geo_px_slots = 2).

Operand sets.
  exact   x uniform in {-3..3}, dy uniform in {-2..2} / 4, previous contents dw0 / db0 in {-8..8} / 4.  Every product is a multiple of 1/4 and every
          partial sum, in any order, a multiple of 1/4 of magnitude <= 1.5 P + 2 < 2^22: exact in fp32 whatever the tree, the split or the order of
          the atomics.  The launch must then equal the fp64 reference bit for bit (bound 0), at any P.
  random  x ~ N(0, 1), dy ~ 0.1 N(0, 1) rounded to bf16, checked against launch_ref.wgrad_bound; P <= 2048 only, where one dropped product
          (about S / P) exceeds the bound (about P u S) by 2^24 / P^2 >= 4.
`poison` shapes hold a large finite value in the columns of dy beyond Cout and of x beyond Cin inside the pixel stride (interior pixels only: the
halo stays zero in every column); nothing stored may depend on them."""

from __future__ import annotations

import math
import zlib
from types import SimpleNamespace

import torch

BF = torch.bfloat16
E_ARG, E_UNSUPPORTED = -1, -2            # YOLO_E_ARG, YOLO_E_UNSUPPORTED
FAMILIES = {"A": (0, 1), "A8": (4,), "B": (2, 3), "C": (5, 6)}
FAMILY_OF = {v: f for f, vs in FAMILIES.items() for v in vs}
POISON = 32768.0
RANDOM_MAX_P = 2048
OPSETS = ("exact", "random")
DESC_FIELDS = ("P", "dy_px_stride", "x_px_stride", "Cout", "Cin", "KH", "KW", "pad", "x_row_stride", "split", "accumulate", "variant", "geo_W", "geo_H",
               "geo_img_slots", "geo_row_slots", "geo_px_slots", "geo_slot0")


def _up(n, m):
    return -(-n // m) * m


# ---- the library's schedule, restated ------------------------------------------------------------------------------------------------------------------

def wgrad_tiles(Cout, Cin, ntaps, variant, x_px_stride=None):
    """(tiles, slots) of a launch: 128 x 128 tiles on 512 workgroup slots (variants 0 / 1 / 4; Cin == 64 pairs the taps), 256 x 128 on 256 (2 / 3),
    256 x 256 on 256 with 256 / Cin taps per tile where Cin < 256 divides 256 into whole 8-channel chunks (5 / 6)"""
    xs = _up(Cin, 8) if x_px_stride is None else x_px_stride
    if variant in (5, 6):
        tt = 256 // Cin if (Cin < 256 and 256 % Cin == 0 and Cin % 8 == 0 and ntaps > 1 and xs >= Cin) else 1
        n_ci = 1 if tt > 1 else -(-Cin // 256)
        return -(-Cout // 256) * n_ci * -(-ntaps // tt), 256
    if variant in (2, 3):
        return -(-Cout // 256) * -(-Cin // 128) * ntaps, 256
    pair = Cin == 64 and ntaps > 1 and xs >= 64
    return -(-Cout // 128) * -(-Cin // 128) * ((ntaps + 1) // 2 if pair else ntaps), 512


def wgrad_schedule(P, tiles, slots):
    """the two-segment schedule of yolo_wgrad (split = 0) -> (main_tiles, main_split, tail_tiles, tail_split): the cost model of wgrad_run in K steps
    of 64 pixels, a round of workgroups costing its steps + 30"""
    steps, E = -(-P // 64), 30.0
    best, bs, bt = 1e30, 1, 1
    sp = 1
    while sp <= slots:
        if sp > 1 and steps // sp < 4:
            break
        tpr = slots // sp
        mt = tiles // tpr * tpr
        tt = tiles - mt
        ts = max(sp, min(slots // tt, max(1, steps // 4))) if tt > 0 else 1
        cost = (mt // tpr) * (-(-steps // sp) + E) + ((-(-steps // ts) + E) if tt > 0 else 0.0)
        if cost < best:
            best, bs, bt = cost, sp, ts
        sp *= 2
    tpr = slots // bs
    main_tiles = tiles // tpr * tpr
    tail_tiles = tiles - main_tiles
    return main_tiles, bs, tail_tiles, (bt if tail_tiles > 0 else 1)


def _filled(P, split):
    """ranges of a `split`-way pixel split that hold pixels: a range is whole 64-pixel steps"""
    per = _up(-(-P // split), 64)
    return -(-P // per)


def ranges_of(d):
    """(main, tail): pixel ranges WITH pixels per tile of the launch d describes (tail = 0: no tail tiles); a uniform split has one segment"""
    ntaps = d.KH * d.KW
    if d.split > 0:
        return _filled(d.P, d.split), 0
    tiles, slots = wgrad_tiles(d.Cout, d.Cin, ntaps, d.variant, d.x_px_stride)
    mt, ms, tt, ts = wgrad_schedule(d.P, tiles, slots)
    return (_filled(d.P, ms) if mt else 0), (_filled(d.P, ts) if tt else 0)


def max_ranges(d):
    return max(1, *ranges_of(d))


# ---- shapes and operands ---------------------------------------------------------------------------------------------------------------------------------

class Shape:
    def __init__(self, Cout, Cin, K=1, P=None, nhw=None, geo="flat", dy_stride=None, x_stride=None, poison=False):
        self.Cout, self.Cin, self.K, self.nhw, self.geo, self.poison = Cout, Cin, K, nhw, geo, poison
        self.dy_stride = dy_stride or _up(Cout, 8)
        self.x_stride = x_stride or _up(Cin, 8)
        if nhw is None:
            assert K == 1 and geo == "flat"
            self.P = P
            self.name = f"lin-P{P}"
        else:
            N, H, W = nhw
            self.Hp, self.Wp = H + 2, W + 2
            self.Ho, self.Wo = (-(-H // 2), -(-W // 2)) if geo == "stride2" else (H, W)
            self.P = N * self.Hp * self.Wp if geo == "flat" else N * self.Ho * self.Wo
            self.name = f"{geo}-{N}x{H}x{W}-k{K}"
        self.name += f"-{Cout}x{Cin}"
        if self.dy_stride != _up(Cout, 8) or self.x_stride != _up(Cin, 8):
            self.name += f"-ld{self.dy_stride}x{self.x_stride}"
        if poison:
            self.name += "-poison"

    def args(self):
        """descriptor fields that do not depend on the mode"""
        a = dict(P=self.P, dy_px_stride=self.dy_stride, x_px_stride=self.x_stride, Cout=self.Cout, Cin=self.Cin, KH=self.K, KW=self.K, pad=self.K // 2,
                 x_row_stride=0, geo_W=0, geo_H=0, geo_img_slots=0, geo_row_slots=0, geo_px_slots=0, geo_slot0=0)
        if self.nhw is not None:
            a["x_row_stride"] = self.Wp * self.x_stride
            if self.geo != "flat":
                s = 2 if self.geo == "stride2" else 1
                a.update(geo_W=self.Wo, geo_H=self.Ho, geo_img_slots=self.Hp * self.Wp, geo_row_slots=s * self.Wp, geo_px_slots=s, geo_slot0=self.Wp + 1)
        return a

    def n_dw(self):
        return self.Cout * self.K * self.K * self.Cin


def _values(opset, gen, shape, what):
    if opset == "exact":
        lo, hi, div = (-3, 4, 1.0) if what == "x" else (-2, 3, 4.0)
        return torch.randint(lo, hi, shape, generator=gen).float() / div
    return torch.randn(shape, generator=gen) * (1.0 if what == "x" else 0.1)


def _seed(shape, opset):
    return zlib.crc32(f"{shape.name}/{opset}".encode())


def operands(shape: Shape, opset: str, device="cpu"):
    """-> namespace: x, dy (flat bf16 stores with their guard bands), x_base, dy_base (element offset of the pointer a launch receives), dw0 [n_dw],
    db0 [Cout] fp32 (the previous contents where a launch adds: multiples of 1/4)"""
    gen = torch.Generator().manual_seed(_seed(shape, opset))
    o = SimpleNamespace()
    for what, C, ld in (("x", shape.Cin, shape.x_stride), ("dy", shape.Cout, shape.dy_stride)):
        if shape.nhw is None:
            m = torch.zeros(shape.P, ld)
            m[:, :C] = _values(opset, gen, (shape.P, C), what)
            if shape.poison:
                m[:, C:] = POISON
            store, base = m.reshape(-1), 0
        else:
            N, H, W = shape.nhw
            guard = _up((shape.Wp + 2) * ld + 512, 128)
            store = torch.zeros(2 * guard + N * shape.Hp * shape.Wp * ld)
            inner = store[guard: guard + N * shape.Hp * shape.Wp * ld].view(N, shape.Hp, shape.Wp, ld)[:, 1: 1 + H, 1: 1 + W]
            v = torch.zeros(N, H, W, ld)
            v[..., :C] = _values(opset, gen, (N, H, W, C), what)
            if shape.poison:
                v[..., C:] = POISON
            if what == "dy" and shape.geo == "stride2":         # zero-stuffed gradient: values on the even pixels of the input's geometry, all columns
                keep = torch.zeros(1, H, W, 1)
                keep[:, ::2, ::2] = 1
                v = v * keep
            inner.copy_(v)
            base = guard
        setattr(o, what, store.to(BF).to(device))
        setattr(o, what + "_base", base)
    o.dw0 = (torch.randint(-8, 9, (shape.n_dw(),), generator=gen).float() / 4).to(device)
    o.db0 = (torch.randint(-8, 9, (shape.Cout,), generator=gen).float() / 4).to(device)
    return o


# ---- modes and cases ---------------------------------------------------------------------------------------------------------------------------------------

class Mode:
    def __init__(self, variant, split=1, accumulate=0, db=True, slabs=False, sumsq=False):
        self.variant, self.split, self.accumulate, self.db, self.slabs, self.sumsq = variant, split, accumulate, db, slabs, sumsq
        self.name = f"v{variant}-s{split}" + ("-acc" if accumulate else "") + ("" if db else "-nodb") + ("-slabs" if slabs else "") + ("-sumsq" if sumsq else "")


class Case:
    def __init__(self, group, shape, mode, opsets=OPSETS):
        self.group, self.shape, self.mode = group, shape, mode
        self.family = FAMILY_OF[mode.variant]
        self.opsets = tuple(o for o in opsets if o == "exact" or shape.P <= RANDOM_MAX_P)
        self.id = f"{shape.name}/{mode.name}"

    def desc(self, cls=SimpleNamespace):
        """the descriptor (a namespace, or yolo._hip.WgradDesc) without the pointers"""
        d = cls()
        vals = dict(self.shape.args(), split=self.mode.split, accumulate=self.mode.accumulate, variant=self.mode.variant)
        for k in DESC_FIELDS:
            setattr(d, k, vals[k])
        return d


def documented_refusal(case):
    """the rule of include/yolo_hip.h that refuses this form, or None.  In the order wgrad_run applies them."""
    s, m = case.shape, case.mode
    d = case.desc()
    pipe, big = m.variant in (5, 6), m.variant in (2, 3)
    if s.geo != "flat" and big:
        return "geometry with variants 2 and 3"
    if pipe and s.geo == "flat" and s.K == 1 and s.P % 32:
        return "variants 5 and 6, pad 0: P % 32 == 0"
    split_tiles = max_ranges(d) > 1
    if m.slabs:
        if big or m.accumulate or s.Cin % 4:
            return "slabs: variant 0 / 1 / 4 / 5 / 6, accumulate = 0, Cin % 4 == 0"
        if pipe and m.db and max_ranges(d) > s.K * s.K * s.Cin:
            return "slabs with db: KH * KW * Cin must hold the ranges"
    if m.sumsq:
        if pipe or big or m.variant == 4 or split_tiles or m.accumulate or s.Cin % 4:
            return "dw_sumsq: split 1, accumulate 0, variant 0 / 1, Cin % 4 == 0"
    return None


def dw_arrives(case):
    """what dw holds before the launch: "nan" where every tile is stored, "dw0" where the launch adds onto the previous contents, "zero" where a split
    tile is added with atomics (the caller zero-fills, as the header asks)"""
    m, d = case.mode, case.desc()
    if m.accumulate:
        return "dw0"
    if m.slabs or max_ranges(d) == 1:
        return "nan"
    return "zero"


def db_arrives(case):
    """db is always added to (-> "db0") except in slab mode with a split tile (every tile of variants 5 / 6), where it is stored (-> "nan")"""
    m, d = case.mode, case.desc()
    if m.slabs and (m.variant in (5, 6) or max_ranges(d) > 1):
        return "nan"
    return "db0"


def repeatable(case):
    """forms without atomics on dw: a second launch must give the same bits"""
    m = case.mode
    return bool(m.slabs) or (not m.accumulate and max_ranges(case.desc()) == 1)


LIN_P_64 = (1, 5, 63, 64, 65, 127, 128, 129, 191, 257)          # one .. four 64-pixel steps, both buffers of the double-buffered loop
LIN_P_32 = (32, 64, 96, 128, 160, 288)                          # the ring of four 32-pixel stages of variants 5 / 6
GEOMETRIES = ((1, 2, 2), (2, 7, 7), (3, 5, 9), (1, 14, 14))
STRIDE2 = ((2, 14, 14), (1, 9, 11))                             # -> 7 x 7, and an odd input -> 5 x 6
CHANNELS = ((128, 128, None, None), (136, 72, None, None), (30, 40, None, None), (264, 320, None, None), (150, 200, 160, None))
SCHED_128 = dict(P=6400, Cout=2176, Cin=2048)                   # 272 tiles: main 256 x 2, tail 16 x 25
SCHED_256 = dict(P=6400, Cout=4352, Cin=2048)                   # 136 tiles: main 128 x 2, tail 8 x 25
EMPTY_P = 1568                                                  # 25 steps: a six-way tail split rounds up to ranges of 320 pixels, five hold pixels


def _lin_p(fam, P):
    """the pixel count a Linear-form case uses in family fam: variants 5 / 6 need P % 32 == 0 there"""
    return _up(P, 32) if fam == "C" else P


def build_matrix():
    cases = []

    def add(group, shape, variants, **mode):
        for v in variants:
            c = Case(group, shape, Mode(v, **mode))
            if all(c.id != o.id for o in cases):         # (a form two groups ask for runs once, in the first)
                cases.append(c)

    for fam, variants in FAMILIES.items():
        # K-step edges, Linear form
        for P in (LIN_P_32 if fam == "C" else LIN_P_64):
            add("ksteps", Shape(136, 72, P=P), variants)
            add("ksteps", Shape(136, 72, P=P), variants, split=0, db=False)
        # geometries: flat over every slot and interior, 3x3 pad 1 and 1x1 pad 0; stride 2 as the executor builds it
        for nhw in GEOMETRIES:
            for K in (3, 1):
                for geo in ("flat", "interior"):
                    add("geometry", Shape(136, 72, K, nhw=nhw, geo=geo), variants, split=0)
        for nhw in STRIDE2:
            for K in (3, 1):
                add("geometry", Shape(136, 72, K, nhw=nhw, geo="stride2"), variants, split=0)
        # channel edges: a conv over every slot (all families), over the interior, and the Linear form
        for Cout, Cin, dyl, xl in CHANNELS:
            add("channels", Shape(Cout, Cin, 3, nhw=(3, 5, 9), geo="flat", dy_stride=dyl, x_stride=xl), variants)
            if fam != "B":
                add("channels", Shape(Cout, Cin, 3, nhw=(3, 5, 9), geo="interior", dy_stride=dyl, x_stride=xl), variants, split=0)
            add("channels", Shape(Cout, Cin, P=_lin_p(fam, 129), dy_stride=dyl, x_stride=xl), variants)
        add("channels", Shape(136, 64, 3, nhw=(2, 7, 7), geo="flat"), variants)                  # pair_taps: nine taps, the last pair has one
        add("channels", Shape(136, 64, 1, nhw=(2, 7, 7), geo="flat" if fam == "B" else "interior"), variants)     # 1x1: no pairing
        for Cin, xl in ((1, 8), (3, 8), (5, 8), (13, 16)):                                       # the data gradient of the Linear behind nn.Flatten
            add("channels", Shape(136, Cin, P=_lin_p(fam, 257), x_stride=xl), variants, split=0, accumulate=1, db=False)
        add("channels", Shape(64, 224, P=_lin_p(fam, 257)), variants, split=2)                   # the im2col stem form
        add("channels", Shape(150, 200, 3, nhw=(2, 7, 7), geo="flat", dy_stride=160, x_stride=208, poison=True), variants)
        add("channels", Shape(150, 200, P=_lin_p(fam, 129), dy_stride=160, x_stride=208, poison=True), variants, split=2)
        # modes
        mode_shapes = [Shape(136, 72, P=_lin_p(fam, 257)), Shape(136, 72, 3, nhw=(3, 5, 9), geo="flat")]
        if fam != "B":
            mode_shapes.append(Shape(30, 40, 3, nhw=(2, 14, 14), geo="stride2"))
        for shape in mode_shapes:
            for split in (1, 2, 3, 0):
                for acc in (0, 1):
                    for db in (True, False):
                        add("modes", shape, variants, split=split, accumulate=acc, db=db)
                for db in (True, False):
                    add("modes", shape, variants, split=split, db=db, slabs=True)
            add("modes", shape, variants, split=3, accumulate=1, slabs=True)                      # refused: slabs do not accumulate
        # schedules: a split = 0 launch whose rounded-up tail split leaves ranges without pixels
        for mode in (dict(), dict(slabs=True), dict(accumulate=1)):
            add("schedule", Shape(264, 320, P=EMPTY_P), variants, split=0, **mode)
    # variants 5 / 6, 3x3: 256 / Cin taps per tile (32, 16, 8, 4, 2), then one tap per tile; 4: fewer than one 8-channel chunk, so no grouping
    for Cin in (4, 8, 16, 32, 64, 128, 192, 256):
        for geo in ("flat", "interior"):
            add("taps", Shape(136, Cin, 3, nhw=(3, 5, 9), geo=geo), FAMILIES["C"], split=0)
        add("taps", Shape(136, Cin, 3, nhw=(3, 5, 9), geo="interior"), FAMILIES["C"], split=2, slabs=True)
    add("ksteps", Shape(136, 72, P=33), FAMILIES["C"])                                           # refused
    # the Linear layers: P = batch, Cout 1470 (not a multiple of 8, so Cout_ld clamps inside the stride), fused sum of squares
    for P in (1, 5, 13):
        add("sumsq", Shape(1470, 256, P=P), (0,), sumsq=True)
    add("sumsq", Shape(136, 72, P=257), (0, 1), sumsq=True)
    add("sumsq", Shape(136, 72, 3, nhw=(2, 7, 7), geo="interior"), (0, 1), sumsq=True)
    add("sumsq", Shape(136, 64, 3, nhw=(2, 7, 7), geo="interior"), (0, 1), sumsq=True)           # with paired taps
    # ... and what the header refuses for it
    add("sumsq", Shape(136, 72, P=288), (2, 3, 4, 5, 6), sumsq=True)
    add("sumsq", Shape(136, 72, P=257), (0, 1), split=2, sumsq=True)
    add("sumsq", Shape(136, 72, P=257), (0, 1), accumulate=1, sumsq=True)
    add("sumsq", Shape(136, 13, P=257, x_stride=16), (0, 1), sumsq=True)
    # both segments of the two-segment schedule split (exact operands only: P > 2048)
    for fam, shp in (("A", SCHED_128), ("A8", SCHED_128), ("C", SCHED_256)):
        for mode in (dict(), dict(slabs=True), dict(accumulate=1)):
            add("both-segments", Shape(shp["Cout"], shp["Cin"], P=shp["P"]), FAMILIES[fam], split=0, **mode)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:5]
    return cases


MATRIX = build_matrix()

# The forms of the matrix that include/yolo_hip.h documents as unsupported: case id -> (return code, rule).  Every other case must run and be checked.
EXPECT_REFUSED = {c.id: (E_UNSUPPORTED, why) for c in MATRIX for why in [documented_refusal(c)] if why}

BIAS_ONLY = [(P, Cout) for P in (1, 31, 1000, 2048) for Cout in (8, 30, 1470, 2056)]
