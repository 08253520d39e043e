"""Constructed batches for the two 10-10-10 methods ("loop_las_cuda", "loop_las_hqs"): inputs and the facts each case relies on.

Every case is built by hand from batch records and the four point arrays, as pcr_las_upload takes them. All cases share one
transform, rows (1,0,0,tx), (0,1,0,0), (0,0,0,0) and w row (0,0,1,0): a point's clip position is (x + tx, y, w = z), its pixel
((x/w + 1) W/2, (y/w + 1) H/2). The level of detail reads world_view (identity) and proj (row 0 = (s,0,0,0), w row given per case)
only, so a batch's level follows from its box diagonal and is independent of where its points land.

CASES maps a name to a builder; build(name) returns
    (batches, xyz12, xyz8, xyz4, rgba, params, W, H, facts)
`facts` holds what the case claims about itself (tests/test_las_cases_cpu.py proves each claim against the references):
    levels   the level of every batch under `params` (-1 culled)
    frames   [(name, params), ...] the frames to draw, in this order, on one context (default: the one `params`)
    pixels   {frame name: sorted framebuffer word indices that are set}, where the case states them from integer arithmetic
    ...      family-specific entries, described at the builders
"""
from __future__ import annotations

import functools

import numpy as np

from pcrhpg24_amd._native import RenderParams, XyzBatch, fb_elems
from tests import oracle

PPB = 65536
F32 = np.float32
WIN_PIXELS = 4096            # capacity of the basic passes' window
WIN_PIXELS_HQS = 4095        # capacity of the colour pass's window


def point_colours(n: int) -> np.ndarray:
    """A hash of the point index: all four bytes vary."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return h.astype(np.uint32)


def make_params(W: int, H: int, s: float, tx: float = 0.0, cull: int = 0, proj_w=(0.0, 0.0, 0.0, 1.0), wv_x: float = 1.0) -> RenderParams:
    p = RenderParams()
    t = [1, 0, 0, tx, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    wv = [wv_x, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    pr = [s, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, *proj_w]
    for k in range(16):
        p.transform[k], p.world_view[k], p.proj[k] = t[k], wv[k], pr[k]
    p.width, p.height = W, H
    p.points_per_thread, p.lod_percent = 64, 100
    p.enable_frustum_culling = cull
    return p


def make_batch(lo, hi) -> XyzBatch:
    b = XyzBatch()
    b.min_x, b.min_y, b.min_z = (float(v) for v in lo)
    b.max_x, b.max_y, b.max_z = (float(v) for v in hi)
    b.num_points = PPB
    for name, v in zip(("min_x", "min_y", "min_z", "max_x", "max_y", "max_z"), (*lo, *hi)):
        assert float(getattr(b, name)) == float(v), f"{name} = {v} is no float32"
    return b


class Scene:
    """Collects batches. A batch's points are given as 30-bit coordinates X, Y, Z (arrays of any length up to 65 536, repeated
    in turn to fill the batch) and the level the case expects it to be drawn at. The arrays that level does not read get
    all-ones fields; bits 30-31 of all three arrays are set from the point index."""

    def __init__(self, W: int, H: int):
        self.W, self.H = W, H
        self.boxes, self.levels, self.words = [], [], []

    def add(self, lo, hi, level: int, X, Y, Z, exact: bool = True) -> int:
        X, Y, Z = (np.resize(np.asarray(a, np.int64), PPB) for a in (X, Y, Z))
        for a in (X, Y, Z):
            assert a.min() >= 0 and a.max() < (1 << 30)
            if level >= 2:
                assert not (a & 0xFFFFF).any(), "a 4-byte level reads the top ten bits only"
            elif level == 1:
                assert not (a & 0x3FF).any(), "the 8-byte level reads the top twenty bits only"
        if exact:                                   # the position is a float32 the dequantisation reaches without rounding
            div = 1024.0 if level >= 2 else 1073741824.0
            for a, l, h in zip((X, Y, Z), lo, hi):
                q = (a >> 20) if level >= 2 else a
                sc = float(F32(F32(F32(h) - F32(l)) / F32(div)))
                pos = q.astype(np.float64) * sc + float(l)
                assert (q.astype(F32).astype(np.int64) == q).all() and (pos.astype(F32).astype(np.float64) == pos).all()
        ones = np.full(PPB, 0x3FFFFFFF, np.uint32)

        def field(shift):
            return (((X >> shift) & 1023) | (((Y >> shift) & 1023) << 10) | (((Z >> shift) & 1023) << 20)).astype(np.uint32)
        w4, w8, w12 = field(20), field(10), field(0)
        if level >= 2 or level < 0:
            w8, w12 = ones, ones
        elif level == 1:
            w12 = ones
        self.boxes.append((tuple(lo), tuple(hi)))
        self.levels.append(level)
        self.words.append((w12, w8, w4))
        return len(self.boxes) - 1

    def add_last(self):
        """The file's last batch is never drawn (render.cu:201-202): a small box in view, its points on pixel (0, 0)."""
        return self.add((-2, -2, 1), (-1, -1, 2), 4, [0], [0], [0], exact=False)

    def finish(self, params: RenderParams, facts: dict):
        nb = len(self.boxes)
        batches = (XyzBatch * nb)()
        for i, (lo, hi) in enumerate(self.boxes):
            batches[i] = make_batch(lo, hi)
        idx = np.arange(nb * PPB, dtype=np.uint32)
        x12, x8, x4 = (np.ascontiguousarray(np.concatenate([w[k] for w in self.words])) for k in range(3))
        x4 |= (idx & np.uint32(3)) << np.uint32(30)
        x8 |= ((idx >> np.uint32(2)) & np.uint32(3)) << np.uint32(30)
        x12 |= ((idx >> np.uint32(4)) & np.uint32(3)) << np.uint32(30)
        facts = dict(facts)
        facts.setdefault("levels", list(self.levels))
        facts.setdefault("frames", [("frame", params)])
        return batches, x12, x8, x4, point_colours(nb * PPB), params, self.W, self.H, facts


# ---- the rectangle rule, restated in float32 for classifying batches (never for an expected frame) --------------------------
def _fma(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _dot4(r, x, y, z):
    return _fma(r[3], F32(1), _fma(r[2], z, _fma(r[1], y, F32(r[0]) * F32(x))))


def window_rect(p: RenderParams, lo, hi, capacity: int):
    """(x0, y0, ww, wh, partial) of a batch box: the window the prepass plans (ww == 0: none) and whether the batch counts as
    heavy (its rectangle does not fit the capacity)."""
    T = [[F32(p.transform[4 * r + c]) for c in range(4)] for r in range(4)]
    fw, fh = F32(p.width), F32(p.height)
    sxs, sys_ = [], []
    for c in range(8):
        x, y, z = (F32(hi[k]) if c >> k & 1 else F32(lo[k]) for k in range(3))
        w = _dot4(T[3], x, y, z)
        if not w > F32(1.0e-6):
            return 0, 0, 0, 0, True
        sxs.append(F32(F32(F32(_dot4(T[0], x, y, z) / w) * F32(0.5) + F32(0.5)) * fw))
        sys_.append(F32(F32(F32(_dot4(T[1], x, y, z) / w) * F32(0.5) + F32(0.5)) * fh))
    minx, maxx, miny, maxy = min(sxs), max(sxs), min(sys_), max(sys_)
    if not (maxx >= -1 and maxy >= -1 and minx <= fw + F32(1) and miny <= fh + F32(1)):
        return 0, 0, 0, 0, True
    x0 = max(0, int(np.floor(max(minx, F32(-2)))) - 1)
    x1 = min(p.width - 1, int(np.floor(min(maxx, fw + F32(2)))) + 1)
    y0 = max(0, int(np.floor(max(miny, F32(-2)))) - 1)
    y1 = min(p.height - 1, int(np.floor(min(maxy, fh + F32(2)))) + 1)
    ww, wh = x1 - x0 + 1, y1 - y0 + 1
    partial = not (ww > 0 and wh > 0 and ww * wh <= capacity)
    if ww > 0 and wh > 0 and capacity < ww * wh <= 16 * capacity:
        sc = F32(np.sqrt(F32(F32(capacity) / F32(F32(ww) * F32(wh)))))
        nw, nh = max(1, int(np.floor(F32(F32(ww) * sc)))), max(1, int(np.floor(F32(F32(wh) * sc))))
        x0 += (ww - nw) // 2
        y0 += (wh - nh) // 2
        ww, wh = nw, nh
    if ww > 0 and wh > 0 and ww * wh <= capacity:
        return x0, y0, ww, wh, partial
    return 0, 0, 0, 0, partial


# ---- shared geometry ---------------------------------------------------------------------------------------------------------
UNIT_LO = -(1 << 23)


def unit_box(zmin: int):
    """A 30-bit box with one world unit per step: x, y = X - 2^23 (X < 2^24 converts to float32 exactly), w = Z + zmin.
    zmin == 0: a corner has w == 0, the batch gets no window; zmin == 1: its rectangle is the whole image."""
    return (UNIT_LO, UNIT_LO, zmin), ((1 << 30) + UNIT_LO, (1 << 30) + UNIT_LO, 1 << 30)


def unit_xyz(x, y, w, zmin: int):
    return np.asarray(x, np.int64) - UNIT_LO, np.asarray(y, np.int64) - UNIT_LO, np.asarray(w, np.int64) - zmin


def mid_pixel(col, row, w, W: int, H: int):
    """Integer (x, y) nearest the middle of pixel (col, row) at depth w (a pixel is 2w/W x 2w/H units)."""
    col, row, w = (np.asarray(a, np.float64) for a in (col, row, w))
    return np.rint((col - W / 2 + 0.5) * 2 * w / W).astype(np.int64), np.rint((row - H / 2 + 0.5) * 2 * w / H).astype(np.int64)


# ---- A: level cuts -------------------------------------------------------------------------------------------------------------
def _adjacent_floats_across(pred, lo: float, hi: float):
    """The two adjacent float32 a < b in [lo, hi] with not pred(a) and pred(b): bisection on the bit pattern (positive floats
    order as their bits do)."""
    a, b = int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))
    assert not pred(float(np.uint32(a).view(F32))) and pred(float(np.uint32(b).view(F32)))
    while b - a > 1:
        m = (a + b) // 2
        if pred(float(np.uint32(m).view(F32))):
            b = m
        else:
            a = m
    return float(np.uint32(a).view(F32)), float(np.uint32(b).view(F32))


def case_level_cuts():
    """256 x 128. Batch b draws on row 8 + 8 b, all of it at depth 128 (flat box; the pc.w == 0 batch at 256), so one x unit is
    one pixel. Boxes are 2^20 (cut 500) or 2^30 (cut 10000) units wide: the column of a point sits in the xyz8 resp. xyz12
    field, so a batch read one level too coarse collapses onto column 0 and one read too fine leaves the screen (the fields it
    must not read are all ones). The level is steered with max_y alone; every point has Y == 0.
    world_view's x row is zero, so the box centre projects to x == 0 and px = 128 (q + 1) - 128 with q = 2 s rad: s is a power of
    two and q + 1 is no finer than q, so as max_y grows float by float px passes through every value of its grid and the first
    batch at or above a cut has px == cut exactly -- the value on which `<` and `<=` differ (level_px restates it for the CPU test).
    facts: cuts = [(batch below, batch above, cut, (max_y pair of the one), (of the other))], each pair adjacent float32."""
    W, H = 256, 128
    s = 2.0 ** -25                                    # px = 256 s rad: a 2^30-wide flat box at depth 128 projects to 8192 pixels
    p = make_params(W, H, s, proj_w=(0.0, 0.0, -1.0 / 256.0, 1.0), wv_x=0.0)   # pc.w = 1 - cz / 256: 0.5 at depth 128, 0 at 256
    sc = Scene(W, H)
    rows = {}

    def box(b, width, dy):
        oy = (8 + 8 * b - 64) * 2
        return (-128, oy, 128), (width - 128, F32(F32(oy) + F32(dy)), 128)

    def level_of(b, width, max_y):
        lo, hi = box(b, width, 0)
        return oracle.las_level(make_batch(lo, (hi[0], max_y, hi[2])), p)

    cols = np.arange(256)
    cuts, b = [], 0
    for cut, width, below in ((500, 1 << 20, 2), (10000, 1 << 30, 1)):
        pairs = []
        for k in range(2):                            # the batch just below the cut, then the one just above (each on its own row)
            bb = b + k
            pair = _adjacent_floats_across(lambda my: level_of(bb, width, my) < below, 1000.0, 2.0 ** 31)
            level = below - k
            # the column sits in the finest field the finer level reads: the coarser level sees column 0
            X = cols * 0 if k == 0 else cols << 10 if cut == 500 else cols
            lo, hi = box(bb, width, 0)
            sc.add(lo, (hi[0], pair[k], hi[2]), level, X, [0], [0])
            rows[bb] = cols if k else cols[:1]
            pairs.append(pair)
        cuts.append((b, b + 1, cut, pairs[0], pairs[1]))
        b += 2
    # pc.w == 0: flat at depth 256, two units per pixel, box 2^31 wide -> x = 2 X - 256, level 0
    oy = (8 + 8 * b - 64) * 4
    sc.add((-256, oy, 256), ((1 << 31) - 256, oy + 64, 256), 0, cols, [0], [0])
    rows[b] = cols
    b += 1
    for level, diag in ((2, 300 * 2.0 ** 17), (3, 150 * 2.0 ** 17), (4, 0.0)):
        lo, hi = box(b, 1 << 20, diag)
        sc.add(lo, hi, level, [0], [0], [0])
        rows[b] = cols[:1]
        b += 1
    sc.add_last()
    pixels = sorted(int(c) + (8 + 8 * k) * W for k, cs in rows.items() for c in cs)
    return sc.finish(p, {"cuts": cuts, "pixels": {"frame": pixels}})


def level_px(g: XyzBatch, p: RenderParams) -> float:
    """The level rule's px of a flat box at depth 128 under case_level_cuts' params (centre at x == 0, pc.w == pe.w == 0.5),
    restated in float32. For showing that a batch sits exactly on its cut, never for an expected frame."""
    dx, dy, dz = F32(g.min_x) - F32(g.max_x), F32(g.min_y) - F32(g.max_y), F32(g.min_z) - F32(g.max_z)
    rad = F32(np.sqrt(_fma(dz, dz, _fma(dy, dy, dx * dx))))
    q = F32(F32(F32(p.proj[0]) * rad) / F32(0.5))
    sex = F32(p.width) * F32(F32(0.5) * F32(q + F32(1)))
    ddx = sex - F32(128)
    return float(F32(np.sqrt(F32(ddx * ddx))))


# ---- B: fields and masks -------------------------------------------------------------------------------------------------------
def case_fields():
    """256 x 128. The box (-128,-128,128)..(128,128,256) scaled by 2^8, 2^3, 2^2, 2^1, 2^0: the same picture at levels 0..4.
    Points: every combination of {0, 1023, a hash} over the nine 10-bit fields (three arrays x three axes), 3^9 patterns;
    X = 0x3FFFFFFF among them. The unread arrays are all ones, bits 30-31 follow the point index (Scene).
    No `pixels` fact: all-ones low fields put points within 2^-16 of a pixel's edge, where the float32 roundings of the conversion,
    the dequantisation and the division decide the pixel, so the set words cannot be stated from integers without restating the
    reference. The case claims what its CPU test proves instead: the fields are there and the masked, unread bits change nothing."""
    W, H = 256, 128
    p = make_params(W, H, 75.0 / 49152.0)            # px = 75 * 2^j for the box scaled by 2^j
    sc = Scene(W, H)
    k = np.arange(3 ** 9)
    h = point_colours(3 ** 9 * 9).reshape(9, -1).astype(np.int64) & 1023
    coords = []
    for axis in range(3):
        v = np.zeros(len(k), np.int64)
        for arr in range(3):                          # arr 0: the xyz4 field (top ten bits)
            d = (k // 3 ** (axis * 3 + arr)) % 3
            f = np.where(d == 0, 0, np.where(d == 1, 1023, h[axis * 3 + arr]))
            v |= f << (20 - 10 * arr)
        coords.append(v)
    for level, j in ((0, 8), (1, 3), (2, 2), (3, 1), (4, 0)):
        m = (1 << 30) - 1 if level == 0 else (1 << 30) - 1024 if level == 1 else (1 << 30) - (1 << 20)
        sc.add((-128 << j, -128 << j, 128 << j), (128 << j, 128 << j, 256 << j), level, *(c & m for c in coords), exact=False)
    sc.add_last()
    return sc.finish(p, {})


# ---- C: frustum border ---------------------------------------------------------------------------------------------------------
def _border_points(wmax=256):
    pts = []
    for w in (64, 128, wmax):
        for t in range(-w + 1, w, max(1, w // 16)):
            pts += [(w, t, w), (w + 1, t, w), (-w, t, w), (-w - 1, t, w), (t, w, w), (t, w + 1, w), (t, -w, w), (t, -w - 1, w)]
        pts += [(sx * w, sy * w, w) for sx in (-1, 1) for sy in (-1, 1)]
        pts += [(w + 1, w, w), (w, w + 1, w), (-w - 1, -w, w), (-w, -w - 1, w), (w + 1, w + 1, w)]
    return np.asarray(pts, np.int64)


def case_border():
    """256 x 128, all batches at level 4 (integer positions from ten bits). Five small flat boxes at depth 128 straddle the right,
    top, top-right, left and bottom planes (whole windows): X or Y == 512 is exactly on the plane, one step further is outside.
    Two boxes (-512,-512,zmin)..(512,512,zmin+1024), zmin 1 (window cut from the whole image) and 0 (no window: a corner has
    w == 0), hold x == +-w, y == +-w, the corners and their outside neighbours at depths 64, 128, 256.
    facts: border_words = the words of column W / row H / the last word that must be set."""
    W, H = 256, 128
    p = make_params(W, H, 2.0 ** -20)
    sc = Scene(W, H)
    words = set()
    k = np.arange(4096)
    a, t = 510 + k % 4, (k // 4) % 1024

    def small(lo, hi, X, Y):
        sc.add(lo, hi, 4, X << 20, Y << 20, [0])
        x = lo[0] + X * (hi[0] - lo[0]) / 1024.0
        y = lo[1] + Y * (hi[1] - lo[1]) / 1024.0
        inside = (abs(x) <= 128) & (abs(y) <= 128)
        words.update((((x[inside] + 128) * W / 256) // 1 + ((y[inside] + 128) * H / 256) // 1 * W).astype(np.int64).tolist())
    small((64, -32, 128), (192, 32, 128), a, t)                       # right: x == w at X == 512
    small((-32, 64, 128), (32, 192, 128), t, a)                       # top
    small((64, 64, 128), (192, 192, 128), 511 + k % 3, 511 + (k // 3) % 3)   # corner: the last word at (512, 512)
    small((-192, -32, 128), (-64, 32, 128), a, t)                     # left: x == -w at X == 512, X == 511 is outside
    small((-32, -192, 128), (32, -64, 128), t, a)                     # bottom
    pts = _border_points()
    x, y, w = pts.T
    for zmin in (1, 0):
        sc.add((-512, -512, zmin), (512, 512, zmin + 1024), 4, (x + 512) << 20, (y + 512) << 20, (w - zmin) << 20)
    inside = (abs(x) <= w) & (abs(y) <= w)
    words.update((((x + w) * W) // (2 * w) + ((y + w) * H) // (2 * w) * W)[inside].tolist())
    sc.add_last()
    must = [W * (H + 1), H * W + 100, W + 64 * W, 0]                   # the last word, a word of row H, column W of row 64, word 0
    return sc.finish(p, {"pixels": {"frame": sorted(words)}, "border_words": must})


TIE_ORDERS = ("ss", "gs", "sg", "sgn", "fg")


# ---- D: ties -------------------------------------------------------------------------------------------------------------------
def _ties(order):
    """512 x 256, pixel (300, 140), depth 256: x = 44, y = 24. 's': a small flat box (whole window, level 4); 'g': the unit box
    with zmin 1, whose rectangle is the whole image, over 16 x the capacity: no window (level 0); 'n': as 'g', one depth step
    nearer; 'f': as 'g', but only its last point is at depth 256. facts: tie = (pixel, winner index, tied points)."""
    W, H = 512, 256
    p = make_params(W, H, 2.0 ** -20)
    sc = Scene(W, H)
    for kind in order:
        lo, hi = unit_box(1)
        if kind == "s":
            sc.add((12, -8, 256), (76, 56, 256), 4, [512 << 20], [512 << 20], [0])
        elif kind == "f":
            # every point behind, at depth 300, but the batch's last one: by the time its thread reaches it the other batch has
            # written the same depth to the pixel, and the pre-read of the global word meets an equal depth with a higher index
            fx, fy = mid_pixel(300, 140, 300, W, H)
            w = np.full(PPB, 300); w[-1] = 256
            sc.add(lo, hi, 0, *unit_xyz(np.where(w == 256, 44, fx), np.where(w == 256, 24, fy), w, 1))
        else:
            sc.add(lo, hi, 0, *unit_xyz([44], [24], [256 if kind == "g" else 255], 1))
    sc.add_last()
    winner = order.index("n") * PPB if "n" in order else PPB - 1 if order[0] == "f" else 0
    tied = PPB if "n" in order else PPB * (len(order) - 1) + 1 if order[0] == "f" else PPB * len(order)
    pix = 300 + 140 * W
    return sc.finish(p, {"pixels": {"frame": [pix]}, "tie": (pix, winner, tied), "kinds": order})


# ---- E: the f32 1 % edge -------------------------------------------------------------------------------------------------------
def case_hqs_edge():
    """256 x 128, one unit box with zmin 1 at level 0: its rectangle is the whole image, cut to the 90 x 45 window in the middle.
    Triples (d, w_in, w_out = w_in + 1) of integer depths on one pixel, w_in = floor(RN_f32(d * 1.01f)): 'edge' triples have
    d = 100 m and w_in == RN_f32(d * 1.01f) == 101 m exactly, 'plain' triples d = 100 m + 37, 'fine' triples a d above 8.4e6 (see
    below). Each triple sits once on a pixel of the window and once on a pixel outside it (global path).
    facts: triples = [(pixel, d, w_in, w_out, kind)], window = (x0, y0, ww, wh)."""
    W, H = 256, 128
    p = make_params(W, H, 2.0 ** -20)
    sc = Scene(W, H)
    one01 = F32(1.01)
    ds, kinds = [], []
    for m in range(100, 1100):
        d = 100 * m
        if float(F32(d) * one01) == 101 * m and len(ds) < 1000:
            ds.append(d); kinds.append("edge")
            ds.append(d + 37); kinds.append("plain")
    n = len(ds)
    i = np.arange(n)
    x0, y0, ww, wh = 83, 41, 90, 45
    assert n == 1000
    places = [(x0 + i % ww, y0 + i // ww), (i % 256, 100 + i // 256)]                  # rows 41..52 of the window; rows 100..103
    # 'fine': d in [8.4e6, 1.6e7), where RN_f32(d * 1.01f) lies in [2^23, 2^24) and is an integer for every d (a 2^-10 grid of depths near 10^4,
    # scaled by a power of two): w_in is the rounded product itself on all of them. |x|, |y| <= 2^23 keeps them left of and below
    # the image centre: columns 83..127 x rows 53..63 of the window, columns 61..82 x rows 30..63 outside it.
    k = np.arange(450)
    ds += (8_400_000 + 15_919 * k).tolist()
    kinds += ["fine"] * len(k)
    places = [(np.concatenate([places[0][0], 83 + k % 45]), np.concatenate([places[0][1], 53 + k // 45])),
              (np.concatenate([places[1][0], 61 + k % 22]), np.concatenate([places[1][1], 30 + k // 22]))]
    ds = np.asarray(ds, np.int64)
    w_in = np.floor((ds.astype(F32) * one01).astype(np.float64)).astype(np.int64)
    xs, ys, zs, triples = [], [], [], []
    for col, row in places:
        for depth in (ds, w_in, w_in + 1):
            x, y = mid_pixel(col, row, depth, W, H)
            xs.append(x); ys.append(y); zs.append(depth)
        triples += [(int(c + r * W), int(d), int(a), int(a) + 1, kd) for c, r, d, a, kd in zip(col, row, ds, w_in, kinds)]
    lo, hi = unit_box(1)
    sc.add(lo, hi, 0, *unit_xyz(np.concatenate(xs), np.concatenate(ys), np.concatenate(zs), 1))
    sc.add_last()
    return sc.finish(p, {"pixels": {"frame": sorted(t[0] for t in triples)}, "triples": triples, "window": (x0, y0, ww, wh)})


# ---- F: window shapes ----------------------------------------------------------------------------------------------------------
def _window(W, H, rect, basic, hqs, stride=1):
    """One flat level-0 box at depth z0 = 32 max(W, H) whose rectangle under the rectangle rule is `rect` = (x0, y0, x1, y1)
    (given unclipped; clipped to the image by the rule), a point in the middle of every pixel its box reaches; then a unit box
    (zmin 1) with a point of its own depth in the middle of every pixel of the clipped rectangle and of the ring around it.
    basic / hqs: the window (x0, y0, ww, wh) each capacity must give, ww == 0 for none.
    A batch's points lie inside its box and the rule adds a pixel on every side, so a whole window's own points cannot reach its
    outermost pixels unless the image edge clips them off; those and the ring are reached by the second batch, which meets the
    first one's merge at every pixel. facts: rect, windows = {capacity: (x0, y0, ww, wh)}."""
    z0 = 32 * max(W, H)
    ux, uy = 2 * z0 // W, 2 * z0 // H
    p = make_params(W, H, 16.0)
    sc = Scene(W, H)
    rx0, ry0, rx1, ry1 = rect
    # screen box [rx0 + 1.25, rx1 - 0.25] x [ry0 + 1.25, ry1 - 0.25]: floor - 1 and floor + 1 give the rectangle
    lo = ((rx0 + 1.25 - W / 2) * ux, (ry0 + 1.25 - H / 2) * uy, z0)
    hi = ((rx1 - 0.25 - W / 2) * ux, (ry1 - 0.25 - H / 2) * uy, z0)
    cols = np.arange(max(rx0 + 1, 0), min(rx1 - 1, W - 1) + 1, stride)
    rows = np.arange(max(ry0 + 1, 0), min(ry1 - 1, H - 1) + 1)
    cc, rr = (a.ravel() for a in np.meshgrid(cols, rows))
    assert 0 < len(cc) <= PPB

    def coord(pix, half, unit, l, h):                 # the 30-bit coordinate nearest the pixel's middle
        if h == l:
            return np.zeros(len(pix), np.int64)
        return np.clip(np.rint(((pix - half + 0.5) * unit - l) / (h - l) * 2.0 ** 30), 0, 2 ** 30 - 1).astype(np.int64)
    sc.add(lo, hi, 0, coord(cc, W / 2, ux, lo[0], hi[0]), coord(rr, H / 2, uy, lo[1], hi[1]), [0], exact=False)
    cx0, cy0, cx1, cy1 = max(rx0, 0), max(ry0, 0), min(rx1, W - 1), min(ry1, H - 1)
    if stride == 1:
        cols = np.arange(max(cx0 - 1, 0), min(cx1 + 1, W - 1) + 1)
        rows = np.arange(max(cy0 - 1, 0), min(cy1 + 1, H - 1) + 1)
        gc, gr = (a.ravel() for a in np.meshgrid(cols, rows))
        assert len(gc) <= PPB
        depth = z0 - len(gc) // 2 + np.arange(len(gc))
        x, y = mid_pixel(gc, gr, depth, W, H)
        ulo, uhi = unit_box(1)
        sc.add(ulo, uhi, 0, *unit_xyz(x, y, depth, 1))
        cc, rr = gc, gr
    sc.add_last()
    pixels = sorted(set((cc + rr * W).tolist()))
    return sc.finish(p, {"pixels": {"frame": pixels}, "rect": (cx0, cy0, cx1, cy1), "windows": {WIN_PIXELS: basic, WIN_PIXELS_HQS: hqs}})


WINDOW_CASES = {
    # name: (W, H, rectangle x0 y0 x1 y1, basic window, colour window)
    "F_64x64": (2048, 128, (500, 30, 563, 93), (500, 30, 64, 64), (500, 30, 63, 63)),
    "F_63x65": (2048, 128, (500, 30, 562, 94), (500, 30, 63, 65), (500, 30, 63, 65)),
    "F_64x65": (2048, 128, (500, 30, 563, 94), (500, 30, 63, 64), (500, 30, 63, 64)),
    "F_128x64": (2048, 128, (500, 30, 627, 93), (519, 39, 90, 45), (519, 39, 90, 45)),      # cut well inside: own points outside it
    "F_3x100": (2048, 128, (700, 10, 702, 109), (700, 10, 3, 100), (700, 10, 3, 100)),
    "F_5x101": (2048, 128, (700, 10, 704, 110), (700, 10, 5, 101), (700, 10, 5, 101)),
    "F_7x99": (2048, 128, (700, 10, 706, 108), (700, 10, 7, 99), (700, 10, 7, 99)),
    "F_1365x3": (2048, 128, (300, 60, 1664, 62), (300, 60, 1365, 3), (300, 60, 1365, 3)),
    "F_none": (2048, 128, (-1, -1, 2048, 128), (0, 0, 0, 0), (0, 0, 0, 0)),                  # 262 144 pixels, over 16 x 4096
    "F_4096x1": (4096, 1, (-1, -1, 4096, 1), (0, 0, 4096, 1), (0, 0, 4095, 1)),
    "F_1x4096": (1, 4096, (-1, -1, 1, 4096), (0, 0, 1, 4096), (0, 0, 1, 4095)),
    "F_2x2048": (2, 2048, (-1, -1, 2, 2048), (0, 0, 2, 2048), (0, 0, 1, 2047)),
    "F_2048x2": (2048, 2, (-1, -1, 2048, 2), (0, 0, 2048, 2), (0, 0, 2047, 1)),
    "F_4096x1_w2": (4096, 1, (-1, -1, 1, 1), (0, 0, 2, 1), (0, 0, 2, 1)),                    # clipped at the left edge to width 2
}


# ---- G: the draw list ----------------------------------------------------------------------------------------------------------
G_W, G_H, G_BAND = 256, 128, 1280            # a batch of band 'b' lies 1280 units (ten screen widths) to the right


def _list_pixel(b):
    return 8 * (b % 32) + 4, 8 * (b // 32) + 4


def _list_scene(kinds):
    """256 x 128, depth 128 (one x unit and two y units per pixel), level 4. Batch b puts all its points on pixel
    (8 (b % 32) + 4, 8 (b // 32) + 4), the middle of its flat box: 'L' 16 x 16 pixels (light: a whole window), 'H' 256 x 128 pixels
    (heavy: larger than the window). A lower-case kind is the same batch in the second band, off screen at tx == 0."""
    sc = Scene(G_W, G_H)
    for b, kind in enumerate(kinds):
        ix, iy = _list_pixel(b)
        cx, cy = ix - 128 + (G_BAND if kind.islower() else 0), (iy - 64) * 2
        rx, ry = (8, 16) if kind in "Ll" else (128, 128)
        sc.add((cx - rx, cy - ry, 128), (cx + rx, cy + ry, 128), 4, [512 << 20], [512 << 20], [0])
    return sc


def _list_facts(kinds, frames):
    """frames: [(name, tx)]. drawn[name] = the batches drawn (all but the culled ones and the last), classes[name] per batch."""
    out = {"frames": [], "pixels": {}, "classes": {}, "drawn": {}}
    n = len(kinds)
    for name, tx in frames:
        vis = [(k.isupper() and tx == 0) or (k.islower() and tx == -G_BAND) for k in kinds]
        out["frames"].append((name, make_params(G_W, G_H, 2.0 ** -20, tx=tx, cull=1)))
        out["classes"][name] = ["C" if not v else k.upper() for k, v in zip(kinds, vis)]
        out["drawn"][name] = [b for b in range(n - 1) if vis[b]]
        out["pixels"][name] = sorted(_list_pixel(b)[0] + _list_pixel(b)[1] * G_W for b in out["drawn"][name])
    out["levels"] = [4 if c != "C" else -1 for c in out["classes"][frames[0][0]]]
    return out


def _list_small(kinds):
    sc = _list_scene(kinds)
    f = _list_facts(kinds, [("frame", 0)])
    return sc.finish(f["frames"][0][1], f)


def _heavy_set(extra):
    return {63, 64, 127, 128, 191, 192, 255, 256} | set(range(2, 2 + 4 * extra, 4))


def case_list_under_quarter():
    """258 batches, none culled: 257 drawn, 64 of them heavy (64 * 4 < 257: drawn class by class), heavy ones at the prepass's wave
    borders 63/64, 127/128, 191/192 and the chunk border 255/256."""
    heavy = _heavy_set(56)
    kinds = "".join("H" if b in heavy else "L" for b in range(258))
    f = _list_facts(kinds, [("frame", 0)])
    f["heavy_drawn"] = {"frame": 64}
    return _list_scene(kinds).finish(f["frames"][0][1], f)


def case_list_frames():
    """258 batches; batch 256 is heavy and lies in the second band. tx == 0 ('many'): 256 drawn, 64 heavy -- exactly a quarter, the
    list is walked in file order, chunk 1 has no record. tx == -1280 ('few'): chunk 0 entirely culled, the one heavy batch of
    chunk 1 drawn. tx == +1280 ('none'): everything culled. Drawn many, few, none, many on one context."""
    heavy = _heavy_set(57)
    kinds = "".join("h" if b == 256 else "H" if b in heavy else "L" for b in range(258))
    f = _list_facts(kinds, [("many", 0), ("few", -G_BAND), ("none", G_BAND), ("many again", 0)])
    f["heavy_drawn"] = {"many": 64, "few": 1, "none": 0, "many again": 64}
    return _list_scene(kinds).finish(f["frames"][0][1], f)


def case_list_quarter():
    """260 batches, three light ones (9, 100, 200) culled: 256 drawn, 64 heavy -- exactly a quarter, so the list is walked in file
    order -- with heavy batches on both sides of the wave borders and of the chunk border 255/256, and records in both chunks."""
    heavy = _heavy_set(56)
    kinds = "".join("l" if b in (9, 100, 200) else "H" if b in heavy else "L" for b in range(260))
    f = _list_facts(kinds, [("frame", 0)])
    f["heavy_drawn"] = {"frame": 64}
    return _list_scene(kinds).finish(f["frames"][0][1], f)


SMALL_LISTS = ["LHl" + a + b for a in "lHL" for b in "lHL"] + ["llll", "lllL", "HLHLlHLHLHLlLHLL"]

CASES = {
    "A_level_cuts": case_level_cuts,
    "B_fields": case_fields,
    "C_border": case_border,
    **{"D_ties_" + o: functools.partial(_ties, o) for o in TIE_ORDERS},
    "E_hqs_edge": case_hqs_edge,
    **{name: functools.partial(_window, v[0], v[1], v[2], v[3], v[4], 4 if name == "F_none" else 1) for name, v in WINDOW_CASES.items()},
    **{"G_list_" + k: functools.partial(_list_small, k) for k in SMALL_LISTS},
    "G_list_258_under_quarter": case_list_under_quarter,
    "G_list_260_quarter": case_list_quarter,
    "G_list_258_frames": case_list_frames,
}


@functools.lru_cache(maxsize=4)
def build(name: str):
    return CASES[name]()


def algorithmic_bytes(levels, colour: bool) -> int:
    """What a frame reads, by the levels of its drawn batches (all but the last): the record, 4 / 8 / 12 bytes per point, and in
    the colour pass 4 bytes of colour per point."""
    return sum(64 + PPB * 4 * ((1 if l >= 2 else 2 if l == 1 else 3) + (1 if colour else 0)) for l in levels[:-1] if l >= 0)


def full_frame_elems(W: int, H: int) -> int:
    return fb_elems(W, H)
