"""Streams, polygons and the numpy side of the polygon-selection tests (tests/test_polygon_cpu.py checks on the CPU, against the
oracle's decoder, that the polygons do what tests/test_gpu_polygon.py needs them to do). Inputs and reference arithmetic only:
in_poly vectorised in int64 and as a plain loop over Python integers, the class rule and the edge-list rule of include/pcr_hip.h."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import select_cases as S

PPB = S.PPB
OUTSIDE, INSIDE, STRADDLING = 0, 1, 2
INT32_MIN, INT32_MAX = S.INT32_MIN, S.INT32_MAX
MAX_VERTICES, INVERT = 4096, 1
MAX_EXTENT = (1 << 31) - 1


class Poly:
    """rings: lists of (x, y) integer vertices; z_min..z_max inclusive; invert: the points not inside (z still applies)."""

    def __init__(self, rings, z_min=INT32_MIN, z_max=INT32_MAX, invert=False):
        self.rings = [[(int(x), int(y)) for x, y in r] for r in rings]
        self.z_min, self.z_max, self.invert = int(z_min), int(z_max), bool(invert)

    def inverted(self):
        return Poly(self.rings, self.z_min, self.z_max, not self.invert)

    def with_z(self, z_min, z_max):
        return Poly(self.rings, z_min, z_max, self.invert)

    def native(self):
        return P.Polygon(self.rings, self.z_min, self.z_max, self.invert)

    def rect(self):
        v = np.array([p for r in self.rings for p in r], np.int64)
        return int(v[:, 0].min()), int(v[:, 1].min()), int(v[:, 0].max()), int(v[:, 1].max())

    def edges(self):
        """Every edge of every ring in ring order as (l.x, l.y, dx, dy) from its lower endpoint, dy >= 0; a horizontal edge
        (dy == 0) from its left end."""
        out = []
        for r in self.rings:
            for i, a in enumerate(r):
                b = r[(i + 1) % len(r)]
                lo, up = (a, b) if (a[1], a[0]) <= (b[1], b[0]) else (b, a)
                out.append((lo[0], lo[1], up[0] - lo[0], up[1] - lo[1]))
        return out


# ---- the predicate -------------------------------------------------------------------------------------------------------------
def in_poly_loop(poly, x, y):
    """in_poly of one point, the rule as written, in Python integers (no rectangle test: nothing can overflow)."""
    x, y, odd = int(x), int(y), False
    for r in poly.rings:
        for i, a in enumerate(r):
            b = r[(i + 1) % len(r)]
            if a[1] == b[1]:
                continue
            lo, up = (a, b) if a[1] < b[1] else (b, a)
            if lo[1] <= y < up[1] and (x - lo[0]) * (up[1] - lo[1]) < (y - lo[1]) * (up[0] - lo[0]):
                odd = not odd
    return odd


def selected_loop(poly, xyz):
    return np.array([poly.z_min <= int(z) <= poly.z_max and in_poly_loop(poly, x, y) != poly.invert for x, y, z in xyz], bool)


def in_poly(poly, x, y):
    """in_poly of integer arrays x, y in int64. Points outside the vertices' rectangle are not in the polygon; the others have
    every difference below 2^31, so the products fit. An edge touches only the points of its rows: a slice of the points in y order."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    x0, y0, x1, y1 = poly.rect()
    assert x1 - x0 <= MAX_EXTENT and y1 - y0 <= MAX_EXTENT
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    order = np.argsort(y, kind="stable")
    ys, xs = y[order], np.clip(x[order], x0, x1)
    odd = np.zeros(len(x), bool)
    for lx, ly, dx, dy in poly.edges():
        if dy == 0:
            continue
        a, b = np.searchsorted(ys, [ly, ly + dy], "left")
        if a < b:
            odd[a:b] ^= (xs[a:b] - lx) * dy < (ys[a:b] - ly) * dx
    out = np.empty(len(x), bool)
    out[order] = odd
    return out & inside


def selected(poly, xyz):
    """Boolean mask of the rows of an integer [n, 3] array the prism selects."""
    xyz = np.asarray(xyz, np.int64)
    return (xyz[:, 2] >= poly.z_min) & (xyz[:, 2] <= poly.z_max) & (in_poly(poly, xyz[:, 0], xyz[:, 1]) != poly.invert)


# ---- the host plan, restated -----------------------------------------------------------------------------------------------------
def plan_batch(poly, bb):
    """(class, base parity, edge list) of a batch with the exact box bb = min x, y, z, max x, y, z, by the rule of pcr_hip.h."""
    bx0, by0, bz0, bx1, by1, bz1 = (int(v) for v in bb)
    if poly.z_min > poly.z_max or bz1 < poly.z_min or bz0 > poly.z_max:
        return OUTSIDE, 0, []
    z_all_in = poly.z_min <= bz0 and bz1 <= poly.z_max
    edges = poly.edges()
    box = [(min(lx, lx + dx), ly, max(lx, lx + dx), ly + dy) for lx, ly, dx, dy in edges]
    near = any(ex0 <= bx1 and ex1 >= bx0 and ey0 <= by1 and ey1 >= by0 for ex0, ey0, ex1, ey1 in box)
    if not near:
        if in_poly_loop(poly, bx0, by0) == poly.invert:
            return OUTSIDE, 0, []
        if z_all_in:
            return INSIDE, 0, []
    base, listed = 0, []
    for e, (ex0, ey0, ex1, ey1) in zip(edges, box):
        if ey0 == ey1 or ey0 > by1 or ey1 <= by0 or ex1 <= bx0:     # horizontal, rows missed, nothing of the rectangle left of it
            continue
        if ex0 > bx1 and ey0 <= by0 and ey1 > by1:
            base ^= 1
        else:
            listed.append(e)
    return STRADDLING, base, listed


def plan(poly, bounds):
    return [plan_batch(poly, bb) for bb in np.asarray(bounds, np.int64)]


def plan_stats(plans):
    strad = [len(p[2]) for p in plans if p[0] == STRADDLING]
    return {"batches_outside": sum(p[0] == OUTSIDE for p in plans), "batches_inside": sum(p[0] == INSIDE for p in plans),
            "batches_straddling": len(strad), "edges_listed": sum(strad), "edges_max": max(strad, default=0)}


def refusal(rings, flags=0, reserved=0):
    """Why pcr_select_polygon refuses a polygon (None: it does not)."""
    if len(rings) < 1 or any(len(r) < 3 for r in rings):
        return "rings"
    if sum(len(r) for r in rings) > MAX_VERTICES:
        return "vertices"
    if flags & ~INVERT or reserved:
        return "flags"
    v = np.array([p for r in rings for p in r], np.int64)
    if ((v.max(axis=0) - v.min(axis=0)) > MAX_EXTENT).any():
        return "extent"
    return None


# ---- streams ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream(name):
    if name == "wide30xy":                              # select_cases' wide30 with the hop on x and on y: two batches, two clusters 2^30 apart on both axes
        rng = np.random.default_rng(22)
        n = 65536 * 2
        hop = np.where(np.arange(n) % 2 == 0, 0, 1 << 30).astype(np.int64)
        x = (hop + rng.integers(0, 3, n)).astype(np.int32)
        y = (hop + rng.integers(0, 2000, n)).astype(np.int32)
        z = rng.integers(0, 50, n).astype(np.int32)
        c = rng.integers(0, 1 << 24, n).astype(np.uint32)
        return S._keep(P.encode_points(x, y, z, c, S.las_for((0, 0, 0), (1 << 30, 1 << 30, 50)), morton_sort=False, nthreads=2)[0])
    return S.stream(name)


def golden(name):
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".huffman"), "rb").read()


# ---- polygons ----------------------------------------------------------------------------------------------------------------------
def ring_box(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


# synth (10 batches, boxes of a 3D Morton order): the east of the tile with a notch cut into its west side. Batch 9 lies inside
# with no edge near it, batch 0 outside, batches 3 and 8 are crossed by the notch; the inverse swaps inside and outside.
CONCAVE = Poly([[(524_000, -10_000), (1_010_000, -10_000), (1_010_000, 1_010_000), (524_000, 1_010_000), (524_000, 600_000), (800_000, 500_000),
                 (524_000, 400_000)]])
# clustered (5 batches): everything, with a hole around the centre cluster: batch 1 lies inside the hole
HOLE = Poly([ring_box(-50_000, -50_000, 1_100_000, 1_100_000), ring_box(470_000, 485_000, 525_000, 528_000)])
# wide30 (x in 0..2 and 2^30 + 0..2, y in 0..1999: about eleven points per lattice site): every vertex a decoded point, a
# horizontal, two vertical and two diagonal edges, all through lattice sites
BOUNDARY = Poly([[(0, 100), (2, 100), (2, 300), (1, 400), (0, 302)]])
# wide30: two polygons that share the diagonal (0, 1000) - (3, 1300), which passes through the sites (1, 1100) and (2, 1200)
PART_A = Poly([[(0, 900), (3, 900), (3, 1300), (0, 1000)]])
PART_B = Poly([[(0, 1000), (3, 1300), (3, 1500), (0, 1500)]])
PART_MERGED = Poly([[(0, 900), (3, 900), (3, 1500), (0, 1500)]])
# garbage_tail: a slanted strip over the north end that reaches past the header's box, where only the tail artefact lies
TAIL = Poly([[(-1_000, 990_000), (1_001_000, 995_000), (1_001_000, 1_010_000), (-1_000, 1_010_000)]])
TAIL_BEYOND_Y = 1_000_000
EVERYTHING = Poly([ring_box(INT32_MIN // 2, INT32_MIN // 2, INT32_MAX // 2, INT32_MAX // 2)])
COLLINEAR = Poly([[(0, 0), (500_000, 500_000), (1_000_000, 1_000_000), (250_000, 250_000)]])
# escape_heavy (two batches that each span the cloud): a quadrilateral across it with a z range
ESCAPE_QUAD = Poly([[(-900_000, -1_000_000), (700_000, -300_000), (1_000_000, 900_000), (-200_000, 400_000)]], -20_000, 30_000)
# synth: the rectangle and the slab that tests/test_gpu_polygon.py holds against read_box
RECT_BOX = ((500_000, 640_000, 0), (900_000, 950_000, 50_000))          # x0, y0, z0 and x1, y1, z1 of the rectangle polygon
RECT = Poly([ring_box(*RECT_BOX[0][:2], *RECT_BOX[1][:2])], RECT_BOX[0][2], RECT_BOX[1][2])
SLAB = EVERYTHING.with_z(20_000, 40_000)
# wide30: a comb of 4093 tooth edges over x = 1 .. 4094, each crossing all rows of the cloud, closed far above it. Both batches
# reach from x = 0 to 2^30 + 2, so every tooth edge and the western closing edge are listed for them: all but two of 4096 edges
COMB = Poly([[(1 + i, -10 if i % 2 == 0 else 2_500) for i in range(MAX_VERTICES - 2)] + [(MAX_VERTICES - 2, 6_000), (1, 6_000)]])
COMB_LISTED = MAX_VERTICES - 2
GOLDEN = ["config1", "ref_packed_batch", "ref_packed_lowentropy", "ref_packed_bc7"]
# wide30xy: the vertices span 2^31 - 1 on both axes; the diagonal y = x + 999 cuts both clusters in half and the long southern edge
# rises 305 over its length, so a point of the far cluster multiplies 2^30 by 2^31
WIDE_X0, WIDE_X1 = -5, -5 + MAX_EXTENT
WIDE = Poly([[(WIDE_X0, 994), (WIDE_X0, -5), (WIDE_X1, 300), (WIDE_X1, WIDE_X1), (WIDE_X1 - 999, WIDE_X1)]])
WIDE_TOO_FAR = [[(WIDE_X0, 994), (WIDE_X0, -5), (WIDE_X1 + 1, 300), (WIDE_X1 + 1, WIDE_X1), (WIDE_X1 - 999, WIDE_X1)]]


@functools.lru_cache(maxsize=None)
def zigzag(centre=(500_000, 500_000), r_mid=635_000, amp=85_000, n=MAX_VERTICES):
    """A ring of n integer vertices around `centre` whose radius alternates between r_mid - amp and r_mid + amp. On clustered its
    band runs through the four corner clusters."""
    k = np.arange(n)
    r = r_mid + np.where(k % 2 == 0, -amp, amp)
    a = 2.0 * np.pi * k / n
    return Poly([np.stack([np.rint(centre[0] + r * np.cos(a)), np.rint(centre[1] + r * np.sin(a))], axis=1).astype(np.int64).tolist()])


def quantile_triangle(xyz):
    """A triangle through order statistics of the distinct points (exact integers; a short stream is mostly its last point
    repeated as padding): it cuts through the middle of any cloud."""
    s = np.sort(np.unique(np.asarray(xyz, np.int64), axis=0), axis=0)
    n = len(s)
    q = lambda k, f: int(s[min(int(n * f), n - 1), k])
    return Poly([[(q(0, 0.1), q(1, 0.15)), (q(0, 0.9), q(1, 0.4)), (q(0, 0.45), q(1, 0.9))]], q(2, 0.05), q(2, 0.9))


def on_boundary(poly, x, y):
    """Boolean mask of the points that lie exactly on an edge (a vertex included)."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    out = np.zeros(len(x), bool)
    for lx, ly, dx, dy in poly.edges():
        t, u = x - lx, y - ly
        out |= (t * dy == u * dx) & (u >= 0) & (u <= dy) & (t >= min(dx, 0)) & (t <= max(dx, 0))
    return out
