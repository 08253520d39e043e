"""Streams, grids and the numpy side of the ground-filter and height-selection tests (tests/test_ground_cpu.py checks on the CPU,
against the oracle's decoder, that the `town` stream does what tests/test_gpu_ground.py needs it to do). Inputs and reference
arithmetic only. The reference is a literal restatement of the definition in include/pcr_hip.h: shifted-window minimum and
maximum over a padded plane with int64 cells and a mask for "empty", and a Jacobi fill with //."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import grid_cases as G
from tests import select_cases as S

PPB = S.PPB
INT32_MIN, INT32_MAX = S.INT32_MIN, S.INT32_MAX
EMPTY = INT32_MIN                                   # PCR_GROUND_EMPTY
CELL_EMPTY, CELL_GROUND, CELL_NONGROUND = 0, 1, 2
MAX_STEPS, MAX_RADIUS, MAX_FILL = 16, 64, 4096
REPLACE_Z = 1
STAT_KEYS = ("cells_empty", "cells_ground", "cells_nonground", "cells_filled", "cells_unfilled", "fill_rounds")

# (grid = (origin_x, origin_y, cell, width, height), radii, thresholds) over `town`
TOWN = [
    ((0, 0, 1000, 64, 64), (1, 2, 4, 8), (60, 85, 135, 235)),
    ((-500, -300, 777, 84, 84), (1, 3, 7, 15), (50, 90, 160, 300)),            # the multiply-high division, a negative origin
    ((10000, 10000, 1000, 30, 20), (1, 2, 4, 8), (60, 85, 135, 235)),           # batches partly outside the grid
]
# the figures of a numpy prototype over the points of `town` before padding (tests/test_ground_cpu.py reproduces them)
TOWN_FIGURES = [
    dict(empty=48, flagged=166, per_step=(13, 35, 28, 90), rounds=5, unfilled=0, covered=128712),
    dict(empty=250, flagged=246, rounds=6),
    dict(flagged=80, rounds=8, covered=19097),
]
HEIGHT_RANGES = [(-30, 30), (200, 2000), (2001, INT32_MAX)]                     # ground, vegetation, buildings
TOWN_RECORDS = (94927, 10645, 4903)                                             # the records of the first grid in each range


def town_points():
    """x, y, z, colour of `town` before encoding: a sloped terrain with noise, three buildings, a wood, a lake without returns."""
    rng = np.random.default_rng(11)
    n = 131072
    x = rng.integers(0, 64000, n); y = rng.integers(0, 64000, n)
    z = 1000 + x // 40 + y // 80 + rng.integers(0, 21, n)
    for x0, y0, x1, y1, h in [(8000, 8000, 18000, 20000, 3000), (30500, 40500, 36500, 43500, 1500), (50000, 10000, 62000, 13000, 6000)]:
        m = (x >= x0) & (x < x1) & (y >= y0) & (y < y1); z[m] += h                      # buildings
    t = (x >= 20000) & (x < 60000) & (y >= 22000) & (y < 38000) & (rng.random(n) < 0.5)  # trees
    z[t] += rng.integers(200, 1500, t.sum())
    keep = ~((x >= 40200) & (x < 49800) & (y >= 48200) & (y < 55800))                    # a lake without returns
    c = rng.integers(0, 1 << 24, n)
    return x[keep].astype(np.int32), y[keep].astype(np.int32), z[keep].astype(np.int32), c[keep].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image of a named stream: `town`, and those of tests/grid_cases.py."""
    if name == "town":
        x, y, z, c = town_points()
        return S._keep(P.encode_points(x, y, z, c, S.las_for((0, 0, 0), (64000, 64000, 9000)), morton_sort=True, nthreads=2)[0])
    return G.stream(name)


def params(radii, thresholds, fill_rounds=MAX_FILL):
    return P.GroundParams(radii, thresholds, fill_rounds)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _window(values, valid, r, op, identity):
    """op over the valid cells of the (2r+1)^2 window around every cell, and whether the window holds one: shifted copies of
    a plane padded by r with invalid cells, the row pass followed by the column pass. int64 values, bool valid."""
    h, w = values.shape
    v = np.where(valid, values, identity)
    for axis in (1, 0):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(v, pad, constant_values=identity)
        n = v.shape[axis]
        cut = lambda d: p[:, d:d + n] if axis == 1 else p[d:d + n, :]
        v = cut(0)
        for d in range(1, 2 * r + 1):
            v = op(v, cut(d))
    return v, v != identity


def opening(a, valid, r):
    """(E, O) of one step as int64 planes with EMPTY for "none": E the minimum of a over the valid cells of W_r, O the maximum of
    E over its non-EMPTY cells."""
    big = np.int64(1) << 40
    e, ev = _window(a, valid, r, np.minimum, big)
    o, ov = _window(e, ev, r, np.maximum, -big)
    return np.where(ev, e, EMPTY), np.where(ov, o, EMPTY)


def fill_round(h):
    """One Jacobi round over an int64 plane with EMPTY cells: (the new plane, the number of cells it filled)."""
    hh, ww = h.shape
    valid = np.pad(h != EMPTY, 1, constant_values=False)
    vals = np.pad(np.where(h != EMPTY, h, 0), 1, constant_values=0)
    m, s = np.zeros((hh, ww), np.int64), np.zeros((hh, ww), np.int64)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                m += valid[dy:dy + hh, dx:dx + ww]
                s += vals[dy:dy + hh, dx:dx + ww]
    take = (h == EMPTY) & (m >= 1)
    out = h.copy()
    out[take] = s[take] // m[take]                                              # numpy's // floors toward minus infinity
    return out, int(take.sum())


def ground_filter(z0, radii, thresholds, fill_rounds=MAX_FILL, steps_out=None):
    """(ground int32, classes uint8, stats dict) of an int32 [height, width] plane, by the definition. steps_out: a list that
    receives the number of newly flagged cells of every step."""
    z0 = np.asarray(z0, np.int32)
    nonempty = z0 != EMPTY
    a = z0.astype(np.int64)
    f = np.zeros(z0.shape, bool)
    for r, t in zip(radii, thresholds):
        _, o = opening(a, nonempty, int(r))
        assert (o[nonempty] <= a[nonempty]).all() and (o[nonempty] != EMPTY).all()
        new = nonempty & (a - o > int(t))
        if steps_out is not None:
            steps_out.append(int((new & ~f).sum()))
        f |= new
        a = np.where(nonempty, o, EMPTY)
    classes = np.where(~nonempty, CELL_EMPTY, np.where(f, CELL_NONGROUND, CELL_GROUND)).astype(np.uint8)
    h = np.where(classes == CELL_GROUND, z0.astype(np.int64), EMPTY)
    st = dict(cells_empty=int((classes == CELL_EMPTY).sum()), cells_ground=int((classes == CELL_GROUND).sum()),
              cells_nonground=int((classes == CELL_NONGROUND).sum()), cells_filled=0, cells_unfilled=0, fill_rounds=0)
    for _ in range(int(fill_rounds)):
        if not (h == EMPTY).any():
            break
        h, filled = fill_round(h)
        if filled == 0:
            break
        st["cells_filled"] += filled
        st["fill_rounds"] += 1
    st["cells_unfilled"] = int((h == EMPTY).sum())
    return h.astype(np.int32), classes, st


def lowest(pts, grid, clip=None):
    """The lowest-point height plane of a POINT_DTYPE array: int32 [height, width], EMPTY for a cell without points."""
    return G.unpack(G.reference(pts, grid, clip)[1], G.EMPTY_BOTTOM)[0]


def heights(pts, grid, ground, clip=None):
    """(in a cell of the grid and the clip, on a cell with ground, h as int64 -- meaningful where both hold) per record."""
    w = int(grid[3])
    m, idx = G.cells_of(pts, grid, clip)
    g = np.full(len(pts), EMPTY, np.int64)
    g[m] = np.asarray(ground, np.int64).ravel()[idx]
    has = m & (g != EMPTY)
    return m, has, pts["z"].astype(np.int64) - g


def select_height(pts, grid, ground, h_min, h_max, clip=None, replace_z=False):
    """(records, heights int32, points_no_ground) of the definition over a POINT_DTYPE array."""
    m, has, h = heights(pts, grid, ground, clip)
    sel = has & (h >= int(h_min)) & (h <= int(h_max))
    out = pts[sel].copy()
    hs = h[sel].astype(np.int32)
    if replace_z:
        out["z"] = hs
    return out, hs, int((m & ~has).sum())


def height_classes(bounds, grid, clip=None):
    """{batches_outside, batches_decoded} of the batch boxes against grid and clip intersected."""
    cls = G.classify(bounds, grid, clip, flags=G.NO_WINDOW)
    return {"batches_outside": cls.count("O"), "batches_decoded": cls.count("D")}
