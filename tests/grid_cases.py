"""Streams, grids and the numpy side of the top-down grid tests (tests/test_grid_cpu.py checks on the CPU, against the oracle's
decoder, that the grids do what tests/test_gpu_grid.py needs them to do). Inputs and reference arithmetic only."""
from __future__ import annotations

import functools
import os

import numpy as np

import pcrhpg24_amd as P
from tests import select_cases as S

PPB = S.PPB
INT32_MIN, INT32_MAX = S.INT32_MIN, S.INT32_MAX
WINDOW_CELLS = 4096                                 # PCR_GRID_WINDOW_CELLS
MAX_CELLS = 1 << 26                                 # PCR_GRID_MAX_CELLS
NO_WINDOW = 1                                       # PCR_GRID_NO_WINDOW
EMPTY_TOP, EMPTY_BOTTOM = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN = ["ref_packed_bc7"]

# (stream, grid = (origin_x, origin_y, cell, width, height), the class of every batch -- O outside, W windowed, D direct -- or
# None where only "no batch outside" is claimed). Chosen from the oracle's exact batch boxes with WINDOW_CELLS = 4096; the cells
# are 1, 3, 7001, 9973, 2^16 and 2^24 among others: powers of two take the shift, the others the multiply-high division.
CASES = [
    ("synth", (0, 0, 7001, 143, 143), "WDDDDWWDWW"),
    ("synth", (530000, 530000, 4000, 118, 118), "OOOOWOOWDD"),          # all three classes
    ("synth", (0, 0, 65536, 16, 16), "WWWWWWWWWW"),
    ("synth", (400000, 400000, 3, 1500, 1500), "ODDODOOOOO"),
    ("escape_heavy", (-1048576, -1048576, 32768, 64, 64), "WW"),        # negative coordinates
    ("escape_heavy", (-300000, -200000, 9973, 40, 30), "WW"),
    ("wide30", (0, 0, 1 << 24, 65, 1), "WW"),                           # x up to 2^30
    ("wide30", (0, 0, 1, 4, 2000), "DD"),
    ("plateau", (0, 0, 1000, 64, 64), "WW"),                            # z in {0..3}: nearly every cell has a tie for the top z
    ("clustered", (0, 0, 20000, 50, 50), None),
    ("garbage_tail", (0, 0, 50000, 20, 20), None),
    ("wide20", (0, 0, 1 << 16, 17, 1), None),
    ("ref_packed_bc7", None, None),                                     # grid from the stream's own box, see grid_over
]
PLATEAU_GRID = (0, 0, 1000, 64, 64)


def golden(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".huffman"), "rb").read()


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image of a named stream: those of tests/select_cases.py, the golden BC7 file, and `plateau`."""
    if name in GOLDEN:
        return golden(name)
    if name == "plateau":
        rng = np.random.default_rng(5)
        n = 131072
        x = rng.integers(0, 64000, n).astype(np.int32)
        y = rng.integers(0, 64000, n).astype(np.int32)
        z = rng.integers(0, 4, n).astype(np.int32)
        c = rng.integers(0, 1 << 24, n).astype(np.uint32)
        return S._keep(P.encode_points(x, y, z, c, S.las_for((0, 0, 0), (64000, 64000, 3)), morton_sort=True, nthreads=2)[0])
    return S.stream(name)


def grid_over(bounds, cells=48):
    """A grid of about `cells` x `cells` cells over the box of all batches (exact integers from the bounds), a non-power-of-two
    cell: for streams whose coordinates the cases above do not know."""
    b = np.asarray(bounds, np.int64)
    lo, hi = b[:, :2].min(axis=0), b[:, 3:5].max(axis=0)
    cell = int(max(1, (max(hi - lo) + cells) // cells)) | 1
    cell += 2 if cell & (cell - 1) == 0 else 0
    return int(lo[0]), int(lo[1]), cell, int((hi[0] - lo[0]) // cell + 1), int((hi[1] - lo[1]) // cell + 1)


def keys(pts):
    """K = (uint64)((uint32)z ^ 0x80000000) << 32 | colour of every record of a POINT_DTYPE array."""
    zb = (pts["z"].astype(np.int64) + (1 << 31)).astype(np.uint64)
    return (zb << np.uint64(32)) | pts["color"].astype(np.uint64)


def cells_of(pts, grid, clip=None):
    """(mask, index): which records fall into a cell of the grid (and into clip), and the linear cell index of those."""
    ox, oy, cell, w, h = (int(v) for v in grid)
    x, y = pts["x"].astype(np.int64), pts["y"].astype(np.int64)
    cx, cy = (x - ox) // cell, (y - oy) // cell
    m = (x >= ox) & (y >= oy) & (cx < w) & (cy < h)
    if clip is not None:
        m &= S.in_box(np.stack([pts["x"], pts["y"], pts["z"]], axis=1), clip)
    return m, (cx + cy * w)[m]


def reference(pts, grid, clip=None):
    """top, bottom (uint64) and count (uint32), shaped [height, width], over the records of a POINT_DTYPE array."""
    w, h = int(grid[3]), int(grid[4])
    m, idx = cells_of(pts, grid, clip)
    k = keys(pts)[m]
    top, bottom = np.full(w * h, EMPTY_TOP, np.uint64), np.full(w * h, EMPTY_BOTTOM, np.uint64)
    np.maximum.at(top, idx, k)
    np.minimum.at(bottom, idx, k)
    count = np.bincount(idx, minlength=w * h).astype(np.uint32)
    return top.reshape(h, w), bottom.reshape(h, w), count.reshape(h, w)


def classify(bounds, grid, clip=None, flags=0):
    """The class of every batch box, as a string of O / W / D: outside -- the box misses grid and clip intersected on x, y or z;
    windowed -- the rectangle of cells it covers inside them has at most WINDOW_CELLS cells; direct -- more (or NO_WINDOW)."""
    ox, oy, cell, w, h = (int(v) for v in grid)
    lo = np.array(S.FULL[0] if clip is None else clip[0], np.int64)
    hi = np.array(S.FULL[1] if clip is None else clip[1], np.int64)
    lo[:2] = np.maximum(lo[:2], (ox, oy))
    hi[:2] = np.minimum(hi[:2], (ox + cell * w - 1, oy + cell * h - 1))
    out = []
    for b in np.asarray(bounds, np.int64):
        if (lo > hi).any() or (b[3:] < lo).any() or (b[:3] > hi).any():
            out.append("O")
            continue
        c0 = (np.maximum(b[:2], lo[:2]) - (ox, oy)) // cell
        c1 = (np.minimum(b[3:5], hi[:2]) - (ox, oy)) // cell
        cells = int((c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1))
        out.append("W" if cells <= WINDOW_CELLS and not flags & NO_WINDOW else "D")
    return "".join(out)


def class_counts(cls: str) -> dict:
    return {"batches_outside": cls.count("O"), "batches_windowed": cls.count("W"), "batches_direct": cls.count("D")}


def unpack(words, which_empty):
    """height (int32, INT32_MIN where empty) and rgba (uint32, 0 where empty) of a plane of words."""
    z = ((words >> np.uint64(32)).astype(np.int64) - (1 << 31)).astype(np.int32)
    rgba = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32) | np.uint32(0xFF000000)
    empty = words == which_empty
    return np.where(empty, np.int32(INT32_MIN), z), np.where(empty, np.uint32(0), rgba)
