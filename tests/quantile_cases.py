"""Streams, grids and the numpy side of the height-percentile tests (tests/test_grid_quantiles_cpu.py proves on the CPU, against
the oracle's decoder, what tests/test_gpu_grid_quantiles.py relies on). Inputs and reference arithmetic only. The streams and
CASES of tests/grid_cases.py are reused by import: their batch classes are proven in tests/test_grid_cpu.py."""
from __future__ import annotations

import functools

import numpy as np

import pcrhpg24_amd as P
from tests import grid_cases as G
from tests import select_cases as S

PPB = S.PPB
INT32_MIN, INT32_MAX = S.INT32_MIN, S.INT32_MAX
ONE = 10000                                         # PCR_QUANTILE_ONE
QUANTILES_MAX = 8                                   # PCR_QUANTILES_MAX
SMALL_MAX = 64                                      # the largest cell the wave-per-cell select takes
Q8 = (0, 100, 2500, 5000, 9500, 10000, 5000, 1)     # eight ranks, one repeated, unsorted

# ---- the constructed stream --------------------------------------------------------------------------------------------------
# A 48 x 48 grid of 1000-step cells. The cells of the left half (cx < 24) are constructed one by one, the right half holds
# filler that brings the stream to exactly two batches (and through which the Morton order puts the batch boundary).
EDGES_GRID = (0, 0, 1000, 48, 48)
POPULATIONS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 5000)    # the small/large edge and the tile edges of both selects
POP_CELLS = {n: (2, 2 + 3 * i) for i, n in enumerate(POPULATIONS)}         # population -> (cx, cy)
CELL_EQUAL, CELL_LOW_BYTE, CELL_HIGH_BYTE, CELL_REPEAT = (8, 4), (8, 10), (8, 16), (8, 22)
SPECIAL_N = 300
REPEAT_LOW, REPEAT_HIGH = (10, 50), (20, 51)        # (z, how many): ranks 0 .. 49 hold 10, ranks 50 .. 100 hold 20


def cell_index(cell, grid=EDGES_GRID):
    return cell[1] * grid[3] + cell[0]


def _edge_cells():
    """{(cx, cy): z values} of every constructed cell."""
    rng = np.random.default_rng(2024)
    cells = {}
    for n, at in POP_CELLS.items():
        if n == 2:
            z = np.array([100, 200])
        elif n == 3:
            z = np.array([100, 200, 300])
        elif n == 5000:
            z = rng.integers(-(1 << 20), 1 << 20, n)                      # three bytes differ, both signs
        else:
            z = rng.integers(-30000, 30000, n)
        cells[at] = z.astype(np.int64)
    cells[CELL_EQUAL] = np.full(SPECIAL_N, 777, np.int64)                   # every radix pass lands in one bin
    cells[CELL_LOW_BYTE] = 0x12345600 + rng.integers(0, 256, SPECIAL_N)     # only the lowest byte differs
    cells[CELL_HIGH_BYTE] = (rng.integers(-64, 64, SPECIAL_N) << 24) + 0x123456     # only the highest; the sign flip decides
    cells[CELL_REPEAT] = np.repeat([REPEAT_LOW[0], REPEAT_HIGH[0]], [REPEAT_LOW[1], REPEAT_HIGH[1]]).astype(np.int64)
    return cells


@functools.lru_cache(maxsize=None)
def edge_points():
    """x, y, z (int32) and colour (uint32) of quantile_edges before encoding: 131 072 points."""
    rng = np.random.default_rng(7)
    xs, ys, zs = [], [], []
    for (cx, cy), z in _edge_cells().items():
        xs.append(cx * 1000 + rng.integers(0, 1000, len(z))); ys.append(cy * 1000 + rng.integers(0, 1000, len(z))); zs.append(z)
    used = sum(len(z) for z in zs)
    fill = 2 * PPB - used
    xs.append(rng.integers(24000, 48000, fill)); ys.append(rng.integers(0, 48000, fill)); zs.append(rng.integers(-30000, 30000, fill))
    x, y, z = (np.concatenate(v).astype(np.int32) for v in (xs, ys, zs))
    perm = rng.permutation(len(x))
    return x[perm], y[perm], z[perm], rng.integers(0, 1 << 24, len(x)).astype(np.uint32)


def edges_floor():
    """The floor plane for quantile_edges, int32 [48, 48]: INT32_MIN (admits all) except in five cells -- through the middle of
    the cells of 5000, 257 and 129 (their median z), equal to the middle z of the cell of 3 (>= admits it), and above every z of
    the cell of 63 (the cell becomes empty)."""
    cells = _edge_cells()
    floor = np.full((EDGES_GRID[4], EDGES_GRID[3]), INT32_MIN, np.int32)
    for n in (5000, 257, 129):
        cx, cy = POP_CELLS[n]
        floor[cy, cx] = int(np.sort(cells[POP_CELLS[n]])[n // 2])
    cx, cy = POP_CELLS[3]
    floor[cy, cx] = 200
    cx, cy = POP_CELLS[63]
    floor[cy, cx] = int(cells[POP_CELLS[63]].max()) + 1
    return floor


@functools.lru_cache(maxsize=None)
def stream(name: str):
    """The .huffman image of a named stream: those of tests/grid_cases.py and `quantile_edges`."""
    if name == "quantile_edges":
        x, y, z, c = edge_points()
        las = S.las_for((0, 0, int(z.min())), (48000, 48000, int(z.max())))
        return S._keep(P.encode_points(x, y, z, c, las, morton_sort=True, pad_tails=True, nthreads=2)[0])
    return G.stream(name)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def candidates(pts, grid, clip=None, floor=None):
    """(z, cell) of the candidates among the records of a POINT_DTYPE array: grid_cases.cells_of plus the floor test."""
    m, idx = G.cells_of(pts, grid, clip)
    z = pts["z"][m].astype(np.int64)
    if floor is not None:
        keep = z >= np.asarray(floor, np.int64).ravel()[idx]
        z, idx = z[keep], idx[keep]
    return z, idx


def reference(pts, grid, q, clip=None, floor=None):
    """planes int32 [len(q), height, width], counts uint32 [height, width] and the three statistics, over the records of a
    POINT_DTYPE array: the candidates sorted by (cell, z), segment starts from the counts, ranks from the integer formula."""
    w, h = int(grid[3]), int(grid[4])
    z, idx = candidates(pts, grid, clip, floor)
    order = np.lexsort((z, idx))
    z = z[order]
    n = np.bincount(idx, minlength=w * h).astype(np.int64)
    start = np.cumsum(n) - n
    occupied = n > 0
    planes = np.full((len(q), w * h), INT32_MIN, np.int32)
    for j, qj in enumerate(q):
        k = (int(qj) * (n[occupied] - 1) + ONE // 2) // ONE
        planes[j, occupied] = z[start[occupied] + k].astype(np.int32)
    stats = {"candidates": int(n.sum()), "cells_occupied": int(occupied.sum()), "max_cell_points": int(n.max()) if n.size else 0}
    return planes.reshape(len(q), h, w), n.astype(np.uint32).reshape(h, w), stats
