"""The top-down grid, the parts that need no GPU: the four entry points and two structs in the headers, the binding tables and the
cross-compiled library; grid_from_world; the exact division the kernel uses, restated with Python integers; the CLI's refusal
of a malformed --ortho before any device is touched; and the preconditions of tests/test_gpu_grid.py, from the oracle's decoder:
the grids of tests/grid_cases.py put the batches into the classes claimed, and the plateau grid has cells whose top z is held
by more than one record."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import grid_cases as G
from tests import oracle
from tests import select_cases as S
from tests.test_abi import declared

SYMBOLS = ("pcr_grid_clear", "pcr_grid_accumulate", "pcr_grid_unpack", "pcr_read_grid")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    acc = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Grid), C.POINTER(N.Box), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(N.GridStats)]
    assert bound.pcr_grid_accumulate.argtypes == acc and bound.pcr_read_grid.argtypes == acc
    assert bound.pcr_grid_clear.argtypes == [C.c_void_p, C.POINTER(N.Grid), C.c_void_p, C.c_void_p, C.c_void_p]
    assert bound.pcr_grid_unpack.argtypes == [C.c_void_p, C.POINTER(N.Grid), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]


def test_structs_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(pcr_grid), offsetof(pcr_grid, origin_x),\n'
                   'offsetof(pcr_grid, origin_y), offsetof(pcr_grid, cell), offsetof(pcr_grid, width), offsetof(pcr_grid, height), offsetof(pcr_grid, reserved),\n'
                   'sizeof(pcr_grid_stats), offsetof(pcr_grid_stats, batches_outside), offsetof(pcr_grid_stats, batches_windowed),\n'
                   'offsetof(pcr_grid_stats, batches_direct), PCR_GRID_MAX_CELLS, PCR_GRID_WINDOW_CELLS, PCR_GRID_NO_WINDOW, PCR_GRID_TOP, PCR_GRID_BOTTOM);\n'
                   'return 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:7] == [24, 0, 4, 8, 12, 16, 20] and got[7:11] == [24, 0, 8, 16]
    assert [C.sizeof(N.Grid)] + [getattr(N.Grid, f).offset for f, _ in N.Grid._fields_] == got[:7]
    assert [C.sizeof(N.GridStats)] + [getattr(N.GridStats, f).offset for f, _ in N.GridStats._fields_] == got[7:11]
    assert [N.GRID_MAX_CELLS, N.GRID_WINDOW_CELLS, N.GRID_NO_WINDOW, N.GRID_TOP, N.GRID_BOTTOM] == got[11:]
    assert [G.MAX_CELLS, G.WINDOW_CELLS, G.NO_WINDOW] == got[11:14]
    assert (P.GRID_NO_WINDOW, P.GRID_TOP, P.GRID_BOTTOM) == (1, 0, 1)


# ---- the division ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [3, 5, 7, 100, 533, 1000, 4000, 7001, 9973, 65535, 65537, (1 << 24) + 1, (1 << 31) - 1, (1 << 31) - 3])
def test_multiply_high_division_is_exact_for_every_32_bit_dividend(cell):
    """k_grid divides by a cell that is no power of two as (d * ceil(2^64 / cell)) >> 64; pcr_grid_accumulate computes the
    constant as (2^64 - 1) / cell + 1 in 64 bits. A wrong quotient can only appear just below a multiple of the cell or at the
    top of the range, so those dividends are checked exhaustively around every such place that matters, the rest at random."""
    magic = ((1 << 64) - 1) // cell + 1
    assert magic < 1 << 64 and magic == -(-(1 << 64) // cell)
    rng = np.random.default_rng(cell)
    mult = np.unique(np.concatenate([np.arange(0, 64), (1 << 32) // cell - np.arange(0, 64), rng.integers(0, (1 << 32) // cell + 1, 2000)]))
    d = (mult[:, None] * cell + np.array([-2, -1, 0, 1, 2, cell // 2])[None, :]).ravel()
    d = np.concatenate([d, (1 << 32) - 1 - np.arange(0, 1000), rng.integers(0, 1 << 32, 20000)])
    for v in d[(d >= 0) & (d < 1 << 32)]:
        v = int(v)
        assert (v * magic) >> 64 == v // cell, (cell, v)


# ---- grid_from_world ---------------------------------------------------------------------------------------------------------
def las(scale=(0.001, 0.001, 0.001), offset=(0.0, 0.0, 0.0)):
    info = P.LasInfo()
    for k in range(3):
        info.scale[k], info.offset[k] = scale[k], offset[k]
    return info


def test_grid_from_world():
    g = P.grid_from_world(las(), (0.0, 0.0), (1000.0, 500.0), 4.0)
    assert (g.origin_x, g.origin_y, g.cell, g.width, g.height, g.reserved) == (0, 0, 4000, 251, 126, 0)
    g = P.grid_from_world(las(), (0.0, 0.0), (999.999, 499.999), 4.0)
    assert (g.width, g.height) == (250, 125)                                # 999 999 // 4000 + 1
    g = P.grid_from_world(las((0.01, 0.01, 0.5), (100.0, -50.0, 3.0)), (101.005, -49.0), (102.0, -48.0), 0.25)
    assert (g.origin_x, g.origin_y, g.cell) == (101, 100, 25)               # the first lattice point at or above lo
    assert (g.width, g.height) == ((200 - 101) // 25 + 1, (200 - 100) // 25 + 1)
    g = P.grid_from_world(las(), (0.0, 0.0), (1.0, 1.0), 0.001)
    assert g.cell == 1 and g.width == 1001
    # every lattice point of the range has a cell, and no cell lies wholly beyond the range
    for hi in (10.0, 10.001, 10.0039, 10.004):
        g = P.grid_from_world(las(), (2.0, 2.0), (hi, hi), 0.004)
        last = P.box_from_world(las(), (2.0, 2.0, 0.0), (hi, hi, 0.0)).max[0]
        assert (last - g.origin_x) // g.cell == g.width - 1


@pytest.mark.parametrize("scale,cell_size", [((0.001, 0.001, 0.001), 0.0015), ((0.001, 0.001, 0.001), 0.0004), ((0.001, 0.002, 0.001), 0.004),
                                             ((0.003, 0.003, 0.001), 1.0), ((0.001, 0.001, 0.001), 0.0), ((0.001, 0.001, 0.001), -1.0)])
def test_grid_from_world_refuses_a_cell_off_the_lattice(scale, cell_size):
    with pytest.raises(ValueError):
        P.grid_from_world(las(scale), (0.0, 0.0), (10.0, 10.0), cell_size)


def test_grid_from_world_refuses_an_empty_or_oversized_range():
    with pytest.raises(ValueError):
        P.grid_from_world(las(), (5.0, 0.0), (4.0, 10.0), 1.0)
    with pytest.raises(ValueError):
        P.grid_from_world(las(), (0.0, 0.0), (100000.0, 100000.0), 0.001)
    assert tuple(getattr(P.as_grid((1, 2, 3, 4, 5)), f) for f, _ in N.Grid._fields_) == (1, 2, 3, 4, 5, 0)
    with pytest.raises(ValueError):
        P.as_grid((0, 0, 1 << 31, 1, 1))


# ---- the numpy reference against a loop -----------------------------------------------------------------------------------------
def test_reference_planes_against_a_plain_loop():
    rng = np.random.default_rng(9)
    n = 500
    pts = np.zeros(n, P.POINT_DTYPE)
    pts["x"], pts["y"] = rng.integers(-40, 60, n), rng.integers(-40, 60, n)
    pts["z"] = rng.choice([S.INT32_MIN, -1, 0, 1, S.INT32_MAX], n)
    pts["color"] = rng.integers(0, 1 << 24, n)
    grid, clip = (-30, -20, 7, 10, 9), ((-25, -40, -1), (60, 35, S.INT32_MAX))
    top, bottom, count = G.reference(pts, grid, clip)
    wt, wb, wc = {}, {}, {}
    for p in pts:
        x, y, z, c = int(p["x"]), int(p["y"]), int(p["z"]), int(p["color"])
        if x < -30 or y < -20 or (x + 30) // 7 >= 10 or (y + 20) // 7 >= 9 or not (-25 <= x <= 60 and y <= 35 and z >= -1):
            continue
        cell, k = ((y + 20) // 7, (x + 30) // 7), ((z + (1 << 31)) << 32) | c
        wt[cell], wb[cell], wc[cell] = max(wt.get(cell, 0), k), min(wb.get(cell, (1 << 64) - 1), k), wc.get(cell, 0) + 1
    assert len(wc) > 20
    for cy in range(9):
        for cx in range(10):
            assert (int(top[cy, cx]), int(bottom[cy, cx]), int(count[cy, cx])) == (wt.get((cy, cx), 0), wb.get((cy, cx), (1 << 64) - 1), wc.get((cy, cx), 0))
    h, rgba = G.unpack(top, G.EMPTY_TOP)
    cy, cx = next(iter(wt))
    assert int(h[cy, cx]) == (wt[(cy, cx)] >> 32) - (1 << 31) and int(rgba[cy, cx]) == (wt[(cy, cx)] & 0xFFFFFFFF) | 0xFF000000
    assert (h[count == 0] == S.INT32_MIN).all() and (rgba[count == 0] == 0).all()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--ortho"], ["--ortho", "x"], ["--ortho", "0"], ["--ortho", "-1"], ["--ortho", "nan"], ["--ortho", "1", "--dsm"],
                                  ["--ortho", "1", "--box", "0", "0", "0", "1", "1"], ["--ortho", "1", "--dsn", "a.asc"], ["--ortho", "1", "2"],
                                  ["--ortho", "1", "--dsm", "a.asc", "--dsm", "b.asc"]])
def test_cli_refuses_a_malformed_ortho_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.ppm"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--ortho CELL" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grid,want", [c for c in G.CASES if c[2] is not None], ids=lambda v: str(v).replace(" ", ""))
def test_grids_put_the_batches_into_the_classes_claimed(name, grid, want):
    of = oracle.OracleFile(G.stream(name))
    bounds = S.oracle_bounds(of)
    assert G.classify(bounds, grid) == want
    assert G.classify(bounds, grid, flags=G.NO_WINDOW) == want.replace("W", "D")
    # outside means outside, point by point, and a windowed batch's points reach at most WINDOW_CELLS cells (the classes come
    # from the boxes: a batch whose box touches the grid need not have a point in it)
    for b, cls in enumerate(want):
        p = S.oracle_points(of, b).astype(np.int64)
        cx, cy = (p[:, 0] - grid[0]) // grid[2], (p[:, 1] - grid[1]) // grid[2]
        m = (cx >= 0) & (cy >= 0) & (cx < grid[3]) & (cy < grid[4])
        if cls == "O":
            assert not m.any()
        elif cls == "W" and m.any():
            assert (np.ptp(cx[m]) + 1) * (np.ptp(cy[m]) + 1) <= G.WINDOW_CELLS


def test_every_class_and_both_division_paths_occur():
    classes = "".join(c[2] for c in G.CASES if c[2])
    assert all(k in classes for k in "OWD")
    assert any(all(k in c[2] for k in "OWD") for c in G.CASES if c[2]), "no single grid with all three classes"
    cells = {c[1][2] for c in G.CASES if c[1]}
    assert {1, 3, 7001, 9973, 1 << 16, 1 << 24} <= cells
    slab = ((S.INT32_MIN, S.INT32_MIN, 30000), (S.INT32_MAX, S.INT32_MAX, 40000))
    for name, clip, want in (("synth", slab, None), ("synth", S.EMPTY, "O" * 10), ("synth", S.NOTHING, "O" * 10)):
        cls = G.classify(S.oracle_bounds(oracle.OracleFile(G.stream(name))), G.CASES[0][1], clip)
        assert cls == want if want else ("W" in cls or "D" in cls)


def test_plateau_cells_have_ties_for_the_top_z():
    of = oracle.OracleFile(G.stream("plateau"))
    assert of.num_batches == 2
    p = np.concatenate([S.oracle_points(of, b) for b in range(2)]).astype(np.int64)
    ox, oy, cell, w, h = G.PLATEAU_GRID
    cx, cy = (p[:, 0] - ox) // cell, (p[:, 1] - oy) // cell
    m = (p[:, 0] >= ox) & (p[:, 1] >= oy) & (cx < w) & (cy < h)
    idx, z = (cx + cy * w)[m], p[m, 2]
    top = np.full(w * h, S.INT32_MIN, np.int64)
    np.maximum.at(top, idx, z)
    holders = np.bincount(idx[z == top[idx]], minlength=w * h)
    print(f"{(holders >= 2).sum()} of {w * h} cells have a top z held by at least 2 records")
    assert (holders >= 2).sum() >= w * h // 2
