"""The ground filter and the height selection, the parts that need no GPU: the four entry points and three structs in the headers,
the binding tables and the cross-compiled library; ground_params_from_world; the numpy reference of tests/ground_cases.py held
against a per-cell double loop; and the preconditions of tests/test_gpu_ground.py, from the oracle's decoder: the `town` stream
has empty cells, cells every step of the filter flags, holes the fill needs several rounds for, and records in every height
range."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import ground_cases as GC
from tests import oracle
from tests import select_cases as S
from tests.test_abi import declared

SYMBOLS = ("pcr_ground_filter", "pcr_read_ground", "pcr_select_height", "pcr_read_height")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    assert bound.pcr_ground_filter.argtypes == [C.c_void_p, C.POINTER(N.Grid), C.POINTER(N.GroundParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(N.GroundStats)]
    sel = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Grid), C.c_void_p, C.POINTER(N.Box), C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
           C.c_size_t, C.POINTER(C.c_int64), C.POINTER(N.HeightStats)]
    assert bound.pcr_select_height.argtypes == sel and bound.pcr_read_height.argtypes == sel


def test_structs_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %lld %d %d %d %d\\n", sizeof(pcr_ground_params), sizeof(pcr_ground_stats),\n'
                   'sizeof(pcr_height_stats), offsetof(pcr_ground_params, fill_rounds), offsetof(pcr_ground_params, radius),\n'
                   'offsetof(pcr_ground_params, threshold), offsetof(pcr_ground_stats, fill_rounds), offsetof(pcr_height_stats, points_selected),\n'
                   'PCR_GROUND_MAX_STEPS, PCR_GROUND_MAX_RADIUS, PCR_GROUND_MAX_FILL, (long long)PCR_GROUND_EMPTY, PCR_CELL_EMPTY, PCR_CELL_GROUND,\n'
                   'PCR_CELL_NONGROUND, PCR_HEIGHT_REPLACE_Z);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:3] == [136, 48, 32]
    assert [C.sizeof(N.GroundParams), C.sizeof(N.GroundStats), C.sizeof(N.HeightStats)] == got[:3]
    assert [N.GroundParams.fill_rounds.offset, N.GroundParams.radius.offset, N.GroundParams.threshold.offset, N.GroundStats.fill_rounds.offset,
            N.HeightStats.points_selected.offset] == got[3:8] == [4, 8, 72, 40, 24]
    assert [N.GROUND_MAX_STEPS, N.GROUND_MAX_RADIUS, N.GROUND_MAX_FILL, N.GROUND_EMPTY, N.CELL_EMPTY, N.CELL_GROUND, N.CELL_NONGROUND, N.HEIGHT_REPLACE_Z] == got[8:]
    assert [GC.MAX_STEPS, GC.MAX_RADIUS, GC.MAX_FILL, GC.EMPTY, GC.CELL_EMPTY, GC.CELL_GROUND, GC.CELL_NONGROUND, GC.REPLACE_Z] == got[8:]
    assert (P.GROUND_EMPTY, P.CELL_EMPTY, P.CELL_GROUND, P.CELL_NONGROUND, P.HEIGHT_REPLACE_Z) == (-(1 << 31), 0, 1, 2, 1)


# ---- the parameters -------------------------------------------------------------------------------------------------------------
def las(scale_z=0.01):
    info = P.LasInfo()
    for k in range(3):
        info.scale[k], info.offset[k] = (0.01, 0.01, scale_z)[k], 0.0
    return info


def test_ground_params_from_world_check_figure():
    gp = P.ground_params_from_world(las(), 1.0, slope=0.15)
    assert gp.radii == (1, 2, 4, 8, 16) and gp.thresholds == (15, 45, 75, 135, 250)
    assert (gp.num_steps, gp.fill_rounds) == (5, 4096) and tuple(gp.radius[5:]) == (0,) * 11 and tuple(gp.threshold[5:]) == (0,) * 11


def test_ground_params_limits():
    gp = P.ground_params_from_world(las(), 100.0)                               # a window of 3 cells is already past max_window: one step all the same
    assert gp.radii == (1,) and gp.thresholds == (15,)
    gp = P.ground_params_from_world(las(), 0.5, max_window=1e9, fill_rounds=7)
    assert gp.radii == (1, 2, 4, 8, 16, 32, 64) and gp.fill_rounds == 7         # r <= 64
    assert all(t >= 0 for t in gp.thresholds) and gp.thresholds[-1] == 250      # max_distance caps the rest
    with pytest.raises(ValueError):
        P.ground_params_from_world(las(0.0), 1.0)
    with pytest.raises(ValueError):
        P.GroundParams((1, 2), (3,))
    gp = P.GroundParams((1, 3), (5, 7), 9)
    assert (gp.num_steps, gp.fill_rounds, gp.radii, gp.thresholds) == (2, 9, (1, 3), (5, 7))
    assert P.GroundParams(range(1, 18), range(17)).num_steps == 17              # kept for the native call to refuse


# ---- the numpy reference against a loop -----------------------------------------------------------------------------------------
def brute_opening(a, r):
    """E and O of one step by the definition, cell by cell, with Python integers and None for "none"."""
    h, w = len(a), len(a[0])

    def over(src, pick):
        out = [[None] * w for _ in range(h)]
        for cy in range(h):
            for cx in range(w):
                vals = [src[y][x] for y in range(max(0, cy - r), min(h, cy + r + 1)) for x in range(max(0, cx - r), min(w, cx + r + 1))
                        if src[y][x] is not None]
                out[cy][cx] = pick(vals) if vals else None
        return out
    e = over(a, min)
    return e, over(e, max)


@pytest.mark.parametrize("r", [1, 2, 5, 30])
def test_reference_opening_against_a_plain_loop(r):
    rng = np.random.default_rng(23 + r)
    z = rng.integers(-1000, 1000, (23, 17)).astype(np.int64)
    z[rng.random((23, 17)) < 0.35] = GC.EMPTY
    z[3, 4], z[20, 2], z[11, 11] = GC.INT32_MAX, GC.INT32_MIN + 1, GC.INT32_MAX
    z[0:9, 9:17] = GC.EMPTY                                                     # a hole wider than the small windows
    z[4, 13] = -7
    e, o = GC.opening(z, z != GC.EMPTY, r)
    be, bo = brute_opening([[None if v == GC.EMPTY else int(v) for v in row] for row in z], r)
    none = lambda p: [[GC.EMPTY if v is None else v for v in row] for row in p]
    assert e.tolist() == none(be) and o.tolist() == none(bo)
    assert (e == GC.EMPTY).any() == (r < 5)


def test_reference_fill_floors_and_counts():
    h = np.full((3, 4), GC.EMPTY, np.int64)
    h[0, 0], h[0, 1] = -3, -4                                                   # sum -7 over 2: floor is -4, truncation would say -3
    out, filled = GC.fill_round(h)
    assert out[1, 0] == -4 and out[1, 1] == -4 and out[1, 2] == -4 and out[0, 2] == -4 and filled == 4
    assert (out[:, 3] == GC.EMPTY).all() and (out[2] == GC.EMPTY).all()
    g, cls, st = GC.ground_filter(h.astype(np.int32), (), (), fill_rounds=1)
    assert st == dict(cells_empty=10, cells_ground=2, cells_nonground=0, cells_filled=4, cells_unfilled=6, fill_rounds=1)
    g, cls, st = GC.ground_filter(h.astype(np.int32), (), ())
    assert st["cells_unfilled"] == 0 and st["fill_rounds"] == 2 and (cls == np.where(h == GC.EMPTY, 0, 1)).all()


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def town():
    """The oracle's decode of the encoded `town` stream as a POINT_DTYPE array (colours zero: nothing here reads them)."""
    of = oracle.OracleFile(GC.stream("town"))
    assert of.num_batches == 2
    xyz = np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)])
    pts = np.zeros(len(xyz), P.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return pts


def raw_town():
    x, y, z, _ = GC.town_points()
    raw = np.zeros(len(x), P.POINT_DTYPE)
    raw["x"], raw["y"], raw["z"] = x, y, z
    return raw


def test_town_first_grid_has_what_the_gpu_tests_need(town):
    """The conditions hold for the records of the encoded stream, the prototype's figures for the points it was made from.
    The two differ by more than padding duplicates: 296 of the stream's 131 072 records are the tail artefact of the
    reference's interleave, some far below the terrain, so the stream's lowest-point grid has outliers
    the input has not and the filter flags their neighbourhoods (1122 cells in steps of 40 / 57 / 286 / 739, 6 fill rounds,
    against the input's 166 in 13 / 35 / 28 / 90 and 5). The GPU tests compare with numpy over read_points of the stream,
    artefact included, so only the conditions matter to them."""
    grid, radii, thresholds = GC.TOWN[0]
    want = GC.TOWN_FIGURES[0]
    steps = []
    ground, cls, st = GC.ground_filter(GC.lowest(town, grid), radii, thresholds, steps_out=steps)
    print(f"town {grid}, the stream's records: {st}, new per step {steps}")
    assert st["cells_empty"] >= 40 and all(s >= 1 for s in steps)
    assert st["fill_rounds"] >= 4 and st["cells_unfilled"] == 0
    for lo, hi in GC.HEIGHT_RANGES:
        got = len(GC.select_height(town, grid, ground, lo, hi)[0])
        print(f"h in [{lo}, {hi}]: {got} records of the stream")
        assert got >= 1000
    # the figures of the prototype, over the points before encoding
    raw = raw_town()
    steps = []
    ground, cls, st = GC.ground_filter(GC.lowest(raw, grid), radii, thresholds, steps_out=steps)
    print(f"town {grid}, the input points: {st}, new per step {steps}")
    assert st["cells_empty"] == want["empty"] and st["cells_nonground"] == want["flagged"] and tuple(steps) == want["per_step"]
    assert st["fill_rounds"] == want["rounds"] and st["cells_unfilled"] == want["unfilled"]
    assert GC.heights(raw, grid, ground)[0].sum() == want["covered"]
    for (lo, hi), n in zip(GC.HEIGHT_RANGES, GC.TOWN_RECORDS):
        assert len(GC.select_height(raw, grid, ground, lo, hi)[0]) == n


@pytest.mark.parametrize("case", [1, 2])
def test_town_other_grids(town, case):
    grid, radii, thresholds = GC.TOWN[case]
    want = GC.TOWN_FIGURES[case]
    raw = raw_town()
    ground, cls, st = GC.ground_filter(GC.lowest(raw, grid), radii, thresholds)
    print(f"town {grid}, the input points: {st}")
    assert st["cells_nonground"] == want["flagged"] and st["fill_rounds"] == want["rounds"]
    assert "empty" not in want or st["cells_empty"] == want["empty"]
    if "covered" in want:
        assert GC.heights(raw, grid, ground)[0].sum() == want["covered"]
        bounds = S.oracle_bounds(oracle.OracleFile(GC.stream("town")))
        lo, hi = np.array(grid[:2]), np.array(grid[:2]) + grid[2] * np.array(grid[3:]) - 1
        assert ((bounds[:, :2] < lo) | (bounds[:, 3:5] > hi)).any(), "no batch reaches beyond the grid"
    # the stream's records: something of every class, and a fill that takes more than one round
    ground, cls, st = GC.ground_filter(GC.lowest(town, grid), radii, thresholds)
    print(f"town {grid}, the stream's records: {st}")
    assert st["cells_ground"] > 0 and st["cells_nonground"] > 0 and st["fill_rounds"] >= 2
