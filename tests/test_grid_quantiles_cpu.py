"""Height percentiles per grid cell, the CPU side: what tests/test_gpu_grid_quantiles.py relies on, proven without a GPU.

The constructed stream `quantile_edges` (tests/quantile_cases.py) is decoded by the oracle and every claim about it is checked on
that decode; the numpy reference is held against a per-cell loop of sorted(); the rank formula against Python integers, in numpy
(P.quantile_rank) and in C++ (csrc/pcr_lattice.h, a stand-alone program under the sanitizers); the CLI's usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import grid_cases as G
from tests import oracle
from tests import quantile_cases as Q
from tests import select_cases as S

PPB = S.PPB
SYMBOLS = ("pcr_grid_quantiles", "pcr_read_grid_quantiles")
LIMITS = [(q, n) for q in (0, 1, 2499, 2500, 4999, 5000, 5001, 9500, 9999, 10000) for n in (1, 2, 3, 4, 64, 65, 10001, (1 << 31) + 1, (1 << 32) - 1)]


def rank(q, n):
    return (q * (n - 1) + 5000) // 10000


def oracle_records(name):
    of = oracle.OracleFile(Q.stream(name))
    xyz = np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)])
    pts = np.zeros(len(xyz), P.POINT_DTYPE)
    for k, n in enumerate(("x", "y", "z")):
        pts[n] = xyz[:, k]
    return pts, S.oracle_bounds(of)


def test_entry_points_constants_and_statistics_match_the_header(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(build.INCLUDE, "pcr_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text) and name in N.HIP_SYMBOLS
    fields = [f for f, _ in N.QuantileStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%d %d %d %zu ", PCR_QUANTILE_ONE, PCR_QUANTILES_MAX, PCR_QUANTILE_MAX_BATCHES, sizeof(pcr_quantile_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_quantile_stats, {f}));\n' for f in fields) + 'printf("%d\\n", PCR_GROUND_EMPTY == INT32_MIN);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:4] == [10000, 8, 65535, 48] and got[4:10] == [getattr(N.QuantileStats, f).offset for f in fields] and got[10] == 1
    assert (P.QUANTILE_ONE, P.QUANTILES_MAX, P.QUANTILE_MAX_BATCHES) == (Q.ONE, Q.QUANTILES_MAX, 65535) == tuple(got[:3])
    assert fields == ["batches_outside", "batches_windowed", "batches_direct", "candidates", "cells_occupied", "max_cell_points"]
    # 65 535 batches hold fewer than 2^32 records: the 32-bit counts and offsets of the kernels cannot wrap
    assert P.QUANTILE_MAX_BATCHES * PPB < 1 << 32 <= (P.QUANTILE_MAX_BATCHES + 1) * PPB


def test_numpy_rank_against_python_integers():
    for q, n in LIMITS:
        got = P.quantile_rank(q, n)
        assert got.dtype == np.uint64 and int(got) == rank(q, n), (q, n)
        assert 0 <= int(got) <= n - 1
    for n in (1, 2, 1000, (1 << 32) - 1):
        assert int(P.quantile_rank(0, n)) == 0 and int(P.quantile_rank(10000, n)) == n - 1
    # broadcast, and the half-way ranks the issue names: n = 2 at q = 5000 takes the upper value, n = 3 at 2500 against 2499
    assert P.quantile_rank([5000, 2500, 2499], [2, 3, 3]).tolist() == [1, 1, 0]
    q, n = np.meshgrid(np.arange(0, 10001, 7), np.arange(1, 300))
    assert np.array_equal(P.quantile_rank(q, n), ((q * (n - 1) + 5000) // 10000).astype(np.uint64))


def test_cxx_rank_at_the_limits_under_the_sanitizers(tmp_path):
    """quantile_rank of csrc/pcr_lattice.h, the function the kernels call, in a stand-alone program of its own."""
    rows = ",\n".join("{%dull, %dull}" % c for c in LIMITS)
    src = tmp_path / "rank.cpp"
    src.write_text('#include <cstdio>\n#include "pcr_lattice.h"\nstruct Case { unsigned long long q, n; };\nstatic const Case cases[] = {\n' + rows +
                   '\n};\nstatic_assert(quantile_rank(5000, 2) == 1 && quantile_rank(2500, 3) == 1 && quantile_rank(2499, 3) == 0, "usable in constant expressions");\n'
                   'static_assert(QUANTILE_ONE == 10000, "basis points");\n'
                   'int main() {\n  for (const Case &c : cases) std::printf("%llu\\n", quantile_rank(c.q, c.n));\n  return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", build.CSRC,
                    str(src), "-o", str(tmp_path / "rank")], check=True)
    res = subprocess.run([str(tmp_path / "rank")], check=True, stdout=subprocess.PIPE, text=True)
    assert [int(v) for v in res.stdout.split()] == [rank(q, n) for q, n in LIMITS]


@pytest.mark.parametrize("grid,clipped,floored", [((40, 40, 7, 9, 6), False, False), ((-20, -13, 5, 12, 11), True, True)])
def test_reference_against_a_plain_loop(grid, clipped, floored):
    rng = np.random.default_rng(grid[2])
    pts = np.zeros(4000, P.POINT_DTYPE)
    pts["x"], pts["y"] = rng.integers(-30, 70, 4000), rng.integers(-30, 70, 4000)
    pts["z"] = rng.integers(-5, 6, 4000) * rng.choice([1, 1 << 24, 100003], 4000)    # repeats, both signs, every byte
    w, h = grid[3], grid[4]
    clip = ((-10, -25, -(1 << 25)), (44, 40, 1 << 26)) if clipped else None
    floor = rng.choice([S.INT32_MIN, -300000, 0, 1 << 24, S.INT32_MAX], (h, w)).astype(np.int32) if floored else None
    planes, counts, st = Q.reference(pts, grid, Q.Q8, clip, floor)
    per_cell = [[] for _ in range(w * h)]
    for x, y, z in zip(pts["x"].tolist(), pts["y"].tolist(), pts["z"].tolist()):
        cx, cy = (x - grid[0]) // grid[2], (y - grid[1]) // grid[2]
        if not (0 <= cx < w and 0 <= cy < h):
            continue
        if clip is not None and not all(lo <= v <= hi for v, lo, hi in zip((x, y, z), *clip)):
            continue
        if floor is not None and z < int(floor[cy, cx]):
            continue
        per_cell[cy * w + cx].append(z)
    assert planes.dtype == np.int32 and planes.shape == (8, h, w) and counts.dtype == np.uint32 and counts.shape == (h, w)
    for c, zs in enumerate(per_cell):
        zs = sorted(zs)
        assert counts.ravel()[c] == len(zs)
        for j, q in enumerate(Q.Q8):
            assert planes[j].ravel()[c] == (zs[rank(q, len(zs))] if zs else S.INT32_MIN)
    sizes = [len(z) for z in per_cell]
    assert st == {"candidates": sum(sizes), "cells_occupied": sum(1 for s in sizes if s), "max_cell_points": max(sizes)}
    assert 0 < st["cells_occupied"] and 0 in sizes and max(sizes) > 1


def test_quantile_edges_decodes_to_its_cells():
    """Every claim of tests/quantile_cases.py about the constructed stream, from the oracle's decode of it."""
    pts, bounds = oracle_records("quantile_edges")
    grid = Q.EDGES_GRID
    assert len(pts) == 2 * PPB and G.classify(bounds, grid) == "WW" and G.classify(bounds, grid, flags=G.NO_WINDOW) == "DD"
    z, idx = Q.candidates(pts, grid)
    assert len(z) == 2 * PPB                                                # no record falls outside the grid
    cell_z = lambda cell: np.sort(z[idx == Q.cell_index(cell)])
    # the populations, in the cells claimed: the small/large edge (64 | 65) and the tile edges of both select kernels
    assert Q.POPULATIONS == (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 5000) and Q.SMALL_MAX == 64
    for n, cell in Q.POP_CELLS.items():
        assert len(cell_z(cell)) == n, (n, cell)
    # a large cell whose values are all equal; one where only the lowest byte differs; one where only the highest does, with both signs
    eq, low, high = cell_z(Q.CELL_EQUAL), cell_z(Q.CELL_LOW_BYTE), cell_z(Q.CELL_HIGH_BYTE)
    assert len(eq) == len(low) == len(high) == Q.SPECIAL_N > Q.SMALL_MAX
    assert (eq == eq[0]).all()
    assert len(set((low >> 8).tolist())) == 1 and len(set((low & 255).tolist())) > 100
    assert len(set((high & 0xFFFFFF).tolist())) == 1 and len(set((high >> 24).tolist())) > 50 and high[0] < 0 < high[-1]
    # a cell whose z repeat: for q = 2500 the k-th and the (k + 1)-th value are equal, for q = 5000 the k-th differs from the one before
    rep = cell_z(Q.CELL_REPEAT)
    k25, k50 = rank(2500, len(rep)), rank(5000, len(rep))
    assert len(rep) == 101 and rep[k25] == rep[k25 + 1] == Q.REPEAT_LOW[0] and rep[k50 - 1] == Q.REPEAT_LOW[0] != rep[k50] == Q.REPEAT_HIGH[0]
    # the half-way ranks
    assert cell_z(Q.POP_CELLS[2]).tolist() == [100, 200] and rank(5000, 2) == 1
    assert cell_z(Q.POP_CELLS[3]).tolist() == [100, 200, 300] and (rank(2500, 3), rank(2499, 3)) == (1, 0)
    # cells fed by both batches (two workgroups reserve in one segment), large ones and small ones
    first, second = np.bincount(idx[:PPB], minlength=48 * 48), np.bincount(Q.candidates(pts[PPB:], grid)[1], minlength=48 * 48)
    shared = (first > 0) & (second > 0)
    assert (shared & (first + second > Q.SMALL_MAX)).sum() >= 10 and (shared & (first + second <= Q.SMALL_MAX)).sum() >= 1
    # the floor plane: through the middle of three cells, equal to a z in one, above every z in another, INT32_MIN elsewhere
    floor = Q.edges_floor()
    _, counts, _ = Q.reference(pts, grid, Q.Q8)
    planes_f, counts_f, st_f = Q.reference(pts, grid, Q.Q8, floor=floor)
    at = lambda n: (Q.POP_CELLS[n][1], Q.POP_CELLS[n][0])
    assert (floor != S.INT32_MIN).sum() == 5
    for n in (5000, 257, 129):
        assert n // 4 < counts_f[at(n)] < 3 * n // 4 + 2 and counts[at(n)] == n
    assert counts_f[at(3)] == 2 and floor[at(3)] == 200 and planes_f[0][at(3)] == 200          # >= admits the z the floor equals
    assert counts_f[at(63)] == 0 and counts[at(63)] == 63 and (planes_f[:, at(63)[0], at(63)[1]] == S.INT32_MIN).all()
    untouched = floor == S.INT32_MIN
    assert np.array_equal(counts_f[untouched], counts[untouched]) and st_f["max_cell_points"] < 5000


def test_the_cases_hold_candidates_in_small_and_large_cells():
    """The streams of tests/grid_cases.py give both select kernels work: cells of at most 64 candidates and larger ones."""
    small = large = 0
    for name, grid, _ in (G.CASES[0], G.CASES[1], G.CASES[5]):
        pts, _ = oracle_records(name)
        _, counts, st = Q.reference(pts, grid, Q.Q8)
        if grid == G.CASES[5][1]:                                           # both sides of the lane-per-cell edge (4 | 5 candidates)
            assert all((counts == n).sum() > 0 for n in (1, 2, 3, 4, 5, 6))
        small += int(((counts > 0) & (counts <= Q.SMALL_MAX)).sum()); large += int((counts > Q.SMALL_MAX).sum())
        assert st["candidates"] == int(counts.sum()) > 0
    assert small > 0 and large > 0


@pytest.mark.parametrize("args", [["--percentile", "95", "1", "--ortho", "1"], ["--percentile", "95", "1", "--dtm", "1"], ["--percentile", "95", "1", "--thin", "1"],
                                  ["--percentile", "95", "1", "--dsm", "x.asc"], ["--ortho", "1", "--percentile", "95", "1"],
                                  ["--thin", "1", "--percentile", "95", "1"], ["--dtm", "1", "--percentile", "95", "1"],
                                  ["--percentile", "95"], ["--percentile", "101", "1"], ["--percentile", "-1", "1"], ["--percentile", "33.333", "1"],
                                  ["--percentile", "95", "0"], ["--percentile", "p95", "1"], ["--percentile", "95", "1", "--box", "0", "0", "0", "1", "1"],
                                  ["--percentile", "95", "1", "--percentile", "50", "1"]])
def test_cli_refuses_percentile_with_another_mode_or_malformed_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.asc"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--percentile" in res.stderr and not out.exists()


def test_python_argument_checks_need_no_gpu():
    assert P.as_quantiles((0, 9500, 10000)).dtype == np.uint32 and P.as_quantiles(5000).tolist() == [5000]
    for bad in ((0.5,), (-1,), (1 << 32,), ((1, 2), (3, 4))):
        with pytest.raises(ValueError):
            P.as_quantiles(bad)
    assert C.sizeof(N.QuantileStats) == 48
