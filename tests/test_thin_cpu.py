"""Voxel thinning, the parts that need no GPU: the two entry points and two structs in the headers, the binding tables and the
cross-compiled library; the lattice arithmetic of csrc/pcr_lattice.h, compiled into a stand-alone program and held against
Python integers; voxels_from_world; the numpy reference of tests/thin_cases.py against a plain loop; the CLI's refusal of a
malformed --thin before any device is touched; and the preconditions of tests/test_gpu_thin.py, from the oracle's decoder.

The preconditions, as the oracle's decode gave them when the cases were chosen (stream, cell, origin, clip: counts):
  synth 7001 (0,0,0) none:               multi_batch 1094, multi_chain 23252, long_runs 115590, reentered 54766
  synth 2048 (-12345,777,-1) none:       multi_batch 1456, multi_chain 42951, long_runs 156802, reentered 102974, center_differs 113276, d2_ties 15
  clustered 1000 (0,0,0) none:           multi_batch 552, multi_chain 11827, long_runs 60113, reentered 31775, center_differs 13697
  garbage_tail 7001 (0,0,0) header box:  multi_batch 573, multi_chain 24934, long_runs 83200, reentered 749
  garbage_tail 2048 (MAX,MIN,0) header:  multi_chain 25445, long_runs 25214, reentered 4, center_differs 23601, d2_ties 6
  plateau 64 (0,0,0) none:               multi_chain 128, long_runs 7858, center_differs 3990, d2_ties 16
  wide30 2 (0,0,0) x in 0..2:            multi_batch 11651, multi_chain 13199, reentered 22, d2_ties 18539
  wide30 1 (-12345,777,-1) x in 0..2:    multi_batch 3230, multi_chain 3243, reentered 4, d2_ties 6148
(a Morton-sorted chain leaves a voxel and comes back more often than not: `reentered` is not special to the unsorted stream.)"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared

SYMBOLS = ("pcr_thin", "pcr_read_thin")


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Voxels), C.POINTER(N.Box), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.ThinStats)]
    assert bound.pcr_thin.argtypes == args and bound.pcr_read_thin.argtypes == args


def test_structs_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirrors."""
    stats = [f for f, _ in N.ThinStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu ", sizeof(pcr_voxels), offsetof(pcr_voxels, origin), offsetof(pcr_voxels, cell), sizeof(pcr_thin_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_thin_stats, {f}));\n' for f in stats)
                   + 'printf("%d %d %d %d\\n", PCR_THIN_FIRST, PCR_THIN_CENTER, PCR_THIN_MAX_CELL, PCR_THIN_MAX_CENTER_CELL);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got[:4] == [16, 0, 12, 48] and got[4:10] == [0, 8, 16, 24, 32, 40]
    assert [C.sizeof(N.Voxels), N.Voxels.origin.offset, N.Voxels.cell.offset, C.sizeof(N.ThinStats)] == got[:4]
    assert [getattr(N.ThinStats, f).offset for f in stats] == got[4:10]
    assert stats == ["batches_outside", "batches_decoded", "points_considered", "runs", "points_kept", "table_slots"]
    assert [N.THIN_FIRST, N.THIN_CENTER, N.THIN_MAX_CELL, N.THIN_MAX_CENTER_CELL] == got[10:]
    assert [T.FIRST, T.CENTER, T.MAX_CELL, T.MAX_CENTER_CELL] == got[10:]
    assert (P.THIN_FIRST, P.THIN_CENTER) == (0, 1)


# ---- the lattice (csrc/pcr_lattice.h) in a program of its own ------------------------------------------------------------------
I32 = (S.INT32_MIN, S.INT32_MAX)
LATTICE_CASES = [
    # origin, cell, q.min, q.max
    ((0, 0, 0), 1, (0, 0, 0), (10, 10, 10)),
    ((0, 0, 0), 1, (-5, 3, 0), ((1 << 21) - 3, 3, 0)),                      # (2^21 - 3 + 5) / 1 + 2 = 2^21 + 4: too many voxels
    ((0, 0, 0), 1, (-5, 3, 0), ((1 << 21) - 7, 3, 0)),                      # exactly 2^21
    ((0, 0, 0), 1, (-5, 3, 0), ((1 << 21) - 6, 3, 0)),                      # one more
    ((-12345, 777, -1), 7001, (-1048562, -1048564, -67759), (1048571, 1048556, 68709)),
    ((I32[1], I32[0], 0), 64, (593, 593, 241), (999406, 999406, 74106)),    # origin' beyond int32 on x and y
    ((I32[1], I32[0], 0), 1 << 30, (I32[0], 0, 0), (-2, 5, 5)),
    ((I32[0], I32[1], 5), 1 << 30, (I32[0], I32[0], I32[0]), (I32[1] - 1, -1, 0)),
    ((0, 0, 0), 1 << 30, (I32[0], 0, 0), (I32[1], 0, 0)),                   # extent 2^32 - 1
    ((0, 0, 0), 1 << 30, (0, I32[0], 0), (0, 0, 0)),                        # extent 2^31 exactly: refused
    ((0, 0, 0), 1 << 30, (0, 0, I32[0] + 1), (0, 0, 0)),                    # extent 2^31 - 1: accepted
    ((5, -5, 17), 2047, (-100000, -100000, -100000), (100000, 100000, 100000)),
    ((5, -5, 17), 2048, (3, -5, 18), (3, -5, 18)),
    ((7, 7, 7), 1000, (0, 0, 0), (1073741826, 1999, 49)),
]


def lattice_by_hand(origin, cell, qmin, qmax):
    out = []
    for k in range(3):
        extent = qmax[k] - qmin[k]
        if extent >= 1 << 31:
            return [1, k]
        if extent // cell + 2 > 1 << 21:
            return [2, k]
        shifted = origin[k] + (qmin[k] - origin[k]) // cell * cell          # Python's // is the floor
        assert shifted <= qmin[k] < shifted + cell and qmax[k] - shifted < (1 << 31) + (1 << 30)
        assert (qmax[k] - shifted) // cell < 1 << 21
        out.append(shifted % (1 << 32))
    pow2 = cell & (cell - 1) == 0
    return [0, 2] + out + [cell, cell.bit_length() - 1 if pow2 else 32, 0 if pow2 else -(-(1 << 64) // cell)]


def test_lattice_shift_limits_and_divisor_against_python_integers(tmp_path):
    """thin_lattice() for origins and boxes at the edges of int32: the refusals, the shifted origin modulo 2^32 and the divisor."""
    rows = ",\n".join("{{%d, %d, %d}, %d, {%d, %d, %d}, {%d, %d, %d}}" % (*o, c, *lo, *hi) for o, c, lo, hi in LATTICE_CASES)
    rows = rows.replace("-2147483648", "(-2147483647 - 1)")
    src = tmp_path / "lattice.cpp"
    src.write_text('#include <cstdio>\n#include "pcr_lattice.h"\nstruct Case { int32_t origin[3]; int32_t cell; int32_t lo[3], hi[3]; };\n'
                   'static const Case cases[] = {\n' + rows + '\n};\nint main() {\n  for (const Case &c : cases) {\n    ThinLattice l{}; int axis = -1;\n'
                   '    const int rc = thin_lattice(c.origin, c.cell, c.lo, c.hi, &l, &axis);\n'
                   '    if (rc) std::printf("%d %d\\n", rc, axis);\n'
                   '    else std::printf("0 %d %u %u %u %u %u %llu\\n", axis, l.origin[0], l.origin[1], l.origin[2], l.cell, l.div.shift, l.div.magic);\n'
                   '  }\n  return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", build.CSRC,
                    str(src), "-o", str(tmp_path / "lattice")], check=True)
    res = subprocess.run([str(tmp_path / "lattice")], check=True, stdout=subprocess.PIPE, text=True)
    got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    want = [lattice_by_hand(*case) for case in LATTICE_CASES]
    assert got == want
    assert sorted({w[0] for w in want}) == [0, 1, 2], "the cases reach both refusals and the accepted path"


@pytest.mark.parametrize("cell", [1000, 7001, 2047, 3, (1 << 30) - 1])
def test_the_cells_of_the_cases_divide_exactly(cell):
    """d / cell by multiply-high for the largest d a thinning call can see, d < 2^31 + 2^30 (test_grid_cpu.py has the full range)."""
    magic = ((1 << 64) - 1) // cell + 1
    top = (1 << 31) + (1 << 30)
    rng = np.random.default_rng(cell)
    mult = np.unique(np.concatenate([np.arange(0, 32), top // cell - np.arange(0, 32), rng.integers(0, top // cell + 1, 500)]))
    d = (mult[:, None] * cell + np.array([-1, 0, 1, cell - 1])[None, :]).ravel()
    for v in d[(d >= 0) & (d < top)]:
        assert (int(v) * magic) >> 64 == int(v) // cell, (cell, int(v))


# ---- voxels_from_world -------------------------------------------------------------------------------------------------------
def las(scale=(0.001, 0.001, 0.001), offset=(0.0, 0.0, 0.0), lo=(0.0, 0.0, 0.0), hi=(1000.0, 1000.0, 100.0)):
    info = P.LasInfo()
    for k in range(3):
        info.scale[k], info.offset[k], info.min[k], info.max[k] = scale[k], offset[k], lo[k], hi[k]
    return info


def fields(v):
    return tuple(v.origin) + (v.cell,)


def test_voxels_from_world():
    assert fields(P.voxels_from_world(las(), 0.5)) == (0, 0, 0, 500)
    assert fields(P.voxels_from_world(las(lo=(1.0005, -2.0, 3.0)), 0.001)) == (1001, -2000, 3000, 1)     # the first lattice point at or above
    assert fields(P.voxels_from_world(las((0.01, 0.01, 0.01), (100.0, -50.0, 3.0)), 0.25, origin=(101.005, -49.0, 3.0))) == (101, 100, 0, 25)
    assert fields(P.voxels_from_world(las(), 1073741.824)) == (0, 0, 0, 1 << 30)
    assert fields(P.as_voxels((1, -2, 3, 4))) == (1, -2, 3, 4) and fields(P.as_voxels(P.as_voxels((1, -2, 3, 4)))) == (1, -2, 3, 4)
    with pytest.raises(ValueError):
        P.as_voxels((0, 0, 1 << 31, 1))


@pytest.mark.parametrize("scale,cell_size", [((0.001, 0.001, 0.001), 0.0015), ((0.001, 0.001, 0.001), 0.0004), ((0.001, 0.001, 0.002), 0.004),
                                             ((0.001, 0.002, 0.001), 0.004), ((0.003, 0.003, 0.003), 1.0), ((0.001, 0.001, 0.001), 0.0),
                                             ((0.001, 0.001, 0.001), -1.0), ((0.001, 0.001, 0.001), 1073741.825)])
def test_voxels_from_world_refuses_a_cell_off_the_lattice(scale, cell_size):
    with pytest.raises(ValueError):
        P.voxels_from_world(las(scale), cell_size)


def test_voxels_from_world_refuses_an_origin_beyond_int32():
    with pytest.raises(ValueError):
        P.voxels_from_world(las(), 1.0, origin=(0.0, 1e10, 0.0))


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [T.FIRST, T.CENTER])
@pytest.mark.parametrize("vox", [(0, 0, 0, 1), (-3, 5, 1, 4), (S.INT32_MAX, S.INT32_MIN, 0, 7), (2, 2, 2, 6)])
def test_reference_against_a_plain_loop(vox, mode):
    rng = np.random.default_rng(sum(vox) & 0xFFFF)
    xyz = rng.integers(-20, 21, (3000, 3))
    xyz[::7] = xyz[1::7][:len(xyz[::7])]                                    # exact duplicates
    clip = ((-15, -20, -18), (20, 12, 20))
    best = {}
    for row, p in enumerate(xyz):
        p = [int(v) for v in p]
        if not all(clip[0][k] <= p[k] <= clip[1][k] for k in range(3)):
            continue
        v = tuple((p[k] - vox[k]) // vox[3] for k in range(3))
        d2 = sum((2 * (p[k] - vox[k] - v[k] * vox[3]) - (vox[3] - 1)) ** 2 for k in range(3))
        cand = (d2, row) if mode == T.CENTER else (row,)
        if v not in best or cand < best[v]:
            best[v] = cand
    want = sorted(c[-1] for c in best.values())
    got = T.reference(xyz, vox, clip, mode)
    assert got.dtype == np.int64 and got.tolist() == want and len(want) > 50


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(T.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


@pytest.mark.parametrize("name,cell,origin,clip,needs", T.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cases_show_the_properties_claimed(name, cell, origin, clip, needs):
    xyz, bounds = oracle_rows(name)
    vox, clip = (*origin, cell), T.case_clip(name, clip, xyz)
    assert T.lattice_refusal(bounds, vox, clip) is None
    got = T.properties(xyz, vox, clip)
    print(f"{name} cell {cell} origin {origin} clip {clip}: {got}, runs {T.count_runs(xyz, vox, clip)} of {int(T.candidates(xyz, clip).sum())} candidates")
    for k in needs:
        assert got[k] >= 1, f"{k}: no such voxel / run in this case"
    # the reference keeps one row per voxel, in increasing order, in both modes
    modes = (T.FIRST, T.CENTER) if cell <= T.MAX_CENTER_CELL else (T.FIRST,)
    for mode in modes:
        rows = T.reference(xyz, vox, clip, mode)
        assert (np.diff(rows) > 0).all() and T.candidates(xyz, clip)[rows].all()
        key, _ = T.voxel_keys(xyz[rows], vox)
        assert len(np.unique(key)) == len(rows) == len(np.unique(T.voxel_keys(xyz[T.candidates(xyz, clip)], vox)[0]))


def test_every_property_cell_path_and_origin_is_covered():
    assert set(T.PROPERTIES) == {k for c in T.CASES for k in c[4]}
    assert any(c[0] == "garbage_tail" and "reentered" in c[4] for c in T.CASES)
    assert {1, 64, 1 << 20, 1000, 7001, 2047, 2048, T.MAX_CELL} == {c[0] for c in T.COMBOS}
    assert {0, 1, 2} == {c[1] for c in T.COMBOS} and {T.FIRST, T.CENTER} == {c[2] for c in T.COMBOS} and {False, True} == {c[3] for c in T.COMBOS}
    assert all(c[2] == T.FIRST or c[0] <= T.MAX_CENTER_CELL for c in T.COMBOS)
    assert T.ORIGINS == [(0, 0, 0), (-12345, 777, -1), (S.INT32_MAX, S.INT32_MIN, 0)]


def test_lattice_limits_of_the_streams():
    """What tests/test_gpu_thin.py expects of the calls without a clip: wide30's two clusters are 2^30 apart and its tail
    artefact reaches below -2^30 (refused at any cell, cell 1 by the voxel limit on x); garbage_tail's artefact stays within
    a few thousand steps of the cloud, so the call without a clip is accepted."""
    _, wide = oracle_rows("wide30")
    assert T.lattice_refusal(wide, (0, 0, 0, 1)) == "voxels"
    assert T.lattice_refusal(wide, (0, 0, 0, 1 << 20)) == "extent" and T.lattice_refusal(wide, (0, 0, 0, 1), T.WIDE30_LOW) is None
    xyz, tail = oracle_rows("garbage_tail")
    span = tail[:, 3:].max(axis=0).astype(np.int64) - tail[:, :3].min(axis=0)
    print(f"garbage_tail spans {span.tolist()} without a clip; {int((~S.in_box(xyz, T.header_clip('garbage_tail'))).sum())} rows lie outside the header's box")
    assert T.lattice_refusal(tail, (0, 0, 0, 1)) == T.GARBAGE_TAIL_UNCLIPPED is None
    assert (~S.in_box(xyz, T.header_clip("garbage_tail"))).sum() >= 1
    for name in T.STREAMS:
        if name not in ("wide30",):
            assert T.lattice_refusal(oracle_rows(name)[1], (0, 0, 0, 1)) is None


def test_table_slots():
    assert [T.table_slots(r) for r in (0, 1, 512, 513, 1 << 20, (1 << 20) + 1)] == [0, 1024, 1024, 2048, 1 << 21, 1 << 22]


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--thin"], ["--thin", "x"], ["--thin", "0"], ["--thin", "-1"], ["--thin", "nan"], ["--thin", "1", "--centre"],
                                  ["--thin", "1", "--box", "0", "0", "0", "1", "1"], ["--thin", "1", "2"], ["--thin", "1", "--center", "--center"],
                                  ["--thin", "1", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_a_malformed_thin_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--thin CELL" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
