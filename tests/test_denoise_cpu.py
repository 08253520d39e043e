"""Voxel denoising, the parts that need no GPU: the two entry points and the struct in the headers, the binding tables and the
cross-compiled library; noise_lattice() of csrc/pcr_lattice.h, compiled into a stand-alone program and held against Python
integers; the numpy reference of tests/denoise_cases.py against a plain loop; the CLI's refusal of a malformed --denoise before
any device is touched; and the preconditions of tests/test_gpu_denoise.py, from the oracle's decoder.

The preconditions, as the oracle's decode gave them when the cases were chosen, origin (0, 0, 0)
(stream cell max_count clip: isolated / candidates, neighbour_decides, other_batch_decides):
  synth 2048 23 none:               341148 / 655360, 258850, 6577
  synth 7001 262 none:              327686 / 655360, 272292, 35989
  synth 1000 6 middle clip:         95938 / 121358, 25420, 809
  plateau 64 2 none:                88294 / 131072, 41771, 64
  wide30 1 5 x in 0..2:             35298 / 65536, 30238, 24477
  clustered 1000 6 none:            975 / 327680, -, 73
  garbage_tail 2048 23 header box:  299943 / 327630, -, 0
Both classes are non-empty in every case, so neither mode can pass by writing everything or nothing."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import pcrhpg24_amd as P
from pcrhpg24_amd import _native as N
from pcrhpg24_amd import build
from tests import denoise_cases as D
from tests import oracle
from tests import select_cases as S
from tests import thin_cases as T
from tests.test_abi import declared

SYMBOLS = ("pcr_denoise", "pcr_read_denoise")
STATS = ["batches_outside", "batches_decoded", "points_considered", "runs", "voxels", "voxels_isolated", "points_isolated", "points_written",
         "table_slots"]


def test_entry_points_are_declared_bound_and_exported():
    for name in SYMBOLS:
        assert name in declared("pcr_hip.h") and name in N.HIP_SYMBOLS
    build.build_hip()
    lib = C.CDLL(build.HIP_LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    bound = N.hip_lib()
    args = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(N.Voxels), C.POINTER(N.Box), C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_int64), C.POINTER(N.DenoiseStats)]
    assert bound.pcr_denoise.argtypes == args and bound.pcr_read_denoise.argtypes == args
    for name in ("DenoiseStats", "DENOISE_KEEP", "DENOISE_ISOLATED"):
        assert hasattr(P, name)
    for name in ("denoise", "read_denoise"):
        assert callable(getattr(P.Context, name))
    assert callable(P.HuffmanLasData.denoised)


def test_struct_and_constants_match_the_header(tmp_path):
    """sizeof / offsetof and the constants as a C compiler sees include/pcr_types.h, against the ctypes mirror."""
    stats = [f for f, _ in N.DenoiseStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcr_types.h"\nint main(void) {\nprintf("%zu ", sizeof(pcr_denoise_stats));\n'
                   + "".join(f'printf("%zu ", offsetof(pcr_denoise_stats, {f}));\n' for f in stats)
                   + 'printf("%d %d\\n", PCR_DENOISE_KEEP, PCR_DENOISE_ISOLATED);\nreturn 0; }\n')
    subprocess.run(["gcc", "-I", build.INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert stats == STATS
    assert got[0] == 72 == C.sizeof(N.DenoiseStats) and got[1:10] == [8 * k for k in range(9)] == [getattr(N.DenoiseStats, f).offset for f in stats]
    assert got[10:] == [N.DENOISE_KEEP, N.DENOISE_ISOLATED] == [D.KEEP, D.ISOLATED] == [P.DENOISE_KEEP, P.DENOISE_ISOLATED] == [0, 1]


# ---- the lattice (csrc/pcr_lattice.h) in a program of its own ------------------------------------------------------------------
I32 = (S.INT32_MIN, S.INT32_MAX)
LATTICE_CASES = [
    # origin, cell, q.min, q.max
    ((0, 0, 0), 1, (0, 0, 0), (10, 10, 10)),
    ((0, 0, 0), 1, (-5, 3, 0), ((1 << 21) - 9, 3, 0)),                      # extent / cell + 4 = 2^21 exactly: accepted
    ((0, 0, 0), 1, (-5, 3, 0), ((1 << 21) - 8, 3, 0)),                      # one above: refused
    ((0, 0, 0), 7, (3, -5, 0), (3, -5 + 7 * ((1 << 21) - 4) + 6, 0)),       # the same at cell 7, with the largest remainder
    ((0, 0, 0), 7, (3, -5, 0), (3, -5 + 7 * ((1 << 21) - 3), 0)),
    ((-12345, 777, -1), 7001, (-1048562, -1048564, -67759), (1048571, 1048556, 68709)),
    ((I32[1], I32[0], 0), 64, (593, 593, 241), (999406, 999406, 74106)),    # origin'' beyond int32 on x and y
    ((I32[0], I32[1], 0), 1000, (I32[0], I32[1] - 5, 7), (I32[0] + 99999, I32[1], 7)),      # origins at both ends of int32, q at them
    ((I32[1], I32[0], 0), 1 << 30, (I32[0], 0, 0), (-2, 5, 5)),
    ((I32[0], I32[1], 5), 1 << 30, (I32[0], I32[0], I32[0]), (I32[1] - 1, -1, 0)),
    ((0, 0, 0), 1 << 30, (0, 0, I32[0] + 1), (0, 0, 0)),                    # extent 2^31 - 1 with cell 2^30: accepted, d up to 2^32 - 1
    ((0, 0, 0), 1 << 30, (0, 0, -1 - (1 << 30)), (0, 0, (1 << 30) - 2)),    # ... with q.min at a cell's last step: d reaches 2^32 - 2
    ((0, 0, 0), 1 << 30, (0, I32[0], 0), (0, 0, 0)),                        # extent 2^31 exactly: refused
    ((0, 0, 0), 1 << 30, (I32[0], 0, 0), (I32[1], 0, 0)),                   # extent 2^32 - 1
    ((5, -5, 17), 2047, (-100000, -100000, -100000), (100000, 100000, 100000)),
    ((5, -5, 17), 2048, (3, -5, 18), (3, -5, 18)),
]


def noise_lattice_by_hand(origin, cell, qmin, qmax):
    out = []
    for k in range(3):
        extent = qmax[k] - qmin[k]
        if extent >= 1 << 31:
            return [1, k]
        if extent // cell + 4 > 1 << 21:
            return [2, k]
        shifted = origin[k] + ((qmin[k] - origin[k]) // cell - 1) * cell    # Python's // is the floor
        # q.min lies in voxel 1, d fits 32 unsigned bits, and every neighbour index of a point in q lies in [0, 2^21)
        assert (qmin[k] - shifted) // cell == 1
        assert cell <= qmin[k] - shifted and qmax[k] - shifted < extent + 2 * cell and qmax[k] - shifted <= (1 << 32) - 1
        for p in (qmin[k], qmax[k]):
            v = (p - shifted) // cell
            assert 0 <= v - 1 and v + 1 < 1 << 21
        out.append(shifted % (1 << 32))
    pow2 = cell & (cell - 1) == 0
    return [0, 2] + out + [cell, cell.bit_length() - 1 if pow2 else 32, 0 if pow2 else -(-(1 << 64) // cell)]


def test_noise_lattice_shift_limits_and_divisor_against_python_integers(tmp_path):
    """noise_lattice() for origins and boxes at the edges of int32: the refusals, the shifted origin modulo 2^32, the divisor; and
    thin_lattice() on the same cases is one cell less of a shift (it has not changed)."""
    rows = ",\n".join("{{%d, %d, %d}, %d, {%d, %d, %d}, {%d, %d, %d}}" % (*o, c, *lo, *hi) for o, c, lo, hi in LATTICE_CASES)
    rows = rows.replace("-2147483648", "(-2147483647 - 1)")
    src = tmp_path / "lattice.cpp"
    src.write_text('#include <cstdio>\n#include "pcr_lattice.h"\nstruct Case { int32_t origin[3]; int32_t cell; int32_t lo[3], hi[3]; };\n'
                   'static const Case cases[] = {\n' + rows + '\n};\nint main() {\n  for (const Case &c : cases) {\n    ThinLattice l{}, t{}; int axis = -1, taxis = -1;\n'
                   '    const int rc = noise_lattice(c.origin, c.cell, c.lo, c.hi, &l, &axis);\n'
                   '    if (rc) { std::printf("%d %d\\n", rc, axis); continue; }\n'
                   '    std::printf("0 %d %u %u %u %u %u %llu", axis, l.origin[0], l.origin[1], l.origin[2], l.cell, l.div.shift, l.div.magic);\n'
                   '    if (thin_lattice(c.origin, c.cell, c.lo, c.hi, &t, &taxis) != 0) return 3;\n'
                   '    std::printf(" %u %u %u\\n", t.origin[0] - l.origin[0], t.origin[1] - l.origin[1], t.origin[2] - l.origin[2]);\n'
                   '  }\n  return 0;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-I", build.CSRC,
                    str(src), "-o", str(tmp_path / "lattice")], check=True)
    res = subprocess.run([str(tmp_path / "lattice")], check=True, stdout=subprocess.PIPE, text=True)
    got = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    want = [noise_lattice_by_hand(*case) for case in LATTICE_CASES]
    want = [w + [w[5]] * 3 if w[0] == 0 else w for w in want]               # thin's origin' - origin'' = one cell
    assert got == want
    assert sorted({w[0] for w in want}) == [0, 1, 2], "the cases reach both refusals and the accepted path"
    assert [w[0] for w in want[1:5]] == [0, 2, 0, 2], "2^21 exactly is accepted, one above refused"


@pytest.mark.parametrize("cell", [1000, 7001, 3, (1 << 30) - 1])
def test_the_cells_divide_exactly_up_to_the_largest_difference(cell):
    """d / cell by multiply-high for the largest d a denoising call can see, d <= 2^32 - 1."""
    magic = ((1 << 64) - 1) // cell + 1
    top = 1 << 32
    rng = np.random.default_rng(cell)
    mult = np.unique(np.concatenate([np.arange(0, 32), top // cell - np.arange(0, 32), rng.integers(0, top // cell + 1, 500)]))
    d = (mult[:, None] * cell + np.array([-1, 0, 1, cell - 1])[None, :]).ravel()
    for v in list(d[(d >= 0) & (d < top)]) + [top - 1]:
        assert (int(v) * magic) >> 64 == int(v) // cell, (cell, int(v))


# ---- the numpy reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_count", [0, 1, 5, 40, D.HUGE])
@pytest.mark.parametrize("vox", [(0, 0, 0, 1), (-3, 5, 1, 4), (S.INT32_MAX, S.INT32_MIN, 0, 7), (2, 2, 2, 6)])
def test_reference_against_a_plain_loop(vox, max_count):
    rng = np.random.default_rng(sum(vox) & 0xFFFF)
    xyz = rng.integers(-20, 21, (3000, 3))
    xyz[::7] = xyz[1::7][:len(xyz[::7])]                                    # exact duplicates
    clip = ((-15, -20, -18), (20, 12, 20))
    count, voxel = {}, {}
    for row, p in enumerate(xyz):
        p = [int(v) for v in p]
        if all(clip[0][k] <= p[k] <= clip[1][k] for k in range(3)):
            voxel[row] = tuple((p[k] - vox[k]) // vox[3] for k in range(3))
            count[voxel[row]] = count.get(voxel[row], 0) + 1
    n27 = {row: sum(count.get((v[0] + dx, v[1] + dy, v[2] + dz), 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)) for row, v in voxel.items()}
    an = D.analyse(xyz, vox, clip)
    assert an["rows"].tolist() == sorted(voxel) and an["n27"].tolist() == [n27[r] for r in sorted(voxel)]
    assert an["own"].tolist() == [count[voxel[r]] for r in sorted(voxel)]
    isolated = sorted(r for r in voxel if n27[r] <= max_count)
    kept = sorted(r for r in voxel if n27[r] > max_count)
    assert D.reference(xyz, vox, max_count, clip, D.ISOLATED).tolist() == isolated
    assert D.reference(xyz, vox, max_count, clip, D.KEEP).tolist() == kept
    assert D.reference(xyz, vox, max_count, clip, D.KEEP).dtype == np.int64 and len(voxel) > 1000
    assert D.voxel_stats(an, max_count) == (len(count), len({voxel[r] for r in isolated}), len(isolated))
    if vox[3] == 1 and max_count == 1:
        assert isolated and kept
    assert (max_count != 0 or not isolated) and (max_count != D.HUGE or not kept)


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    of = oracle.OracleFile(T.stream(name))
    return np.concatenate([S.oracle_points(of, b) for b in range(of.num_batches)]).astype(np.int64), S.oracle_bounds(of)


@pytest.mark.parametrize("name,cell,max_count,clip,needs", D.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cases_show_the_properties_claimed(name, cell, max_count, clip, needs):
    xyz, bounds = oracle_rows(name)
    vox, clip = (0, 0, 0, cell), D.case_clip(name, clip, xyz)
    assert D.lattice_refusal(bounds, vox, clip) is None
    got = D.properties(xyz, vox, max_count, clip)
    print(f"{name} cell {cell} max_count {max_count} clip {clip}: {got}")
    assert 0 < got["isolated"] < got["candidates"], "a mode could pass by writing everything or nothing"
    for k in needs:
        assert got[k] >= 1, f"{k}: no such row in this case"
    if name == "garbage_tail":
        assert (~S.in_box(xyz, clip)).sum() >= 1, "no row of the tail artefact lies outside the header's box"


def test_every_property_is_covered():
    assert set(D.PROPERTIES) == {k for c in D.CASES for k in c[4]}
    assert {c[0] for c in D.CASES} == {"synth", "plateau", "wide30", "clustered", "garbage_tail"}
    assert {1, 64, 1000, 2048, 1 << 30} == {c[0] for c in D.COMBOS} and {0, 1, 2} == {c[1] for c in D.COMBOS}


def test_lattice_limits_of_the_streams():
    """wide30 without a clip is refused as for pcr_thin; with the clip on its low cluster cell 1 is accepted."""
    _, wide = oracle_rows("wide30")
    assert D.lattice_refusal(wide, (0, 0, 0, 1)) == "voxels" and D.lattice_refusal(wide, (0, 0, 0, 1 << 20)) == "extent"
    assert D.lattice_refusal(wide, (0, 0, 0, 1), D.WIDE30_LOW) is None
    one = [[0, 0, 0, (1 << 21) - 4, 0, 0]]
    assert D.lattice_refusal(one, (0, 0, 0, 1)) is None and T.lattice_refusal(one, (0, 0, 0, 1)) is None
    one = [[0, 0, 0, (1 << 21) - 3, 0, 0]]
    assert D.lattice_refusal(one, (0, 0, 0, 1)) == "voxels" and T.lattice_refusal(one, (0, 0, 0, 1)) is None


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [["--denoise"], ["--denoise", "1"], ["--denoise", "x", "3"], ["--denoise", "0", "3"], ["--denoise", "-1", "3"],
                                  ["--denoise", "nan", "3"], ["--denoise", "1", "x"], ["--denoise", "1", "-1"], ["--denoise", "1", "2.5"],
                                  ["--denoise", "1", "99999999999999999999"], ["--denoise", "1", "3", "--isolate"],
                                  ["--denoise", "1", "3", "--isolated", "--isolated"], ["--denoise", "1", "3", "4"],
                                  ["--denoise", "1", "3", "--box", "0", "0", "0", "1", "1"], ["--denoise", "1", "3", "--center"],
                                  ["--denoise", "1", "3", "--box", "0", "0", "0", "1", "1", "1", "--box", "0", "0", "0", "1", "1", "1"]])
def test_cli_refuses_a_malformed_denoise_before_it_creates_a_context(tmp_path, args):
    build.build_tools()
    out = tmp_path / "out.las"
    res = subprocess.run([build.DECODE_BIN, str(tmp_path / "missing.huffman"), str(out), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert res.returncode == 2 and res.stderr.startswith("usage: pcr_decode") and "--denoise CELL MAXCOUNT" in res.stderr
    assert "pcr_create" not in res.stderr and "missing.huffman" not in res.stderr and not out.exists()
